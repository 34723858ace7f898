// dfx: the resampler in step form (dfx_stream_resampler_*): the polyphase bank of dfx_resampler applied call by call, with the samples a
// later call still needs carried in the handle.  A part of dfx_io.hip (included at its end).
//
// Contract.  With P = ceil(width / orig) * orig (the delay in input samples, a whole number of frames) the concatenated output of a row
// equals the whole-signal resampler applied to P zeros followed by the row's signal, cut to frames * nw samples, whatever the cut into
// calls.  Per row the handle keeps the last hist = P + width samples; output frame f of a call is the window [f orig, f orig + K) of
// [history | new input] (K = 2 width + orig; the last frame ends at m orig + 2 width <= hist + m orig because width <= P), and the
// new history is the last `hist` samples of that array.  Every output sample is one fmaf chain over k = 0 .. K-1 that starts at 0, so
// the samples do not depend on the cut, nor on which thread computes them.
//
// The history is double-buffered (read d_hist[cur], write d_hist[cur ^ 1], flip on the host): several workgroups may then work on
// one row's call (frame tiles), and none reads what another writes.
#pragma once

#define DFX_RS_LDS_FLOATS 12288 // window floats per workgroup (48 KB: inside the default dynamic LDS limit)
#define DFX_RS_MASK_ROWS 4096   // rows per launch of a masked call: the mask travels as 512 bytes of kernel arguments (no upload, no wait)
#define DFX_RS_RESET_IDS 512

struct DfxRsMask {
    unsigned bits[DFX_RS_MASK_ROWS / 32];   // bit k: row row0 + k sits the call out
};
struct DfxRsIds {
    int n;
    int id[DFX_RS_RESET_IDS];
};
struct DfxRsStepArgs {
    int64_t row0, row_end, x_stride, y_stride;   // the rows [row0, row_end) of this launch
    int frames, orig, nw, nw_pad, K, hist;
    int mt, rg, seg;                             // frames per tile (blockIdx.y), rows per workgroup, window floats per row in LDS
    int fw, jw;                                  // the workgroup's 4 waves: fw groups of 64 (row, frame) slots x jw groups of phase tiles
    int x_fmt, y_fmt, masked;                    // DFX_FMT_* of x and y
};

struct dfx_stream_resampler {
    const dfx_resampler *r = nullptr;
    int64_t rows = 0, max_in = 0;
    int P = 0, D = 0, hist = 0;
    float *d_hist[2] = {nullptr, nullptr};   // [rows, hist] each
    int cur = 0;
};

// G711: the instance that also knows the two G.711 formats (a call with codes on either side); float32 / int16 calls run the instance without them
template <bool G711>
static __device__ __forceinline__ float dfx_rs_load(const void *x, int fmt, int64_t i) {
    if (!G711) return fmt ? (float)static_cast<const int16_t *>(x)[i] * (1.0f / 32768.0f) : static_cast<const float *>(x)[i];
    if (fmt == DFX_FMT_F32) return static_cast<const float *>(x)[i];
    if (fmt == DFX_FMT_PCM16) return (float)static_cast<const int16_t *>(x)[i] * (1.0f / 32768.0f);
    return (float)dfx_g711_to_s16(static_cast<const uint8_t *>(x)[i], fmt - DFX_FMT_ULAW + DFX_G711_ULAW) * (1.0f / 32768.0f);
}

// Workgroup (g, t, z): rows [row0 + g rg, + rg) x frames [t mt, + mt); z splits the phase tiles further when the rows alone give the chip too few
// workgroups.  The rows' windows are staged in LDS (an inactive row: zeros, so its outputs are exact zeros).  As in dfx_k_resample a lane owns
// one output frame — here a (row, frame) slot of the workgroup, rg * mt <= 64 fw of them — and JT phases at a time in registers; the taps are
// wave-uniform (s_load through the scalar cache: wt is a __restrict__ parameter of its own), the samples come from LDS at stride orig
// between the frames of a row: 4 LDS reads per 4 JT FMAs.  Every accumulator is one fmaf chain over k = 0 .. K-1 (four taps per iteration,
// then the K % 4 last ones singly: no padded tap is ever multiplied with a sample outside the frame's window).  JT = 16, or 4 where the bank
// has at most 4 phases (the down-samplers to 8 / 16 kHz have one).  Tile (t = 0, z = 0) also writes the rows' new history (an inactive row's:
// a copy of the old one).  x and y are converted from and to their sample formats (DFX_FMT_*) in the loads and stores; the two G.711 forms live in
// an instance of their own (G711), so that the float32 / int16 instance keeps its registers.
template <int JT, bool G711>
__global__ void __launch_bounds__(256) dfx_k_resample_step(const void *__restrict__ x, void *__restrict__ y, const float *__restrict__ wt,
                                                           const float *__restrict__ hist_in, float *__restrict__ hist_out, DfxRsStepArgs A,
                                                           DfxRsMask M) {
    DFX_DYN_SMEM(float, xs);
    const int64_t r0 = A.row0 + (int64_t)blockIdx.x * A.rg;
    if (r0 >= A.row_end) return;
    const int nr = (int)(A.row_end - r0 < A.rg ? A.row_end - r0 : A.rg);
    const int f0 = (int)blockIdx.y * A.mt;
    const int mtc = A.frames - f0 < A.mt ? A.frames - f0 : A.mt;
    const int segc = (mtc - 1) * A.orig + A.K;   // <= A.seg
    const int tid = threadIdx.x;
    // one flat index over the rows' windows, eight loads in flight per lane before the first LDS store (a load -> store loop would wait out
    // one memory latency per element)
    const int total = nr * segc;
    auto window = [&](int idx, int &at) -> float {   // element idx of the staged windows: its LDS index and value
        const int r = idx / segc, i = idx - r * segc;
        const int64_t row = r0 + r;
        const int mk = (int)(row - A.row0);
        at = r * A.seg + i;
        if (A.masked && ((M.bits[mk >> 5] >> (mk & 31)) & 1u)) return 0.f;
        const int w = f0 * A.orig + i;   // index into [history | new input]
        return w < A.hist ? hist_in[row * A.hist + w] : dfx_rs_load<G711>(x, A.x_fmt, row * A.x_stride - A.hist + w);
    };
    for (int i0 = tid; i0 < total; i0 += 8 * 256) {
        float v[8];
        int at[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            at[u] = -1;
            v[u] = 0.f;
            if (i0 + 256 * u < total) v[u] = window(i0 + 256 * u, at[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (at[u] >= 0) xs[at[u]] = v[u];
    }
    if (blockIdx.y == 0 && blockIdx.z == 0)
        for (int idx = tid; idx < nr * A.hist; idx += 256) {
            const int r = idx / A.hist, i = idx - r * A.hist;
            const int64_t row = r0 + r, w = (int64_t)A.frames * A.orig + i;
            const int mk = (int)(row - A.row0);
            const bool off = A.masked && ((M.bits[mk >> 5] >> (mk & 31)) & 1u);
            const float *hr = hist_in + row * A.hist;
            hist_out[row * A.hist + i] = off ? hr[i] : (w < A.hist ? hr[w] : dfx_rs_load<G711>(x, A.x_fmt, row * A.x_stride - A.hist + w));
        }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int wf = dfx_wave_uniform(wave % A.fw), wj = dfx_wave_uniform(wave / A.fw);
    const int slots = nr * mtc;
    if (wf * 64 >= slots) return;
    const int sl = wf * 64 + lane;
    const bool live = sl < slots;
    const int sc = live ? sl : slots - 1;   // (a lane past the last slot recomputes it and stores nothing)
    const int r = sc / mtc, f = sc - r * mtc;
    const float *xp = xs + r * A.seg + f * A.orig;
    const int64_t yo = (r0 + r) * A.y_stride + (int64_t)(f0 + f) * A.nw;
    for (int j0 = ((int)blockIdx.z * A.jw + wj) * JT; j0 < A.nw; j0 += (int)gridDim.z * A.jw * JT) {
        float acc[JT];
#pragma unroll
        for (int i = 0; i < JT; ++i) acc[i] = 0.f;
        const float *wp = wt + j0;
        int k = 0;
        for (; k + 4 <= A.K; k += 4) {
            const float x0 = xp[k], x1 = xp[k + 1], x2 = xp[k + 2], x3 = xp[k + 3];
            const float *w0 = wp + (int64_t)k * A.nw_pad;
#pragma unroll
            for (int i = 0; i < JT; ++i) {
                float a = acc[i];
                a = fmaf(w0[i], x0, a);
                a = fmaf(w0[A.nw_pad + i], x1, a);
                a = fmaf(w0[2 * A.nw_pad + i], x2, a);
                a = fmaf(w0[3 * A.nw_pad + i], x3, a);
                acc[i] = a;
            }
        }
        for (; k < A.K; ++k) {
            const float x0 = xp[k];
            const float *w0 = wp + (int64_t)k * A.nw_pad;
#pragma unroll
            for (int i = 0; i < JT; ++i) acc[i] = fmaf(w0[i], x0, acc[i]);
        }
        if (!live) continue;
#pragma unroll
        for (int i = 0; i < JT; ++i) {
            if (j0 + i >= A.nw) continue;
            if (G711 ? A.y_fmt == DFX_FMT_PCM16 : A.y_fmt != DFX_FMT_F32) {   // dfx_k_f32_to_pcm16's encoding
                float v = acc[i] * 32768.0f;
                v = v != v ? 0.f : fminf(fmaxf(v, -9.0e18f), 9.0e18f);
                static_cast<int16_t *>(y)[yo + j0 + i] = (int16_t)(uint16_t)(uint64_t)(int64_t)v;
            } else if (!G711 || A.y_fmt == DFX_FMT_F32) {
                static_cast<float *>(y)[yo + j0 + i] = acc[i];
            } else {   // G.711: the saturating rule (dfx_g711.h); an inactive row's exact zeros come out as the law's silence code
                static_cast<uint8_t *>(y)[yo + j0 + i] = (uint8_t)dfx_s16_to_g711(dfx_f32_to_s16_sat(acc[i]), A.y_fmt - DFX_FMT_ULAW + DFX_G711_ULAW);
            }
        }
    }
}

// rows I.id[0 .. n) start over: both history buffers
__global__ void __launch_bounds__(256) dfx_k_resample_reset_rows(DfxRsIds I, float *h0, float *h1, int hist) {
    if ((int)blockIdx.x >= I.n) return;
    const int64_t o = (int64_t)I.id[blockIdx.x] * hist;
    for (int i = threadIdx.x; i < hist; i += 256) h0[o + i] = 0.f, h1[o + i] = 0.f;
}

extern "C" int dfx_stream_resampler_create(const dfx_resampler *r, int64_t rows, int64_t max_in_samples, dfx_stream_resampler **out) {
    if (!r || !out || rows <= 0 || rows > 0x7fffffff || max_in_samples <= 0)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_create: bad arguments");
    if (max_in_samples % r->orig)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_create: max_in_samples must be a multiple of the block (%d samples)", r->orig);
    if (max_in_samples > ((int64_t)1 << 30)) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_resampler_create: more than 2^30 samples per call");
    if (r->K > DFX_RS_LDS_FLOATS)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_resampler_create: rate ratio %d:%d has %d taps per phase (at most %d in the step form)", r->orig, r->nw,
                 r->K, DFX_RS_LDS_FLOATS);
    if (int rc = dfx_require_device()) return rc;
    dfx_stream_resampler *h = new dfx_stream_resampler();
    h->r = r, h->rows = rows, h->max_in = max_in_samples;
    h->P = (r->width + r->orig - 1) / r->orig * r->orig;
    h->D = h->P / r->orig * r->nw;
    h->hist = h->P + r->width;
    const size_t bytes = (size_t)rows * h->hist * 4;
    for (int i = 0; i < 2; ++i)
        if (hipMalloc(reinterpret_cast<void **>(&h->d_hist[i]), bytes) != hipSuccess || hipMemset(h->d_hist[i], 0, bytes) != hipSuccess) {
            for (int k = 0; k < 2; ++k)
                if (h->d_hist[k]) (void)hipFree(h->d_hist[k]);
            delete h;
            DFX_FAIL(DFX_ERR_ALLOC, "dfx_stream_resampler_create: device allocation of %zu bytes failed", bytes);
        }
    *out = h;
    return DFX_OK;
}

extern "C" void dfx_stream_resampler_free(dfx_stream_resampler *h) {
    if (!h) return;
    for (int i = 0; i < 2; ++i)
        if (h->d_hist[i]) (void)hipFree(h->d_hist[i]);
    delete h;
}

extern "C" int dfx_stream_resampler_delay(const dfx_stream_resampler *h, int64_t *in_samples, int64_t *out_samples) {
    if (!h) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_delay: null handle");
    if (in_samples) *in_samples = h->P;
    if (out_samples) *out_samples = h->D;
    return DFX_OK;
}

extern "C" int dfx_stream_resampler_reset(dfx_stream_resampler *h, const int64_t *rows, int64_t count, void *stream) {
    if (!h) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_reset: null handle");
    if (int rc = dfx_require_device()) return rc;
    hipStream_t s = dfx_stream(stream);
    if (!rows) {
        for (int i = 0; i < 2; ++i) DFX_HIP(hipMemsetAsync(h->d_hist[i], 0, (size_t)h->rows * h->hist * 4, s));
        return DFX_OK;
    }
    if (count < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_reset: negative count");
    for (int64_t i = 0; i < count; ++i)
        if (rows[i] < 0 || rows[i] >= h->rows)
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_reset: row %lld is not in [0, %lld)", (long long)rows[i], (long long)h->rows);
    for (int64_t i0 = 0; i0 < count; i0 += DFX_RS_RESET_IDS) {
        DfxRsIds I;
        I.n = (int)(count - i0 < DFX_RS_RESET_IDS ? count - i0 : DFX_RS_RESET_IDS);
        for (int i = 0; i < I.n; ++i) I.id[i] = (int)rows[i0 + i];
        dfx_launch(dfx_k_resample_reset_rows, dim3((unsigned)I.n), dim3(256), 0, s, I, h->d_hist[0], h->d_hist[1], h->hist);
        DFX_LAUNCH_CHECK();
    }
    return DFX_OK;
}

// The rows' histories for the model's stream export / import (dfx_stream_move.h): the buffer that is current, the one the next call writes, and
// the floats per row.  Internal (dfx_common.h): a stream's rows are moved by the table kernel that moves the rest of its state.
void dfx_stream_resampler_rows(const dfx_stream_resampler *h, float **cur, float **other, int *hist) {
    *cur = h->d_hist[h->cur], *other = h->d_hist[h->cur ^ 1], *hist = h->hist;
}

extern "C" int dfx_stream_resampler_process(dfx_stream_resampler *h, const void *x, int x_format, int64_t in_len, int64_t x_stride, void *y,
                                            int y_format, int64_t y_stride, const unsigned char *active_host, void *stream) {
    if (!h) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_process: null handle");
    if (x_format < DFX_FMT_F32 || x_format > DFX_FMT_ALAW || y_format < DFX_FMT_F32 || y_format > DFX_FMT_ALAW)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_process: sample formats %d, %d (DFX_FMT_F32 .. DFX_FMT_ALAW)", x_format, y_format);
    const dfx_resampler *r = h->r;
    if (in_len < 0 || in_len % r->orig)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_process: %lld input samples are not a multiple of the block (%d)", (long long)in_len, r->orig);
    if (in_len > h->max_in)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_process: %lld input samples, the handle was created for at most %lld", (long long)in_len,
                 (long long)h->max_in);
    const int64_t frames = in_len / r->orig, out_len = frames * r->nw;
    if (x_stride < in_len || y_stride < out_len) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_process: row stride shorter than the row");
    if (int rc = dfx_require_device()) return rc;
    if (frames == 0) return DFX_OK;
    if (!x || !y) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_resampler_process: null buffer");
    DfxRsStepArgs A;
    A.x_stride = x_stride, A.y_stride = y_stride;
    A.frames = (int)frames, A.orig = r->orig, A.nw = r->nw, A.nw_pad = r->nw_pad, A.K = r->K, A.hist = h->hist;
    A.x_fmt = x_format, A.y_fmt = y_format, A.masked = active_host != nullptr;
    // The 4 waves: jw of them split the phase tiles (as many as there are tiles: 1 / 2 / 4), fw = 4 / jw own 64 (row, frame) slots each.  A
    // workgroup takes up to 64 fw frames of a row (as many as the window has room for) and, where a call has fewer, as many rows as fill its
    // slots; nz: the phase tiles go over that many workgroups more when the rows give the chip fewer than ~1024 of them.
    const int jt = r->nw <= 4 ? 4 : DFX_RS_JT, ntiles = (r->nw + jt - 1) / jt;
    A.jw = ntiles >= 4 ? 4 : (ntiles >= 2 ? 2 : 1);
    A.fw = 4 / A.jw;
    const int64_t cap = 64 * A.fw, mt_max = (DFX_RS_LDS_FLOATS - r->K) / r->orig + 1;
    A.mt = (int)(frames < cap ? frames : cap);
    if (A.mt > mt_max) A.mt = (int)mt_max;
    A.seg = (A.mt - 1) * r->orig + r->K;
    int64_t rgl = cap / A.mt;
    if (rgl > DFX_RS_LDS_FLOATS / A.seg) rgl = DFX_RS_LDS_FLOATS / A.seg;
    if (rgl > h->rows) rgl = h->rows;
    A.rg = (int)(rgl > 1 ? rgl : 1);
    const size_t smem = (size_t)A.rg * A.seg * sizeof(float);
    const unsigned tiles = (unsigned)dfx_ceil_div(frames, A.mt);
    if (tiles > 65535) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_resampler_process: call too long");
    const int64_t wgs = dfx_ceil_div(h->rows, A.rg) * tiles, zmax = dfx_ceil_div(ntiles, A.jw), zwant = dfx_ceil_div(1024, wgs);
    const unsigned nz = (unsigned)(zwant < zmax ? zwant : zmax);
    const bool g711 = x_format >= DFX_FMT_ULAW || y_format >= DFX_FMT_ULAW;
    hipStream_t s = dfx_stream(stream);
    DfxKScope ks(DFX_K_RESAMPLE, s);
    DfxRsMask M;
    memset(M.bits, 0, sizeof(M.bits));
    const int64_t per = active_host ? DFX_RS_MASK_ROWS : h->rows;
    for (int64_t row0 = 0; row0 < h->rows; row0 += per) {
        A.row0 = row0, A.row_end = row0 + per < h->rows ? row0 + per : h->rows;
        if (active_host) {
            memset(M.bits, 0, sizeof(M.bits));
            for (int64_t k = row0; k < A.row_end; ++k)
                if (!active_host[k]) M.bits[(k - row0) >> 5] |= 1u << ((k - row0) & 31);
        }
        const dim3 grid((unsigned)dfx_ceil_div(A.row_end - row0, A.rg), tiles, nz);
        if (jt == 4 && g711)
            dfx_launch(dfx_k_resample_step<4, true>, grid, dim3(256), smem, s, (const void *)x, y, (const float *)r->d_wt,
                       (const float *)h->d_hist[h->cur], h->d_hist[h->cur ^ 1], A, M);
        else if (g711)
            dfx_launch(dfx_k_resample_step<DFX_RS_JT, true>, grid, dim3(256), smem, s, (const void *)x, y, (const float *)r->d_wt,
                       (const float *)h->d_hist[h->cur], h->d_hist[h->cur ^ 1], A, M);
        else if (jt == 4)
            dfx_launch(dfx_k_resample_step<4, false>, grid, dim3(256), smem, s, (const void *)x, y, (const float *)r->d_wt,
                       (const float *)h->d_hist[h->cur], h->d_hist[h->cur ^ 1], A, M);
        else
            dfx_launch(dfx_k_resample_step<DFX_RS_JT, false>, grid, dim3(256), smem, s, (const void *)x, y, (const float *)r->d_wt,
                       (const float *)h->d_hist[h->cur], h->d_hist[h->cur ^ 1], A, M);
        DFX_LAUNCH_CHECK();
    }
    h->cur ^= 1;
    return DFX_OK;
}
