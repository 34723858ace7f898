// dfx: scoring on the device — SI-SDR (df/evaluation_utils.py:599-619, si_sdr_speechmetrics) and STOI (df/stoi.py:163-231) of batches of clips.
// A part of dfx_io.hip.  Every row is scored as if it were alone: nothing a row computes depends on the rows around it, on the batch's padded
// length or on what the workspace held, and every sum is taken in an order fixed by the row's own length (no atomics).
//
// STOI of one row, after both signals were brought to 10 kHz (dfx_k_resample with the row's own length):
//   energy   256-sample windows at hop 128 over the clean signal padded by pad = 256 - n % 256 (front pad / 2, back the rest), window
//            hann(258)[1:-1]:  e[w] = 20 log10(|x_w| / 16 + eps)                                                            (stoi.py:58-76)
//   select   keep window w where max(e) - 40 - e[w] < 0; the kept indices in order (an exclusive scan), K of them            (stoi.py:79-83)
//            the silence-free signal has (K + 1) 128 samples; pad_front goes when window 0 was kept, pad_end when the last was (stoi.py:103-109);
//            n samples remain: n < 512 -> the row is skipped (NaN, J = 0); L = (n - 256) / 128 + 1 frames; J = L - 29 segments (L <= 30: one)
//   bands    frame l = samples trim_front + 128 l + [0, 256) of that signal, each the overlap-add of the (at most two) kept windows covering it
//            divided by the overlap-added window (stoi.py:85-100) — computed from the kept list, the signal is never stored —, times the
//            window, a 512-point transform (256 samples at offset 128 of 512 in the reference: a phase, which |X|^2 does not see), |X / sum(w)|^2
//            summed over the 15 third-octave bands of thirdoct(10000, 512, 15, 150), square root                           (stoi.py:198-205)
//   corr     per segment of 30 frames and band: normalise, clip at 1 + 10^(15/20), remove the means, divide by the norms, correlate
//            (stoi.py:213-225); block partial sums in float64, added in a fixed order, / (15 J)                              (stoi.py:230)
#pragma once

#define DFX_MT_ROWS 256          // rows per upload launch (kernel arguments, like dfx_launch_varlen_rows)
#define DFX_STOI_FS 10000
#define DFX_STOI_BANDS 15
#define DFX_STOI_SEG 30          // frames per segment (N)
#define DFX_STOI_WPB 32          // windows per workgroup of the energy kernel
#define DFX_STOI_FPB 16          // frames per workgroup of the band kernel
#define DFX_STOI_SPB 16          // segments per workgroup of the correlation kernel
#define DFX_STOI_EPS 2.220446049250313e-16f   /* np.finfo("float").eps, as float32 arithmetic sees it */
#define DFX_SISDR_TILE 4096      // samples per workgroup of the SI-SDR passes
#define DFX_F32_EPS 1.1920928955078125e-07f

struct DfxMtRows {
    int64_t *rows;     // [2][B]: samples, samples at 10 kHz (ceil(samples * nw / orig))
    int64_t B, row0;   // this launch's rows: row0 .. row0 + n - 1
    int n, orig, nw;
    int64_t len[DFX_MT_ROWS];
};
__global__ void __launch_bounds__(DFX_MT_ROWS) dfx_k_metric_rows(DfxMtRows A) {
    const int i = (int)threadIdx.x;
    if (i >= A.n) return;
    const int64_t b = A.row0 + i, n = A.len[i];
    A.rows[b] = n;
    A.rows[A.B + b] = (n * A.nw + A.orig - 1) / A.orig;
}

static int dfx_launch_metric_rows(const int64_t *lens, int64_t B, int64_t *rows, int orig, int nw, hipStream_t s) {
    for (int64_t r0 = 0; r0 < B; r0 += DFX_MT_ROWS) {
        DfxMtRows A;
        A.rows = rows;
        A.B = B, A.row0 = r0;
        A.n = (int)(B - r0 < DFX_MT_ROWS ? B - r0 : DFX_MT_ROWS);
        A.orig = orig, A.nw = nw;
        for (int i = 0; i < A.n; ++i) A.len[i] = lens[r0 + i];
        dfx_launch(dfx_k_metric_rows, dim3(1), dim3(DFX_MT_ROWS), 0, s, A);
        DFX_LAUNCH_CHECK();
    }
    return DFX_OK;
}

template <typename T>
static __device__ __forceinline__ T dfx_wave_sum(T v) {   // xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- SI-SDR -----------------------------------------------------------------------------------------------------------------------------------
// Two passes, as the reference: (1) rss = ref . ref and ref . est, a = (eps + ref . est) / (rss + eps) in float32; (2) sum (a ref)^2 and
// sum (est - a ref)^2 with the float32 products and differences the reference forms.  The sums are float64.
struct DfxSdrArgs {
    const float *ref, *est;
    int64_t stride, B, tiles;
    const int64_t *rows;   // [2][B]
    double *part;          // [B][tiles][2]
    double *ab;            // [B][2]: rss, ref . est
    float *out;            // [B]
};

template <int PASS>
__global__ void __launch_bounds__(256) dfx_k_sisdr_pass(DfxSdrArgs A) {
    __shared__ double red[2][4];
    const int64_t b = blockIdx.x / A.tiles, t = blockIdx.x - b * A.tiles;
    const int64_t n = A.rows[b], i0 = t * DFX_SISDR_TILE;
    if (i0 >= n && t > 0) return;   // (tile 0 always writes its partial: a row of no samples still has one)
    const float *r = A.ref + b * A.stride, *e = A.est + b * A.stride;
    float a = 0.f;
    if (PASS == 2) a = __fdiv_rn(__fadd_rn(DFX_F32_EPS, (float)A.ab[2 * b + 1]), __fadd_rn((float)A.ab[2 * b], DFX_F32_EPS));
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int u = 0; u < DFX_SISDR_TILE / 256; ++u) {
        const int64_t i = i0 + threadIdx.x + 256 * u;
        if (i < n) {
            const float rv = r[i], ev = e[i];
            if (PASS == 1) {
                s0 += (double)rv * (double)rv;
                s1 += (double)rv * (double)ev;
            } else {
                const float et = __fmul_rn(a, rv), er = __fadd_rn(ev, -et);
                s0 += (double)__fmul_rn(et, et);
                s1 += (double)__fmul_rn(er, er);
            }
        }
    }
    s0 = dfx_wave_sum(s0), s1 = dfx_wave_sum(s1);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[0][wave] = s0, red[1][wave] = s1;
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *q = red[threadIdx.x];
        A.part[(b * A.tiles + t) * 2 + threadIdx.x] = ((q[0] + q[1]) + q[2]) + q[3];
    }
}

// one wave per row: the row's tile partials, lane-strided and then the xor tree.  FINAL: 10 log10((eps + sss) / (eps + snn))
template <bool FINAL>
__global__ void __launch_bounds__(64) dfx_k_sisdr_reduce(DfxSdrArgs A) {
    const int64_t b = blockIdx.x, n = A.rows[b];
    int64_t nt = (n + DFX_SISDR_TILE - 1) / DFX_SISDR_TILE;
    if (nt < 1) nt = 1;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t t = threadIdx.x; t < nt; t += 64) {
        s0 += A.part[(b * A.tiles + t) * 2];
        s1 += A.part[(b * A.tiles + t) * 2 + 1];
    }
    s0 = dfx_wave_sum(s0), s1 = dfx_wave_sum(s1);
    if (threadIdx.x == 0) {
        if (FINAL)
            A.out[b] = (float)(10.0 * log10(((double)DFX_F32_EPS + s0) / ((double)DFX_F32_EPS + s1)));
        else
            A.ab[2 * b] = s0, A.ab[2 * b + 1] = s1;
    }
}

static int64_t dfx_align256(int64_t n) { return (n + 255) / 256 * 256; }

struct DfxSdrPlan {
    int64_t tiles, off_part, off_ab, bytes;   // rows at offset 0
};
static int dfx_sisdr_plan(int64_t B, const int64_t *lens, int64_t stride, DfxSdrPlan *P) {
    if (B < 0 || (B > 0 && !lens)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_si_sdr: bad arguments (B >= 0, lengths: a host array of B sample counts)");
    int64_t mx = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (lens[b] < 0 || (stride >= 0 && lens[b] > stride))
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_si_sdr: lengths[%lld] = %lld outside [0, stride]", (long long)b, (long long)lens[b]);
        if (lens[b] > mx) mx = lens[b];
    }
    P->tiles = dfx_ceil_div(mx, DFX_SISDR_TILE) > 0 ? dfx_ceil_div(mx, DFX_SISDR_TILE) : 1;
    if (B * P->tiles > 0x7fffffff) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_si_sdr: grid too large");
    P->off_part = dfx_align256(2 * B * 8);
    P->off_ab = P->off_part + dfx_align256(B * P->tiles * 16);
    P->bytes = P->off_ab + dfx_align256(B * 16);
    return DFX_OK;
}

extern "C" int dfx_si_sdr_workspace_bytes(int64_t B, const int64_t *lengths_host, int64_t *bytes) {
    if (!bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_si_sdr_workspace_bytes: null out");
    DfxSdrPlan P;
    if (int rc = dfx_sisdr_plan(B, lengths_host, -1, &P)) return rc;
    *bytes = P.bytes;
    return DFX_OK;
}

extern "C" int dfx_si_sdr(const float *ref, const float *est, int64_t B, int64_t stride, const int64_t *lengths_host, float *out, void *ws,
                          int64_t ws_bytes, void *stream) {
    if (stride < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_si_sdr: bad arguments");
    DfxSdrPlan P;
    if (int rc = dfx_sisdr_plan(B, lengths_host, stride, &P)) return rc;
    if (int rc = dfx_require_device()) return rc;
    if (B == 0) return DFX_OK;
    if (!ref || !est || !out || !ws || ((uintptr_t)ws & 15)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_si_sdr: null buffer (the workspace: 16-byte aligned)");
    if (ws_bytes < P.bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_si_sdr: workspace of %lld bytes, %lld needed (dfx_si_sdr_workspace_bytes)", (long long)ws_bytes, (long long)P.bytes);
    hipStream_t s = dfx_stream(stream);
    char *w = static_cast<char *>(ws);
    DfxSdrArgs A;
    A.ref = ref, A.est = est, A.stride = stride, A.B = B, A.tiles = P.tiles;
    A.rows = reinterpret_cast<int64_t *>(w), A.part = reinterpret_cast<double *>(w + P.off_part), A.ab = reinterpret_cast<double *>(w + P.off_ab);
    A.out = out;
    if (int rc = dfx_launch_metric_rows(lengths_host, B, reinterpret_cast<int64_t *>(w), 1, 1, s)) return rc;
    DfxKScope ks(DFX_K_SISDR, s);
    const dim3 g((unsigned)(B * P.tiles));
    dfx_launch(dfx_k_sisdr_pass<1>, g, dim3(256), 0, s, A);
    dfx_launch(dfx_k_sisdr_reduce<false>, dim3((unsigned)B), dim3(64), 0, s, A);
    dfx_launch(dfx_k_sisdr_pass<2>, g, dim3(256), 0, s, A);
    dfx_launch(dfx_k_sisdr_reduce<true>, dim3((unsigned)B), dim3(64), 0, s, A);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}

// ---- STOI -------------------------------------------------------------------------------------------------------------------------------------
struct DfxStoiTab {      // in the workspace, written by every call (dfx_k_stoi_tables)
    float win[256];      // hann(258)[1:-1]
    float2 tw[512];      // exp(-2 pi i k / 512)
    float inv_wsum;      // 1 / sum(win)
    int lo[DFX_STOI_BANDS], hi[DFX_STOI_BANDS];   // band b sums bins [lo, hi)
};
struct DfxStoiBands {
    int lo[DFX_STOI_BANDS], hi[DFX_STOI_BANDS];
};

// thirdoct(fs, nfft, num_bands, min_freq) (stoi.py:113-143) for (10000, 512, 15, 150): the nearest bin (first of equals, as np.argmin) to each
// band's lower and upper edge; the band is bins [lo, hi)
static void dfx_stoi_thirdoct(DfxStoiBands *t) {
    const double fs = DFX_STOI_FS, min_freq = 150.0;
    const int nfft = 512;
    auto nearest = [&](double f0) {
        int best = 0;
        double bd = 0.0;
        for (int i = 0; i <= nfft / 2; ++i) {
            const double f = (double)i * (fs / nfft), d = (f - f0) * (f - f0);
            if (i == 0 || d < bd) best = i, bd = d;
        }
        return best;
    };
    for (int k = 0; k < DFX_STOI_BANDS; ++k) {
        t->lo[k] = nearest(min_freq * std::pow(2.0, (2.0 * k - 1.0) / 6.0));
        t->hi[k] = nearest(min_freq * std::pow(2.0, (2.0 * k + 1.0) / 6.0));
    }
}

__global__ void __launch_bounds__(512) dfx_k_stoi_tables(DfxStoiTab *t, DfxStoiBands bands) {
    const int i = (int)threadIdx.x;
    const double pi = 3.14159265358979323846;
    const double a = -2.0 * pi * (double)i / 512.0;
    t->tw[i] = make_float2((float)cos(a), (float)sin(a));
    if (i < 256) t->win[i] = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)(i + 1) / 257.0));
    if (i == 256) {
        double s = 0.0;
        for (int k = 0; k < 256; ++k) s += (double)(float)(0.5 - 0.5 * cos(2.0 * pi * (double)(k + 1) / 257.0));
        t->inv_wsum = (float)(1.0 / (double)(float)s);
    }
#pragma unroll
    for (int k = 0; k < DFX_STOI_BANDS; ++k)
        if (i == 300 + k) t->lo[k] = bands.lo[k], t->hi[k] = bands.hi[k];
}

// the padding and the window count of a row of n samples at 10 kHz (stoi.py:58-61,72)
static __host__ __device__ __forceinline__ void dfx_stoi_geometry(int64_t n, int64_t *W, int *pad_front, int *pad_end) {
    const int pad = 256 - (int)(n % 256);
    *pad_front = pad / 2, *pad_end = pad - pad / 2;
    *W = (n + pad) / 128 - 1;
}

struct DfxStoiArgs {
    const float *clean, *degraded;   // at 10 kHz
    int64_t stride, B, Wmax;
    int64_t tilesE, tilesF, tilesJ;
    const int64_t *rows;             // [2][B]; rows[B + b]: samples at 10 kHz
    const DfxStoiTab *tab;
    float *e;                        // [B][Wmax]
    int *kept;                       // [B][Wmax]
    int *rowinfo;                    // [B][4]: K, L, J, trim_front
    float *env;                      // [B][2][Wmax][16]
    double *part;                    // [B][tilesJ]
    float *out;                      // [B]
    int *info;                       // null or [B][4]: windows, kept, L, J
};

// one wave per window: |x_w|, 4 samples a lane
__global__ void __launch_bounds__(256) dfx_k_stoi_energy(DfxStoiArgs A) {
    const int64_t b = blockIdx.x / A.tilesE, w0 = (blockIdx.x - b * A.tilesE) * DFX_STOI_WPB;
    const int64_t n = A.rows[A.B + b];
    int64_t W;
    int pf, pe;
    dfx_stoi_geometry(n, &W, &pf, &pe);
    if (w0 >= W) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *x = A.clean + b * A.stride;
    float wv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) wv[m] = A.tab->win[lane + 64 * m];
    for (int it = 0; it < DFX_STOI_WPB / 4; ++it) {
        const int64_t w = w0 + it * 4 + wave;
        if (w >= W) break;   // (the whole wave)
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int64_t j = w * 128 + lane + 64 * m - pf;
            const float v = __fmul_rn((j >= 0 && j < n) ? x[j] : 0.f, wv[m]);
            s = fmaf(v, v, s);
        }
        s = dfx_wave_sum(s);
        if (lane == 0) A.e[b * A.Wmax + w] = 20.f * log10f(__fadd_rn(__fdiv_rn(sqrtf(s), 16.f), DFX_STOI_EPS));
    }
}

// one workgroup per row, looping over the row: the maximum, then the kept windows' indices in order (ballot + prefix counts, 256 windows a step)
__global__ void __launch_bounds__(256) dfx_k_stoi_select(DfxStoiArgs A) {
    __shared__ float wmax[4];
    __shared__ int wcnt[4];
    const int64_t b = blockIdx.x, n = A.rows[A.B + b];
    int64_t W;
    int pf, pe;
    dfx_stoi_geometry(n, &W, &pf, &pe);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *e = A.e + b * A.Wmax;
    int *kept = A.kept + b * A.Wmax;
    float mx = -INFINITY;
    for (int64_t w = threadIdx.x; w < W; w += 256) mx = fmaxf(mx, e[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float thr = __fadd_rn(mx, -40.f);
    int64_t K = 0;
    for (int64_t c0 = 0; c0 < W; c0 += 256) {
        const int64_t w = c0 + threadIdx.x;
        const int keep = w < W && __fadd_rn(thr, -e[w]) < 0.f;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[wave] = __builtin_popcountll(m);
        __syncthreads();
        int64_t at = K;
        for (int v = 0; v < wave; ++v) at += wcnt[v];
        if (keep) kept[at + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (int)w;
        K += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool first = W > 0 && __fadd_rn(thr, -e[0]) < 0.f, last = W > 0 && __fadd_rn(thr, -e[W - 1]) < 0.f;
        const int tf = first ? pf : 0;
        const int64_t ns = (K + 1) * 128 - tf - (last ? pe : 0);
        int64_t L = 0, J = 0;
        if (K > 0 && ns >= 512) {
            L = (ns - 256) / 128 + 1;
            J = L > DFX_STOI_SEG ? L - (DFX_STOI_SEG - 1) : 1;
        }
        int *ri = A.rowinfo + 4 * b;
        ri[0] = (int)K, ri[1] = (int)L, ri[2] = (int)J, ri[3] = tf;
        if (A.info) {
            int *o = A.info + 4 * b;
            o[0] = (int)W, o[1] = (int)K, o[2] = (int)L, o[3] = (int)J;
        }
    }
}

static __device__ __forceinline__ float2 dfx_mt_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// one radix-4 Stockham pass of a 256-point complex transform, 64 lanes: NS = 1, 4, 16, 64
template <int NS>
static __device__ __forceinline__ void dfx_stoi_fft_pass(const float2 *in, float2 *out, const float2 *tw, int j) {
    const int k = j & (NS - 1);
    float2 v0 = in[j], v1 = in[j + 64], v2 = in[j + 128], v3 = in[j + 192];
    if (NS > 1) {
        const int m = k * (128 / NS);
        v1 = dfx_mt_cmul(v1, tw[m]), v2 = dfx_mt_cmul(v2, tw[2 * m]), v3 = dfx_mt_cmul(v3, tw[3 * m]);
    }
    const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
    const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y), a3 = make_float2(v1.y - v3.y, -(v1.x - v3.x));   // (v1 - v3) * -i
    const int j0 = ((j - k) << 2) + k;
    out[j0] = make_float2(a0.x + a2.x, a0.y + a2.y);
    out[j0 + NS] = make_float2(a1.x + a3.x, a1.y + a3.y);
    out[j0 + 2 * NS] = make_float2(a0.x - a2.x, a0.y - a2.y);
    out[j0 + 3 * NS] = make_float2(a1.x - a3.x, a1.y - a3.y);
}

// Workgroup = DFX_STOI_FPB frames of one signal of one row, one wave per frame at a time.  The 256 real samples of a frame are packed as 128
// complex values (zero-padded to 256: the 512-point real transform as a 256-point complex one and a split), transformed in LDS, and the
// bins' powers summed per band by four lanes a band.
__global__ void __launch_bounds__(256) dfx_k_stoi_bands(DfxStoiArgs A) {
    __shared__ float2 tw[512];
    __shared__ float win[256];
    __shared__ float2 bufa[4][256], bufb[4][256];
    const int64_t tile = blockIdx.x % A.tilesF, bs = blockIdx.x / A.tilesF, b = bs >> 1;
    const int sig = (int)(bs & 1);
    const int *ri = A.rowinfo + 4 * b;
    const int64_t K = ri[0], L = ri[1], f0 = tile * DFX_STOI_FPB;
    if (f0 >= L) return;
    const int tf = ri[3];
    const int64_t n = A.rows[A.B + b];
    int64_t W;
    int pf, pe;
    dfx_stoi_geometry(n, &W, &pf, &pe);
    const float *x = (sig ? A.degraded : A.clean) + b * A.stride;
    const int *kept = A.kept + b * A.Wmax;
    for (int i = threadIdx.x; i < 512; i += 256) tw[i] = A.tab->tw[i];
    win[threadIdx.x] = A.tab->win[threadIdx.x];
    const float inv = A.tab->inv_wsum;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int lo = 0, hi = 0;
    if (lane < 4 * DFX_STOI_BANDS) {
        const int band = lane >> 2, q = lane & 3, l0 = A.tab->lo[band], len = A.tab->hi[band] - l0;
        lo = l0 + len * q / 4, hi = l0 + len * (q + 1) / 4;
    }
    float2 *za = bufa[wave], *zb = bufb[wave];
    __syncthreads();
    for (int it = 0; it < DFX_STOI_FPB / 4; ++it) {
        const int64_t l = f0 + it * 4 + wave;
        const bool active = l < L;
        // sample i of the frame: position p of the silence-free signal = kept window p / 128 at offset p % 128 and the one before it at + 128
        float xs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = 2 * (lane + 64 * (u >> 1)) + (u & 1);
            float v = 0.f;
            if (active) {
                const int64_t p = tf + l * 128 + i, q = p >> 7;
                const int r = (int)(p & 127);
                float num = 0.f, den = 0.f;
                if (q < K) {
                    const int64_t j = (int64_t)kept[q] * 128 + r - pf;
                    num = __fmul_rn((j >= 0 && j < n) ? x[j] : 0.f, win[r]);
                    den = win[r];
                }
                if (q >= 1) {
                    const int64_t j = (int64_t)kept[q - 1] * 128 + r + 128 - pf;
                    num = __fadd_rn(__fmul_rn((j >= 0 && j < n) ? x[j] : 0.f, win[r + 128]), num);
                    den = __fadd_rn(win[r + 128], den);
                }
                v = __fmul_rn(__fdiv_rn(num, den), win[i]);
            }
            xs[u] = v;
        }
        za[lane] = make_float2(xs[0], xs[1]);
        za[lane + 64] = make_float2(xs[2], xs[3]);
        za[lane + 128] = make_float2(0.f, 0.f);
        za[lane + 192] = make_float2(0.f, 0.f);
        __syncthreads();
        dfx_stoi_fft_pass<1>(za, zb, tw, lane);
        __syncthreads();
        dfx_stoi_fft_pass<4>(zb, za, tw, lane);
        __syncthreads();
        dfx_stoi_fft_pass<16>(za, zb, tw, lane);
        __syncthreads();
        dfx_stoi_fft_pass<64>(zb, za, tw, lane);
        __syncthreads();
        // X[k] = (Z[k] + conj Z[256 - k]) / 2 - i / 2 exp(-2 pi i k / 512) (Z[k] - conj Z[256 - k]);  power of X / sum(w)
        float *pw = reinterpret_cast<float *>(zb);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = lane + 64 * m;
            const float2 z = za[k], zc = za[(256 - k) & 255];
            const float2 ev = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
            const float2 od = dfx_mt_cmul(make_float2(0.5f * (z.y + zc.y), -0.5f * (z.x - zc.x)), tw[k]);
            const float re = (ev.x + od.x) * inv, im = (ev.y + od.y) * inv;
            pw[k] = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
        }
        __syncthreads();
        float s = 0.f;
        for (int k = lo; k < hi; ++k) s += pw[k];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (active && lane < 4 * DFX_STOI_BANDS && (lane & 3) == 0) A.env[((b * 2 + sig) * A.Wmax + l) * 16 + (lane >> 2)] = sqrtf(s);
        __syncthreads();
    }
}

// Workgroup = DFX_STOI_SPB segments of one row; a thread = one band of one segment (stoi.py:213-225 in their order); the frames' envelopes in LDS
#define DFX_STOI_CF (DFX_STOI_SPB + DFX_STOI_SEG - 1)
__global__ void __launch_bounds__(256) dfx_k_stoi_corr(DfxStoiArgs A) {
    __shared__ float xe[2][DFX_STOI_CF * 16];
    __shared__ double red[4];
    const int64_t b = blockIdx.x / A.tilesJ, t = blockIdx.x - b * A.tilesJ;
    const int *ri = A.rowinfo + 4 * b;
    const int64_t L = ri[1], J = ri[2], j0 = t * DFX_STOI_SPB;
    if (j0 >= J) return;
    const int nf = L > DFX_STOI_SEG ? DFX_STOI_SEG : (int)L;             // frames of a segment
    const int nload = (int)(L - j0 < DFX_STOI_CF ? L - j0 : DFX_STOI_CF);
    for (int i = threadIdx.x; i < 2 * nload * 16; i += 256) {
        const int s = i / (nload * 16), r = i - s * nload * 16;
        xe[s][r] = A.env[((b * 2 + s) * A.Wmax + j0) * 16 + r];
    }
    __syncthreads();
    const int seg = threadIdx.x / DFX_STOI_BANDS, band = threadIdx.x - seg * DFX_STOI_BANDS;
    double c = 0.0;
    if (seg < DFX_STOI_SPB && j0 + seg < J) {
        const float *xp = xe[0] + seg * 16 + band, *yp = xe[1] + seg * 16 + band;
        const float clip = 6.623413251903491f;   // 1 + 10^(15/20)
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < nf; ++i) {
            const float xv = xp[16 * i], yv = yp[16 * i];
            sx += (double)xv * xv, sy += (double)yv * yv;
        }
        const float norm = __fdiv_rn(sqrtf((float)sx), __fadd_rn(sqrtf((float)sy), DFX_STOI_EPS));
        double mx = 0.0, my = 0.0;
        for (int i = 0; i < nf; ++i) {
            const float xv = xp[16 * i];
            mx += xv, my += fminf(__fmul_rn(yp[16 * i], norm), __fmul_rn(xv, clip));
        }
        const float mxf = (float)(mx / nf), myf = (float)(my / nf);
        sx = 0.0, sy = 0.0;
        for (int i = 0; i < nf; ++i) {
            const float xv = xp[16 * i], xc = __fadd_rn(xv, -mxf);
            const float yc = __fadd_rn(fminf(__fmul_rn(yp[16 * i], norm), __fmul_rn(xv, clip)), -myf);
            sx += (double)xc * xc, sy += (double)yc * yc;
        }
        const float dx = __fadd_rn(sqrtf((float)sx), DFX_STOI_EPS), dy = __fadd_rn(sqrtf((float)sy), DFX_STOI_EPS);
        for (int i = 0; i < nf; ++i) {
            const float xv = xp[16 * i], xc = __fadd_rn(xv, -mxf);
            const float yc = __fadd_rn(fminf(__fmul_rn(yp[16 * i], norm), __fmul_rn(xv, clip)), -myf);
            c += (double)__fmul_rn(__fdiv_rn(xc, dx), __fdiv_rn(yc, dy));
        }
    }
    c = dfx_wave_sum(c);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) A.part[b * A.tilesJ + t] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per row: the segment tiles' partial sums in a fixed order, / (15 J); a skipped row: NaN
__global__ void __launch_bounds__(64) dfx_k_stoi_final(DfxStoiArgs A) {
    const int64_t b = blockIdx.x, J = A.rowinfo[4 * b + 2];
    const int64_t nt = (J + DFX_STOI_SPB - 1) / DFX_STOI_SPB;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < nt; t += 64) s += A.part[b * A.tilesJ + t];
    s = dfx_wave_sum(s);
    if (threadIdx.x == 0) A.out[b] = J > 0 ? (float)(s / (double)(DFX_STOI_BANDS * J)) : __int_as_float(0x7fc00000);
}

struct DfxStoiPlan {
    int orig, nw;                 // fs_source : 10000 after dividing by their gcd
    int64_t Tmax, S10, Wmax, tilesE, tilesF, tilesJ;
    int64_t off_tab, off_rowinfo, off_rs, off_e, off_kept, off_env, off_part, bytes;   // rows at offset 0
};
static int dfx_stoi_plan(int fs_source, int64_t B, const int64_t *lens, int64_t stride, DfxStoiPlan *P) {
    if (fs_source <= 0 || B < 0 || (B > 0 && !lens))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi: bad arguments (fs_source > 0, B >= 0, lengths: a host array of B sample counts)");
    const int64_t g = gcd64(fs_source, DFX_STOI_FS);
    P->orig = (int)(fs_source / g), P->nw = (int)(DFX_STOI_FS / g);
    int64_t mx = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (lens[b] < 0 || (stride >= 0 && lens[b] > stride))
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi: lengths[%lld] = %lld outside [0, stride]", (long long)b, (long long)lens[b]);
        if (lens[b] > mx) mx = lens[b];
    }
    if (mx > ((int64_t)1 << 36)) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stoi: a row of more than 2^36 samples");
    P->Tmax = mx;
    const int64_t n10 = (mx * P->nw + P->orig - 1) / P->orig;
    int pf, pe;
    dfx_stoi_geometry(n10, &P->Wmax, &pf, &pe);
    P->S10 = (n10 + 3) / 4 * 4;
    P->tilesE = dfx_ceil_div(P->Wmax, DFX_STOI_WPB);
    P->tilesF = dfx_ceil_div(P->Wmax, DFX_STOI_FPB);
    P->tilesJ = dfx_ceil_div(P->Wmax, DFX_STOI_SPB);
    if (2 * B * P->tilesF > 0x7fffffff) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stoi: grid too large");
    int64_t at = dfx_align256(2 * B * 8);
    P->off_tab = at, at += dfx_align256((int64_t)sizeof(DfxStoiTab));
    P->off_rowinfo = at, at += dfx_align256(B * 16);
    P->off_rs = at, at += P->orig != P->nw ? dfx_align256(2 * B * P->S10 * 4) : 0;
    P->off_e = at, at += dfx_align256(B * P->Wmax * 4);
    P->off_kept = at, at += dfx_align256(B * P->Wmax * 4);
    P->off_env = at, at += dfx_align256(B * 2 * P->Wmax * 64);
    P->off_part = at, at += dfx_align256(B * P->tilesJ * 8);
    P->bytes = at;
    return DFX_OK;
}

extern "C" int dfx_stoi_workspace_bytes(int fs_source, int64_t B, const int64_t *lengths_host, int64_t *bytes) {
    if (!bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi_workspace_bytes: null out");
    DfxStoiPlan P;
    if (int rc = dfx_stoi_plan(fs_source, B, lengths_host, -1, &P)) return rc;
    *bytes = P.bytes;
    return DFX_OK;
}

extern "C" int dfx_stoi(const dfx_resampler *r, const float *clean, const float *degraded, int64_t B, int64_t stride, const int64_t *lengths_host,
                        float *out, int32_t *info, void *ws, int64_t ws_bytes, void *stream) {
    if (stride < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi: bad arguments");
    if (r && r->new_sr != DFX_STOI_FS) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi: the resampler must convert to %d Hz, not %d", DFX_STOI_FS, r->new_sr);
    DfxStoiPlan P;
    if (int rc = dfx_stoi_plan(r ? r->orig_sr : DFX_STOI_FS, B, lengths_host, stride, &P)) return rc;
    if (int rc = dfx_require_device()) return rc;
    if (B == 0) return DFX_OK;
    if (!clean || !degraded || !out || !ws || ((uintptr_t)ws & 15)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi: null buffer (the workspace: 16-byte aligned)");
    if (ws_bytes < P.bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stoi: workspace of %lld bytes, %lld needed (dfx_stoi_workspace_bytes)", (long long)ws_bytes, (long long)P.bytes);
    hipStream_t s = dfx_stream(stream);
    char *w = static_cast<char *>(ws);
    int64_t *rows = reinterpret_cast<int64_t *>(w);
    if (int rc = dfx_launch_metric_rows(lengths_host, B, rows, P.orig, P.nw, s)) return rc;
    DfxStoiArgs A;
    A.clean = clean, A.degraded = degraded, A.stride = stride;
    if (P.orig != P.nw) {   // both signals to 10 kHz, every row with its own length
        float *rs = reinterpret_cast<float *>(w + P.off_rs);
        if (int rc = dfx_resample_rows(r, clean, B, P.Tmax, stride, rs, P.S10, rows, stream)) return rc;
        if (int rc = dfx_resample_rows(r, degraded, B, P.Tmax, stride, rs + B * P.S10, P.S10, rows, stream)) return rc;
        A.clean = rs, A.degraded = rs + B * P.S10, A.stride = P.S10;
    }
    A.B = B, A.Wmax = P.Wmax, A.tilesE = P.tilesE, A.tilesF = P.tilesF, A.tilesJ = P.tilesJ;
    A.rows = rows;
    DfxStoiTab *tab = reinterpret_cast<DfxStoiTab *>(w + P.off_tab);
    A.tab = tab;
    A.e = reinterpret_cast<float *>(w + P.off_e), A.kept = reinterpret_cast<int *>(w + P.off_kept);
    A.rowinfo = reinterpret_cast<int *>(w + P.off_rowinfo), A.env = reinterpret_cast<float *>(w + P.off_env);
    A.part = reinterpret_cast<double *>(w + P.off_part), A.out = out, A.info = info;
    DfxStoiBands bands;
    dfx_stoi_thirdoct(&bands);
    dfx_launch(dfx_k_stoi_tables, dim3(1), dim3(512), 0, s, tab, bands);
    {
        DfxKScope ks(DFX_K_STOI_ENERGY, s);
        dfx_launch(dfx_k_stoi_energy, dim3((unsigned)(B * P.tilesE)), dim3(256), 0, s, A);
    }
    {
        DfxKScope ks(DFX_K_STOI_SELECT, s);
        dfx_launch(dfx_k_stoi_select, dim3((unsigned)B), dim3(256), 0, s, A);
    }
    {
        DfxKScope ks(DFX_K_STOI_BANDS, s);
        dfx_launch(dfx_k_stoi_bands, dim3((unsigned)(2 * B * P.tilesF)), dim3(256), 0, s, A);
    }
    {
        DfxKScope ks(DFX_K_STOI_CORR, s);
        dfx_launch(dfx_k_stoi_corr, dim3((unsigned)(B * P.tilesJ)), dim3(256), 0, s, A);
        dfx_launch(dfx_k_stoi_final, dim3((unsigned)B), dim3(64), 0, s, A);
    }
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}
