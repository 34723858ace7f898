// dfx: enhance() as one C call (dfx_enhance / dfx_enhance_pcm16, and dfx_enhance_varlen[_pcm16] for clips of different lengths: workspace
// plan, STFT features, forward pass with the fused finishing kernel).
// A part of dfx_model.hip (one translation unit: included from there, in this order — launch helpers, forward pass, streaming, enhance()).
#pragma once

// ------------------------------------------------------------------------------------------------ enhance()
// row stride (complex elements) of enhance()'s spec / spec_e buffers: F rounded up to a multiple of 8 = rows that start on a
// 64-byte boundary (F = 481 -> 488): every access of the row-streaming deep-filter kernel is then a 16-byte access inside whole
// 64-byte sectors.  Measured (tools/dev/dfa_bench.hip, profiles/r02_dfa_bench.log): stride 481 (flat-stream kernel) 4.9 TB/s,
// 482 -> 6.0, 488 / 496 / 512 -> 6.2 TB/s.
static inline int64_t enh_spec_stride(const dfx_state *st) {
    const int64_t F = (int64_t)st->N / 2 + 1;
    return (F + 7) & ~(int64_t)7;
}
namespace {
struct EnhWs {
    size_t spec, spec_e, feat_erb, feat_spec, model, total;  // bytes
};
EnhWs plan_enh(const dfx_model *m, const dfx_state *st, int64_t B, int64_t T, int pad) {
    EnhWs w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const int64_t Tp = pad ? T + st->N : T, Tf = Tp / st->hop, F = enh_spec_stride(st);
    w.spec = take((size_t)B * Tf * F * 8);
    w.spec_e = take((size_t)B * Tf * F * 8);
    w.feat_erb = take((size_t)B * Tf * m->cfg.nb_erb * 4);
    w.feat_spec = take((size_t)B * Tf * m->cfg.nb_df * 8);
    int64_t mb = 0;
    dfx_model_workspace_bytes(m, B, Tf, &mb);
    w.model = take((size_t)mb);
    w.total = off + 256;
    return w;
}
}  // namespace

// Clips of different lengths (dfx_enhance_varlen).  Every row runs the Tf frames of the pass's longest row, and frames t >= Tf_b of row b may
// hold anything without reaching frames < Tf_b: every stage between the features and the finishing kernel is causal in time (time convolutions
// pad at the front, forward GRUs, df_convp and the norm scans look back only), the network's lookahead enters only through the features and
// the deep filter's only through the spectrum.  So a row gets the bits of a pass of its own when (1) the STFT reads its samples [0, len_b) and
// zeros behind them, (2) its spectrum and normalised features are zero from frame Tf_b on — MF.DF's zero padding behind a clip
// (multiframe.py:72-76) and pad_feat's (deepfilternet3.py:359,409-410) — and (3) its output holds out_len_b samples, then zeros: output hop k
// depends only on frames <= k (lib.rs:396-427).  (1) is the VL instance of the analysis kernel; (2) and (3) are one dfx_k_zero_tails launch
// each, behind the features and behind the finishing kernels, and only where a row is shorter than the pass: the norm scans and the finishing
// kernels are the uniform ones.  The per-row metadata sits in front of the chunks' workspaces: [3][B] int64 (dfx_k_varlen_rows).
static inline size_t enh_rows_bytes(int64_t B) { return ((size_t)B * 3 * sizeof(int64_t) + 255) & ~(size_t)255; }
struct EnhRows {
    const int64_t *len = nullptr, *frames = nullptr;   // device, the chunk's rows (null: the uniform pass)
    bool short_frames = false;                         // a row of the chunk has fewer frames than the pass
};

static int enh_chunks(const dfx_model *m, int64_t B, int64_t *sizes) {
    int nc = 1;
    if (m->concurrent && m->max_chunks > 1) {
        const int64_t groups = dfx_ceil_div(B, 16);
        nc = (int)(groups / 2 < m->max_chunks ? groups / 2 : m->max_chunks);  // at least 32 clips per chunk
        if (nc < 1) nc = 1;
    }
    const int64_t groups = dfx_ceil_div(B, 16);
    int64_t done = 0;
    for (int c = 0; c < nc; ++c) {
        int64_t g = groups / nc + (c < groups % nc ? 1 : 0);
        int64_t n = g * 16;
        if (done + n > B) n = B - done;
        sizes[c] = n;
        done += n;
    }
    return nc;
}

extern "C" int dfx_enhance_workspace_bytes(const dfx_model *m, const dfx_state *st, int64_t B, int64_t T, int pad, int64_t *bytes) {
    if (!m || !st || !bytes || B < 0 || T < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance_workspace_bytes: bad arguments");
    // sized for the finest chunking the handle may use, so toggling dfx_model_set_streams never needs a bigger workspace
    int64_t sizes[DFX_MAX_LANES];
    int64_t total = (int64_t)plan_enh(m, st, B, T, pad).total;
    if (m->max_chunks > 1) {
        const bool was = m->concurrent;
        const_cast<dfx_model *>(m)->concurrent = true;
        const int nc = enh_chunks(m, B, sizes);
        const_cast<dfx_model *>(m)->concurrent = was;
        int64_t sum = 0;
        for (int c = 0; c < nc; ++c) sum += (int64_t)plan_enh(m, st, sizes[c], T, pad).total;
        if (sum > total) total = sum;
    }
    *bytes = total;
    return DFX_OK;
}

// pcm16: x and y point at int16_t samples (same strides in samples); the conversions of df/io.py run in the STFT kernel's loads and the
// ISTFT kernel's stores
static int enhance_chunk(const dfx_model *m, const dfx_state *st, const float *x, int64_t B, int64_t T, int pad, float lim,
                         float *y, unsigned char *base, hipStream_t s, const DfxLane *ln, bool signal_front, bool pcm16,
                         int64_t x_stride, int64_t y_stride, const EnhRows &rows) {
    const dfx_model_cfg &c = m->cfg;
    const EnhWs w = plan_enh(m, st, B, T, pad);
    const int64_t Tp = pad ? T + st->N : T, Tf = Tp / st->hop;
    float *spec = reinterpret_cast<float *>(base + w.spec), *spec_e = reinterpret_cast<float *>(base + w.spec_e);
    float *fe = reinterpret_cast<float *>(base + w.feat_erb), *fs = reinterpret_cast<float *>(base + w.feat_spec);
    // F.pad(audio, (0, n_fft)) (enhance.py:230-233) is implicit: the analysis reads zeros past the T samples of a row
    const int64_t sstride = enh_spec_stride(st);
    // the pre-split copy of feat_spec for the c0 kernels of the pass (can.c0_presplit) comes out of the norm scan, into its slot of the model workspace
    int64_t mb = 0;
    dfx_model_workspace_bytes(m, B, Tf, &mb);
    void *fps = m->can.c0_presplit ? dfx_ws_base(base + w.model) + plan_ws(m, B * Tf, B).fps : nullptr;
    const bool fs_unread = fps && Tf >= 16 && dfx_feat_spec_unread(m, B, Tf);   // (Tf < 16: the one-lane scan, the copy is made from its fp32 output)
    int rc = dfx_features_padded(st, x, B, Tp, T, x_stride, c.nb_df, c.norm_alpha, spec, fe, fs_unread ? nullptr : fs, (void *)s, sstride, pcm16, rows.len, fps,
                                 m->d_err);
    if (rc) return rc;
    if (rows.short_frames) {   // (2) above: spectrum and features of the frames behind a shorter row's end
        DfxTails t;
        t.add(spec, Tf * sstride * 2, Tf * sstride * 2, sstride * 2);
        t.add(fe, Tf * c.nb_erb, Tf * c.nb_erb, c.nb_erb);
        // the pre-split copy like feat_spec (zero words are the halves of 0.f): in its place where the fp32 values are not written, else a launch of its own
        t.add(fs_unread ? fps : fs, Tf * c.nb_df * 2, Tf * c.nb_df * 2, c.nb_df * 2);
        if ((rc = dfx_launch_zero_tails(t, rows.frames, B, s))) return rc;
        if (fps && !fs_unread) {
            DfxTails tp;
            tp.add(fps, Tf * c.nb_df * 2, Tf * c.nb_df * 2, c.nb_df * 2);
            if ((rc = dfx_launch_zero_tails(tp, rows.frames, B, s))) return rc;
        }
    }
    // the synthesis is enqueued by the model forward (per time chunk when the GRU phase is pipelined); with pad it stores exactly
    // the window audio[:, d : orig_len + d] of enhance.py:248-249
    DfxFinish fin;
    fin.st = st;
    fin.y = y;
    fin.out_stride = y_stride;
    fin.out_skip = pad ? st->N - st->hop : 0;
    fin.out_len = pad ? T : Tf * st->hop;
    fin.spec_stride = sstride;
    fin.out_i16 = pcm16;
    fin.feat_ps_made = fps != nullptr;
    return model_forward_lane(m, st->bands, spec, fe, fs, B, Tf, lim, spec_e, nullptr, nullptr, nullptr, base + w.model, mb, (void *)s, ln,
                              signal_front, &fin);
}

// lens (dfx_enhance_varlen): host [B], the samples of every row, T their maximum; rows of x / y x_stride / y_stride apart.  Null: the uniform pass
// (rows T / its output apart).
static int enhance_any(const dfx_model *m, const dfx_state *st, const float *x, int64_t B, int64_t T, int pad,
                       float atten_lim_db, float *y, void *workspace, int64_t workspace_bytes, void *stream, bool pcm16,
                       const int64_t *lens = nullptr, int64_t x_stride = 0, int64_t y_stride = 0) {
    if (!m || !st || B < 0 || T < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance: bad arguments");
    const dfx_model_cfg &c = m->cfg;
    if (st->N != c.fft_size || st->hop != c.hop_size || st->nb != c.nb_erb)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance: DF state does not match the model configuration");
    if (pad && st->N % st->hop) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance: pad requires fft_size %% hop_size == 0 (enhance.py:247)");
    const int64_t Tp = pad ? T + st->N : T, Tf = Tp / st->hop;
    const int64_t out_len = pad ? T : Tf * st->hop;
    const int64_t xs = lens ? x_stride : T, ys = lens ? y_stride : out_len;
    if (lens && (xs < T || ys < out_len))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance_varlen: x_stride %lld / y_stride %lld below the longest clip (%lld) / its output (%lld)",
                 (long long)xs, (long long)ys, (long long)T, (long long)out_len);
    if (int rc = dfx_require_device()) return rc;
    if (B == 0) return DFX_OK;
    if (!x || !y || !workspace) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance: null buffer");
    int64_t sizes[DFX_MAX_LANES];
    const int nc = enh_chunks(m, B, sizes);
    int64_t need = lens ? (int64_t)enh_rows_bytes(B) : 0;
    for (int i = 0; i < nc; ++i) need += (int64_t)plan_enh(m, st, sizes[i], T, pad).total;
    if (workspace_bytes < need) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance: workspace too small");
    unsigned char *base = reinterpret_cast<unsigned char *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipStream_t s = dfx_stream(stream);
    if (Tf == 0) {   // (no pad, every row shorter than a hop: nothing to store)
        if (out_len > 0) DFX_HIP(hipMemsetAsync(y, 0, (size_t)B * out_len * (pcm16 ? 2 : 4), s));
        return DFX_OK;
    }
    float lim = 0.f;
    if (atten_lim_db != 0.f) {
        lim = powf(10.f, -fabsf(atten_lim_db) / 20.f);  // enhance.py:238-239
        if (lim >= 1.f) lim = 0.99999994f;              // |dB| tiny: the reference mixes with lim == 1.0f (the noisy signal passes)
    }
    if (int rc = pass_begin(m, B * Tf)) return rc;
    DfxTurn turn(m, s, true);
    if (int rc = dfx_ws_fill(m, workspace, need, s)) return rc;   // (the row metadata of a varlen call and every chunk's layout)
    int64_t *meta = nullptr;
    bool short_out = false;
    if (lens) {
        meta = reinterpret_cast<int64_t *>(base);
        base += enh_rows_bytes(B);
        if (int rc = dfx_launch_varlen_rows(lens, B, meta, st->hop, pad ? st->N : 0, s)) return rc;
        for (int64_t b = 0; b < B; ++b) short_out |= (pad ? lens[b] : lens[b] / st->hop * st->hop) < out_len;
    }
    auto rows_of = [&](int64_t row, int64_t n) {
        EnhRows r;
        if (!lens) return r;
        r.len = meta + row, r.frames = meta + B + row;
        for (int64_t b = row; b < row + n; ++b) r.short_frames |= (lens[b] + (pad ? st->N : 0)) / st->hop < Tf;
        return r;
    };
    // (3) above: a shorter row's output is followed by zeros up to the pass's widest output, once every chunk has joined back into s
    auto tails = [&]() -> int {
        if (!short_out) return DFX_OK;
        DfxTails t;
        t.add(y, ys, out_len, 1);
        t.elem16 = pcm16;
        return dfx_launch_zero_tails(t, meta + 2 * B, B, s);
    };
    if (nc == 1) {
        if (int rc = enhance_chunk(m, st, x, B, T, pad, lim, y, base, s, &m->lanes[0], false, pcm16, xs, ys, rows_of(0, B))) return rc;
        if (int rc = tails()) return rc;
        turn.passed();
        return pass_end(m, B * Tf, s);
    }
    // ---- pipelined chunks: fork from the caller's stream, stagger the fronts, join back
    DFX_HIP(hipEventRecord(m->ev_fork, s));
    int64_t row = 0;
    for (int i = 0; i < nc; ++i) {
        const DfxLane *ln = &m->lanes[i];
        DFX_HIP(hipStreamWaitEvent(ln->main, m->ev_fork, 0));
        if (i > 0) DFX_HIP(hipStreamWaitEvent(ln->main, m->lanes[i - 1].ev[EV_FRONT], 0));
        // (16-bit samples: the float-typed pointers advance by half as many elements)
        const float *xi = pcm16 ? reinterpret_cast<const float *>(reinterpret_cast<const int16_t *>(x) + row * xs) : x + row * xs;
        float *yi = pcm16 ? reinterpret_cast<float *>(reinterpret_cast<int16_t *>(y) + row * ys) : y + row * ys;
        if (int rc = enhance_chunk(m, st, xi, sizes[i], T, pad, lim, yi, base, ln->main, ln, true, pcm16, xs, ys, rows_of(row, sizes[i])))
            return rc;
        DFX_HIP(hipEventRecord(ln->ev[EV_DONE], ln->main));
        base += (plan_enh(m, st, sizes[i], T, pad).total + 255) & ~(size_t)255;
        row += sizes[i];
    }
    for (int i = 0; i < nc; ++i) DFX_HIP(hipStreamWaitEvent(s, m->lanes[i].ev[EV_DONE], 0));
    if (int rc = tails()) return rc;
    turn.passed();
    return pass_end(m, B * Tf, s);
}
extern "C" int dfx_enhance(const dfx_model *m, const dfx_state *st, const float *x, int64_t B, int64_t T, int pad,
                           float atten_lim_db, float *y, void *workspace, int64_t workspace_bytes, void *stream) {
    return enhance_any(m, st, x, B, T, pad, atten_lim_db, y, workspace, workspace_bytes, stream, false);
}
extern "C" int dfx_enhance_pcm16(const dfx_model *m, const dfx_state *st, const int16_t *x, int64_t B, int64_t T, int pad,
                                 float atten_lim_db, int16_t *y, void *workspace, int64_t workspace_bytes, void *stream) {
    return enhance_any(m, st, reinterpret_cast<const float *>(x), B, T, pad, atten_lim_db, reinterpret_cast<float *>(y), workspace, workspace_bytes,
                       stream, true);
}

// the lengths of a dfx_enhance_varlen call, checked before anything else happens, and their maximum
static int varlen_longest(int64_t B, const int64_t *lengths, int64_t *T) {
    if (B < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance_varlen: B < 0");
    if (B > 0 && !lengths) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance_varlen: null lengths");
    *T = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (lengths[b] < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_enhance_varlen: lengths[%lld] = %lld", (long long)b, (long long)lengths[b]);
        if (lengths[b] > *T) *T = lengths[b];
    }
    return DFX_OK;
}
extern "C" int dfx_enhance_varlen_workspace_bytes(const dfx_model *m, const dfx_state *st, int64_t B, const int64_t *lengths, int pad,
                                                  int64_t *bytes) {
    int64_t T = 0;
    if (int rc = varlen_longest(B, lengths, &T)) return rc;
    if (int rc = dfx_enhance_workspace_bytes(m, st, B, T, pad, bytes)) return rc;
    *bytes += (int64_t)enh_rows_bytes(B);
    return DFX_OK;
}
extern "C" int dfx_enhance_varlen(const dfx_model *m, const dfx_state *st, const float *x, int64_t B, int64_t x_stride, const int64_t *lengths,
                                  int pad, float atten_lim_db, float *y, int64_t y_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    int64_t T = 0;
    if (int rc = varlen_longest(B, lengths, &T)) return rc;
    return enhance_any(m, st, x, B, T, pad, atten_lim_db, y, workspace, workspace_bytes, stream, false, B > 0 ? lengths : nullptr, x_stride, y_stride);
}
extern "C" int dfx_enhance_varlen_pcm16(const dfx_model *m, const dfx_state *st, const int16_t *x, int64_t B, int64_t x_stride,
                                        const int64_t *lengths, int pad, float atten_lim_db, int16_t *y, int64_t y_stride, void *workspace,
                                        int64_t workspace_bytes, void *stream) {
    int64_t T = 0;
    if (int rc = varlen_longest(B, lengths, &T)) return rc;
    return enhance_any(m, st, reinterpret_cast<const float *>(x), B, T, pad, atten_lim_db, reinterpret_cast<float *>(y), workspace, workspace_bytes,
                       stream, true, B > 0 ? lengths : nullptr, x_stride, y_stride);
}
