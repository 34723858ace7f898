// dfx: the frame-by-frame runtime (dfx_stream_*: DfTract::process for many lockstep streams).
// A part of dfx_model.hip (one translation unit: included from there, in this order — launch helpers, forward pass, streaming, enhance()).
#pragma once

// Streaming history ring of one per-frame quantity (row floats per frame): work[b] = [hist_in[b] (h frames) ; new[b] (n frames, the
// first `skip` of them replaced by zeros)], and hist_out[b] = the last h frames of that window (hist_in != hist_out).
__global__ void dfx_k_ring_step(const float *hist_in, const float *nw, float *work, float *hist_out, int64_t B, int64_t h, int64_t n,
                                int64_t row, int64_t skip) {
    const int64_t wl = (h + n) * row, total = B * wl;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / wl, j = i - b * wl, fr = j / row;
        float v;
        if (fr < h) v = hist_in[b * h * row + j];
        else v = (fr - h < skip) ? 0.f : nw[b * n * row + (j - h * row)];
        work[i] = v;
        if (fr >= n) hist_out[b * h * row + (j - n * row)] = v;
    }
}

// copy rows with zero padding / offset: dst[b, i] = (i + src_off < src_len) ? src[b, i + src_off] : 0
__global__ void dfx_k_copy_rows(const float *src, int64_t src_stride, int64_t src_len, int64_t src_off, float *dst,
                                int64_t dst_stride, int64_t dst_len, int64_t B) {
    const int64_t n = B * dst_len;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / dst_len, j = i - b * dst_len;
        const int64_t sj = j + src_off;
        dst[b * dst_stride + j] = sj < src_len ? src[b * src_stride + sj] : 0.f;
    }
}

__global__ void dfx_k_fill_rows(float *dst, int64_t dst_stride, int64_t len, int64_t B, float v) {
    const int64_t n = B * len;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / len;
        dst[b * dst_stride + (i - b * len)] = v;
    }
}

// ---- streams of one handle that start over on their own (dfx_stream_reset_streams) -----------------------------------------------------
// DfxRowClear lists, per state array of the handle, the part of a row that a stream's start zeroes: entry e covers bytes[e] bytes at
// p[e] + rep * rep_stride[e] + row * stride[e], rep < reps[e] (the GRU layers).  The same table form serves the reset itself (rows = the
// caller's ids) and the warm-up of a reset stream (rows = the streams that are younger than the lookahead: dfx_k_stream_warm).
#define DFX_ROWS_MAX_ENTRIES 32
#define DFX_RESET_IDS 512   /* stream indices per launch of the reset kernel (they travel as kernel arguments: no upload, no wait) */
struct DfxRowClear {
    unsigned char *p[DFX_ROWS_MAX_ENTRIES];
    int64_t stride[DFX_ROWS_MAX_ENTRIES], bytes[DFX_ROWS_MAX_ENTRIES], rep_stride[DFX_ROWS_MAX_ENTRIES];
    int reps[DFX_ROWS_MAX_ENTRIES];
    int n;
    // host: appends an entry; false when the table is full (the callers report that: the table travels by value as a kernel argument)
    bool add(void *ptr, int64_t stride_, int64_t bytes_, int reps_ = 1, int64_t rep_stride_ = 0) {
        if (bytes_ <= 0) return true;
        if (n >= DFX_ROWS_MAX_ENTRIES) return false;
        p[n] = static_cast<unsigned char *>(ptr), stride[n] = stride_, bytes[n] = bytes_, reps[n] = reps_, rep_stride[n] = rep_stride_;
        ++n;
        return true;
    }
};
struct DfxRowIds {
    int n;
    int id[DFX_RESET_IDS];
};
// part / parts: the workgroups that share one row
static __device__ __forceinline__ void dfx_clear_row(const DfxRowClear &R, int64_t row, int part, int parts) {
    const int64_t i0 = (int64_t)part * blockDim.x + threadIdx.x, step = (int64_t)parts * blockDim.x;
    for (int e = 0; e < R.n; ++e)
        for (int r = 0; r < R.reps[e]; ++r) {
            unsigned char *p = R.p[e] + r * R.rep_stride[e] + row * R.stride[e];
            const int64_t nb = R.bytes[e];
            if ((((uintptr_t)p | (uintptr_t)nb) & 15) == 0) {
                float4 *q = reinterpret_cast<float4 *>(p);
                for (int64_t i = i0; i < (nb >> 4); i += step) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else if ((((uintptr_t)p | (uintptr_t)nb) & 3) == 0) {
                float *q = reinterpret_cast<float *>(p);
                for (int64_t i = i0; i < (nb >> 2); i += step) q[i] = 0.f;
            } else {
                for (int64_t i = i0; i < nb; i += step) p[i] = 0;
            }
        }
}

// Workgroups (k * ch + c, part): channel c of stream I.id[k] starts over — its rows of every state array are zeroed, its running means take
// the initial values of a fresh erb_norm / unit_norm (the expressions of dfx_stream_reset, evaluated with the same roundings) and
// birth[row] = the handle's hop count.  Duplicate ids write the same values twice.
__global__ void __launch_bounds__(256) dfx_k_stream_reset_rows(DfxRowClear R, DfxRowIds I, int ch, float *erb_state, int E, float erb_step,
                                                               float *unit_state, int Fd, float unit_step, int64_t *birth, int64_t now) {
    const int k = (int)blockIdx.x / ch;
    if (k >= I.n) return;
    const int64_t row = (int64_t)I.id[k] * ch + (int)blockIdx.x % ch;
    dfx_clear_row(R, row, (int)blockIdx.y, (int)gridDim.y);
    if (blockIdx.y != 0) return;
    for (int i = threadIdx.x; i < E; i += blockDim.x) erb_state[row * E + i] = __fadd_rn(-60.f, __fmul_rn(erb_step, (float)i));
    for (int i = threadIdx.x; i < Fd; i += blockDim.x) unit_state[row * Fd + i] = __fadd_rn(0.001f, __fmul_rn(unit_step, (float)i));
    if (threadIdx.x == 0) birth[row] = now;
}

// Per-stream start of the network time inside this pass's window: tz[b] = local index of stream b's net position 0 (DfxStreamCtx::t_zero
// with the stream's own age now - birth[b] in place of the handle's hop count), 0 once the stream is older than the window.
__global__ void dfx_k_stream_tzero(const int64_t *birth, int64_t now, int64_t Hs, int *tz, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    // (a stream that sits this pass out — dfx_k_stream_pause has moved its birth already — may read one hop younger than 0: its pass is discarded)
    const int64_t age = now > birth[b] ? now - birth[b] : 0;
    tz[b] = age < Hs ? (int)(Hs - age) : 0;
}

// Warm-up of a stream that started over while the others run on (one new hop per pass): the hop has no net position yet (tz[b] > H: the new
// frame, local index H, lies before the stream's position 0), so — like the first `lookahead` hops of a fresh handle — its features enter
// the windows as zeros, its network state (GRU rows, df_convp's sums / delay line) and its enhanced spectrum are zero again after the
// pass; STFT memory, running means and rolling spectra have advanced.  Gated handles: no stage decision was taken for the stream — its
// flags are cleared and its silent-input counter is lowered by the one dfx_k_gate_finish then adds for "gains absent".
__global__ void __launch_bounds__(256) dfx_k_stream_warm(DfxRowClear R, const int *tz, int H, int *gate_counter, int64_t B) {
    const int64_t b = blockIdx.x;
    if (b >= B || tz[b] <= H) return;
    dfx_clear_row(R, b, (int)blockIdx.y, (int)gridDim.y);
    if (gate_counter && blockIdx.y == 0 && threadIdx.x == 0) gate_counter[b] -= 1;
}

// The same on a pausable handle: a stream that sits the pass out (DFX_GATE_PAUSED) did not consume the hop — nothing of it is cleared and its
// silent-input counter stays.
__global__ void __launch_bounds__(256) dfx_k_stream_warm_active(DfxRowClear R, const int *tz, int H, int *gate_counter, const unsigned char *flags, int64_t B) {
    const int64_t b = blockIdx.x;
    if (b >= B || tz[b] <= H || (flags[b] & DFX_GATE_PAUSED)) return;
    dfx_clear_row(R, b, (int)blockIdx.y, (int)gridDim.y);
    if (gate_counter && blockIdx.y == 0 && threadIdx.x == 0) gate_counter[b] -= 1;
}

// ---- streams that sit a call out (dfx_stream_process_active) ------------------------------------------------------------------------------
// The call's mask travels as a bit field in the kernel arguments (no upload, no wait): bit k of DfxPauseMask = stream first + k is paused.
// One thread per row of the streams [first, first + n): a paused row is flagged DFX_GATE_FROZEN | DFX_GATE_PAUSED for this pass — the hold /
// commit kernels of the gated runtime then hand it every state array back — its silent-input counter takes the value it had before
// dfx_k_gate_pre looked at the hop (counter_before; null: no silent-input test ran), and birth[row] moves forward by `bump` hops, so that
// the stream's age (handle hop count - birth) stands still.  set_all: the rows that take part get flags 0 (a handle without the silent-input
// test, where no other kernel initialises the flags of the pass).
#define DFX_PAUSE_STREAMS 4096   /* streams per launch: 512 bytes of kernel arguments */
struct DfxPauseMask {
    int first, n;
    unsigned bits[DFX_PAUSE_STREAMS / 32];
};
__global__ void __launch_bounds__(256) dfx_k_stream_pause(DfxPauseMask P, int ch, unsigned char *flags, int set_all, int *counter, const int *counter_before,
                                                          int64_t *birth, int bump) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (int64_t)P.n * ch) return;
    const int st = (int)(k / ch);
    const int64_t row = (int64_t)P.first * ch + k;
    if ((P.bits[st >> 5] >> (st & 31)) & 1u) {
        flags[row] = DFX_GATE_FROZEN | DFX_GATE_PAUSED;
        if (counter_before) counter[row] = counter_before[row];
        birth[row] += bump;
    } else if (set_all) {
        flags[row] = 0;
    }
}

// ---- settings that belong to one stream of a handle (dfx_stream_set_*_streams) ------------------------------------------------------------
// The ids and their values travel as kernel arguments, like DfxRowIds (no upload, no wait).  DFX_SET_IDS ids per launch: with three values
// per id (the thresholds) the argument block is 4 + 192 * 4 + 192 * 12 = 3076 bytes, inside the 4 KB a launch can carry.
// One thread per row of the named streams: dst[row][0..W) = the stream's W values (row = id * ch + channel).  The host has resolved
// duplicate ids (one entry per stream, the last occurrence's values), so no two threads write one row.
#define DFX_SET_IDS 192
template <int W>
struct DfxRowVals {
    int n;
    int id[DFX_SET_IDS];
    float v[DFX_SET_IDS * W];
};
template <int W>
__global__ void __launch_bounds__(256) dfx_k_stream_set_rows(DfxRowVals<W> V, int ch, float *dst, int64_t B) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= V.n * ch) return;
    const int k = i / ch;
    const int64_t row = (int64_t)V.id[k] * ch + i % ch;
    if (row >= B) return;
#pragma unroll
    for (int j = 0; j < W; ++j) dst[row * W + j] = V.v[k * W + j];
}

// ---- clips that end inside a call (dfx_stream_process_ends) ---------------------------------------------------------------------------------
// keep[row] = the hops of this pass that still belong to the row's clip.  The counts travel as kernel arguments, like the pause mask and the
// varlen path's row metadata (dfx_k_varlen_rows): no upload, no wait, and the caller's array is free when the call returns.
#define DFX_END_ROWS 512   /* rows per launch: 2 KB of kernel arguments */
struct DfxEndRows {
    int64_t *keep;
    int64_t row0;
    int n;
    int cnt[DFX_END_ROWS];
};
__global__ void __launch_bounds__(256) dfx_k_stream_end_rows(DfxEndRows A) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < A.n) A.keep[A.row0 + i] = A.cnt[i];
}

// ------------------------------------------------------------------------------------------------ streaming (dfx_stream_*)
// Frame loop of DfTract::process (tract.rs:509-642) for many lockstep streams: every call runs the batch kernels on a window of
// H history + n new frames per stream (DfxStreamCtx), with all recurrent state carried in the handle.
struct dfx_stream_state {
    const dfx_model *m = nullptr;
    const dfx_state *st = nullptr;
    int64_t B = 0;
    int nmax = 0, H = 0, L = 0, layers = 0;
    int64_t frames = 0;       // hops consumed since the last reset of the whole handle: the lockstep network time of all streams
    // The start-of-stream position is per stream: birth[row] = `frames` when the row last started over (dfx_stream_reset_streams; 0 after
    // a reset of the whole handle), on the host and — for the kernels — on the device.  While frames < mixed_until some stream is younger
    // than the window (H + L hops) and younger than the handle: passes then compute the per-row t_zero (dfx_k_stream_tzero); while
    // frames < warm_until some such stream is younger than the lookahead: passes carry one hop and end with dfx_k_stream_warm.  Past both, a
    // pass enqueues exactly what a handle without individual resets enqueues.
    std::vector<int64_t> birth;
    int64_t mixed_until = 0, warm_until = 0;
    size_t birth_dev = 0, tz_rows = 0;   // byte offsets into buf: int64 [B], int [B]
    float lim = 0.f;          // linear attenuation limit: 0 = off, 1 = bypass (tract.rs:387-398)
    float pf_beta = -1.f;     // < 0: the model's setting
    unsigned char *buf = nullptr;
    size_t bytes = 0;
    // byte offsets into buf
    size_t ana_mem[2], syn_mem[2], erb_state, unit_state, hist_fe[2], hist_fs[2], hist_spec[2], new_spec, new_fe, new_fs, work_fe, work_fs,
        work_spec, out_spec, h_state, h_state2, lsnr, model_ws;
    int hflip = 0;            // which of h_state / h_state2 holds the GRU states (the one-step kernel writes the other one: dfx_k_gru_step_h3)
    size_t c0ring = 0;        // pending sums of df_convp's next kt - 1 outputs (dfx_k_df_convp_step); c0ring_bytes == 0: not available
    size_t c0ring_bytes = 0;
    bool c0ring_ok = true;    // the sums are current (all zeros after a reset; stale after a pass that did not go through the step kernel)
    int64_t model_ws_bytes = 0;
    int flip = 0;             // which of the double-buffered STFT memories is current
    // The rolling spectra of an ungated handle live in a LINEAR buffer [B, lin_cap, F] through which the window [lin_pos, lin_pos + Hs + n)
    // slides: a call appends its n new frames and the deep filter reads the window in place (clip stride lin_cap frames); only when the
    // window reaches the end are its last Hs frames moved back to the front (once per lin_cap - Hs - n hops).  The ring form below
    // (hist_spec -> work_spec, dfx_k_ring_step) rewrites the whole window on every call — at 4096 streams 95 us of a 720 us hop — and stays
    // for gated handles (a frozen stream's spectra must not move) and graph replay (fixed addresses).  lin_owns: which form holds the state.
    int64_t Fp = 0;           // bins per spectrum row of the handle's buffers: F rounded up to a multiple of 8 (64-byte rows: the row-streaming deep filter takes them)
    size_t spec_lin = 0;
    int64_t lin_cap = 0, lin_pos = 0;
    bool lin_owns = false;
    // the encoder's feature windows in the same form (stream_body): [B, feat_cap, E] and [B, feat_cap, Fd, 2] at the same lin_pos
    size_t fe_lin = 0, fs_lin = 0;
    int64_t feat_cap = 0;
    bool feat_owns = false;
    // per-stream stage gating (dfx_stream_set_gating; DfTract::process, tract.rs:509-616,658-672): off by default
    bool gated = false;
    int channels = 1, reduce_mask = 2;    // multi-channel streams: ch consecutive rows per stream; ReduceMask::MEAN is the reference default
    float thr[3] = {-10.f, 30.f, 20.f};   // RuntimeParams::default_with_ch (tract.rs:177-189)
    unsigned char *gate_buf = nullptr;    // own allocation, made when gating is first switched on
    size_t g_flags = 0, g_counter = 0, g_sh_erb = 0, g_sh_unit = 0, g_sh_h = 0, g_c0_win = 0, g_mask = 0, g_coefs = 0, gate_bytes = 0;
    size_t g_pend2 = 0, g_par = 0, g_cnt = 0;   // pending-sum form of the gated df_convp (g_pend2_ok; then g_c0_win is not allocated)
    bool g_pend2_ok = false;
    size_t g_sh_counter = 0;  // the silent-input counters as they were before dfx_k_gate_pre (a paused stream gets its own back)
    // Pausable handles (dfx_stream_set_pausable): a call may carry a mask of the streams that take part (dfx_stream_process_active).  Such a
    // handle keeps its state in the per-stream forms of the gated runtime from its first hop (one hop per pass; without gating every stage
    // is forced on and the silent-input test is off), and a paused stream is one more kind of frozen row (DFX_GATE_PAUSED).  The handle's hop
    // count still advances with every pass; a paused stream's birth moves with it — here and, by dfx_k_stream_pause, on the device — so its
    // age stands still.  Which passes take the per-row t_zero / the warm-up is decided per pass from the ages of the streams that take part.
    bool pausable = false;
    bool fresh = true;        // no hop consumed since create / dfx_stream_reset
    std::vector<unsigned char> paused;   // [B / channels], this call: 1 = sits out
    bool any_paused = false;
    // Settings per stream (dfx_stream_set_*_streams): in the reference the attenuation limit, the post-filter beta and the thresholds belong to
    // one DfTract, i.e. to one caller (capi.rs:136-156, tract.rs:160-170).  The host keeps every row's values (what dfx_stream_get_settings
    // reports; the handle-wide setters write all rows); the device arrays — own allocation, made by the first per-stream setter — are read by
    // the finishing kernel (lim, beta) and dfx_k_gate_post (thr) only while the handle is per-row in that setting (*_rows).  A handle-wide
    // setter makes the handle uniform in its setting again: passes then take the scalars above, as on a handle that never was per-row, and
    // the device array of that setting is stale until the next per-stream setter refills it.
    std::vector<float> row_lim_db, row_beta, row_thr;   // [B] |dB| (100 = off), [B] beta (resolved: the model's where none was set), [B][3]
    bool lim_rows = false, beta_rows = false, thr_rows = false;
    unsigned char *set_buf = nullptr;   // float lim [B] (linear), beta [B], thr [B][3]
    size_t sb_lim = 0, sb_beta = 0, sb_thr = 0;
    // Streaming at the caller's rate (dfx_stream_set_sample_rate): an up-sampler sr -> model rate in front of the pass and a down-sampler
    // behind it, both over all rows and in step form (dfx_stream_resampler_*: csrc/dfx_io_stream.h), around model-rate staging rows
    // [B, nmax * hop].  sr == 0: no rate set — a call takes today's path (the staging rows then serve dfx_stream_process_pcm16 / _g711 alone).
    int sr = 0;
    int64_t hop_native = 0;
    int rs_width = 0, rs_method = 0;     // the converters' parameters as they were given (a snapshot's layout fingerprint covers them)
    double rs_rolloff = 0., rs_beta = 0.;
    dfx_resampler *rs_up = nullptr, *rs_dn = nullptr;
    dfx_stream_resampler *up = nullptr, *dn = nullptr;
    float *stage_in = nullptr, *stage_out = nullptr;   // [B, nmax * hop] each
    void *thru_tmp = nullptr;                          // [B, nmax * hop_native] floats: where the down-sampler writes during the pass-through
    std::vector<unsigned char> row_active;             // [B], this call: the resamplers' mask (a paused stream's rows: 0)
    // Clips that end inside a call (dfx_stream_process_ends): ended[row] — host — marks a row whose clip has ended and that was not reset since;
    // call_valid — the running call's valid_hops (null: no row ends in it), from which stream_process_impl derives every pass's counts
    // pass_keep [B] and whether a row of the pass is short of the pass's hops (pass_ends: then features() zeroes the frames behind the ends).
    // (a row that has ended stays behind its end in every later call, whichever entry point makes it, until it is reset)
    std::vector<unsigned char> ended;
    int64_t n_ended = 0;
    const int64_t *call_valid = nullptr;
    std::vector<int> pass_keep;
    bool pass_ends = false;
    size_t keep_dev = 0;      // byte offset into buf: int64 [B]
    // (Replaying a steady-state call from a hipGraph was built in round 1 and removed in round 4: on ROCm 7.2 the replay of the hop's kernel nodes
    // took 2.0-2.2 ms per call where plain launches take 0.4.)
};

static int stream_copy_rows(const float *src, int64_t src_stride, int64_t src_len, int64_t src_off, float *dst, int64_t dst_stride,
                            int64_t dst_len, int64_t B, hipStream_t s) {
    if (B <= 0 || dst_len <= 0) return DFX_OK;
    DfxKScope ks(DFX_K_COPY_ROWS, s);
    dfx_launch(dfx_k_copy_rows, dim3((unsigned)nn_grid(dfx_ceil_div(B * dst_len, 256), 16)), dim3(256), 0, s, src, src_stride, src_len,
               src_off, dst, dst_stride, dst_len, B);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}

// Bytes per stream of df_convp's pending sums (dfx_k_df_convp_step): [kt-1][nfb][64 lanes] x 16 bytes.  A gated handle keeps them twice
// per stream (DfxGate::pend2: the half that is current and the one being built).
static inline size_t stream_c0ring_row_bytes(const dfx_model_cfg &c) {
    return (size_t)(c.df_pathway_kernel_size_t - 1) * ((c.nb_df + 15) / 16) * 64 * 16;
}
static inline size_t stream_pend2_row_bytes(const dfx_model_cfg &c) { return 2 * stream_c0ring_row_bytes(c); }

// what a model and a DF state must be for a handle (dfx_stream_create, dfx_stream_memory_bytes)
static int stream_create_check(const dfx_model *m, const dfx_state *st, int64_t streams, int max_frames, const char *who) {
    if (!m || !st || streams <= 0 || max_frames <= 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: bad arguments", who);
    const dfx_model_cfg &c = m->cfg;
    if (st->N != c.fft_size || st->hop != c.hop_size || st->nb != c.nb_erb)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: the DF state does not match the model (fft/hop/nb_erb)", who);
    if (c.conv_lookahead != c.df_lookahead)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: conv_lookahead != df_lookahead is not supported by the streaming path", who);
    // (either arithmetic, DF stage on or off: an exact handle keeps its feature windows in ring form and a gated one its c0 window — the forms of
    // every model without fp16-split fragments — and its GRU layers step on dfx_k_gru_step_x32 / dfx_k_gru_rec_x32)
    if (!m->can.fuse_c0)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: streaming needs the fused DF encoder (df_pathway_kernel_size_t <= 5, df_order <= 8)", who);
    if (!m->can.fuse_enc)   // (what DfxPass::plan() would refuse on the first hop)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: streaming needs the fused ERB encoder head (nb_erb even and <= 62, a frame's rows within the LDS)", who);
    return DFX_OK;
}

// The layout of a handle's device buffer for s->m, s->st, s->B rows and s->nmax hops per call: every byte offset, the window geometry and
// s->bytes.  No device access: dfx_stream_create allocates what this plans, dfx_stream_memory_bytes reports it.
static void stream_layout(dfx_stream_state *s) {
    const dfx_model *m = s->m;
    const dfx_state *st = s->st;
    const dfx_model_cfg &c = m->cfg;
    const int64_t streams = s->B;
    const int max_frames = s->nmax;
    s->L = c.df_lookahead;
    // history in front of the new frames: 2 frames for the 3-tap input convolutions + kt-1 frames of (recomputed) c0 for df_convp
    const int hist_conv = 2 + (c.df_pathway_kernel_size_t - 1), hist_df = c.df_order - 1 - c.df_lookahead;
    s->H = hist_conv > hist_df ? hist_conv : hist_df;
    s->layers = (int)(m->enc_gru.size() + m->dec_gru.size() + m->df_gru.size());
    const int64_t B = streams, n = max_frames, H = s->H, Hs = s->H + s->L, F = (st->N / 2 + 1 + 7) & ~(int64_t)7 /* padded rows */, E = c.nb_erb, Fd = c.nb_df,
                  ML = st->N - st->hop;
    s->Fp = F;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    for (int i = 0; i < 2; ++i) s->ana_mem[i] = take((size_t)B * ML * 4), s->syn_mem[i] = take((size_t)B * ML * 4);
    s->erb_state = take((size_t)B * E * 4);
    s->unit_state = take((size_t)B * Fd * 4);
    for (int i = 0; i < 2; ++i) {
        s->hist_fe[i] = take((size_t)B * H * E * 4);
        s->hist_fs[i] = take((size_t)B * H * Fd * 8);
        s->hist_spec[i] = take((size_t)B * Hs * F * 8);
    }
    s->new_spec = take((size_t)B * n * F * 8);
    s->new_fe = take((size_t)B * n * E * 4);
    s->new_fs = take((size_t)B * n * Fd * 8);
    s->work_fe = take((size_t)B * (H + n) * E * 4);
    s->work_fs = take((size_t)B * (H + n) * Fd * 8);
    s->work_spec = take((size_t)B * (Hs + n) * F * 8);
    s->out_spec = take((size_t)B * n * F * 8);
    {   // linear rolling-spectra buffer: slack of at least one window (so that the move back to the front never overlaps), at most ~1 GB
        const char *lin_e = getenv("DFX_STREAM_LINEAR");   // test hook, read at every create: 0 = ring form, n > 1 = slack of n frames (the wrap of the linear buffers every few hops)
        const int lin_env = lin_e ? atoi(lin_e) : 1;
        int64_t slack = lin_env > 1 ? lin_env : 32;   // (DFX_STREAM_LINEAR=0: ring form only; = n > 1: slack of n frames, tests)
        while (slack > Hs + n && (size_t)B * (Hs + n + slack) * F * 8 > ((size_t)1 << 30)) slack /= 2;
        if (slack < Hs + n) slack = Hs + n;
        if (lin_env && (size_t)B * (Hs + n + slack) * F * 8 <= ((size_t)3 << 29)) {
            s->lin_cap = Hs + n + slack;
            s->spec_lin = take((size_t)B * s->lin_cap * F * 8);
            s->feat_cap = H + n + slack;   // the same slack: the three windows reach the end in the same call
            s->fe_lin = take((size_t)B * s->feat_cap * E * 4);
            s->fs_lin = take((size_t)B * s->feat_cap * Fd * 8);
        }
    }
    s->h_state = take((size_t)s->layers * B * 256 * 4);
    s->h_state2 = take((size_t)s->layers * B * 256 * 4);
    {   // pending sums of dfx_k_df_convp_step (4096 streams of the released model: 101 MB)
        const size_t rb = c.df_pathway_kernel_size_t >= 2 && c.conv_ch % 32 == 0 ? (size_t)B * stream_c0ring_row_bytes(c) : 0;
        if (rb > 0 && rb <= ((size_t)1 << 30) && !m->exact_fp32) {   // (only the fp16-split step kernel keeps pending sums)
            s->c0ring_bytes = rb;
            s->c0ring = take(rb);
        }
    }
    s->lsnr = take((size_t)B * (H + n) * 4);
    s->birth_dev = take((size_t)B * 8);
    s->tz_rows = take((size_t)B * 4);
    s->keep_dev = take((size_t)B * 8);
    dfx_model_workspace_bytes(m, B, H + n, &s->model_ws_bytes);
    s->model_ws = take((size_t)s->model_ws_bytes);
    s->bytes = off;
}

extern "C" int dfx_stream_create(const dfx_model *m, const dfx_state *st, int64_t streams, int max_frames, dfx_stream_state **out) {
    if (!out) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_create: bad arguments");
    if (int rc = stream_create_check(m, st, streams, max_frames, "dfx_stream_create")) return rc;
    const dfx_model_cfg &c = m->cfg;
    if (int rc = dfx_require_device()) return rc;
    dfx_stream_state *s = new dfx_stream_state();
    s->m = m;
    s->st = st;
    s->B = streams;
    s->nmax = max_frames;
    stream_layout(s);
    const int64_t B = streams;
    s->birth.assign((size_t)B, 0);
    s->ended.assign((size_t)B, 0);
    s->row_lim_db.assign((size_t)B, 100.f);
    s->row_beta.assign((size_t)B, c.mask_pf ? c.pf_beta : 0.f);
    s->row_thr.resize((size_t)B * 3);
    for (int64_t b = 0; b < B; ++b)
        for (int j = 0; j < 3; ++j) s->row_thr[(size_t)b * 3 + j] = s->thr[j];
    if (hipMalloc(reinterpret_cast<void **>(&s->buf), s->bytes) != hipSuccess) {
        const size_t bytes = s->bytes;
        delete s;
        DFX_FAIL(DFX_ERR_ALLOC, "dfx_stream_create: device allocation of %zu bytes failed", bytes);
    }
    if (int rc = dfx_stream_reset(s, nullptr)) {
        dfx_stream_free(s);
        return rc;
    }
    *out = s;
    return DFX_OK;
}

// the handle's sample-rate converters (dfx_stream_set_sample_rate) go; the staging rows stay
static void stream_rate_clear(dfx_stream_state *s) {
    dfx_stream_resampler_free(s->up), dfx_stream_resampler_free(s->dn);
    dfx_resampler_free(s->rs_up), dfx_resampler_free(s->rs_dn);
    if (s->thru_tmp) (void)hipFree(s->thru_tmp);
    s->up = s->dn = nullptr, s->rs_up = s->rs_dn = nullptr, s->thru_tmp = nullptr;
    s->sr = 0, s->hop_native = 0;
}

extern "C" void dfx_stream_free(dfx_stream_state *s) {
    if (!s) return;
    if (s->buf) (void)hipFree(s->buf);
    if (s->gate_buf) (void)hipFree(s->gate_buf);
    if (s->set_buf) (void)hipFree(s->set_buf);
    stream_rate_clear(s);
    if (s->stage_in) (void)hipFree(s->stage_in);
    if (s->stage_out) (void)hipFree(s->stage_out);
    delete s;
}

extern "C" int dfx_stream_reset(dfx_stream_state *s, void *stream) {
    if (!s) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_reset: null handle");
    hipStream_t hs = dfx_stream(stream);
    DFX_HIP(hipMemsetAsync(s->buf, 0, s->model_ws, hs));  // every state and history buffer (all of buf but the model workspace)
    // running means start like a fresh erb_norm / unit_norm (lib.rs:12-13, transforms.rs:308-318,339-349): the same expressions as
    // dfx_k_norm_scan evaluates when it is given no state
    const dfx_model_cfg &c = s->m->cfg;
    const int E = c.nb_erb, Fd = c.nb_df;
    std::vector<float> es((size_t)s->B * E), us((size_t)s->B * Fd);
    for (int ch = 0; ch < E; ++ch) {
        volatile float step = E > 1 ? (-90.f - -60.f) / (float)(E - 1) : 0.f;
        volatile float prod = step * (float)ch;
        const float v = -60.f + prod;
        for (int64_t b = 0; b < s->B; ++b) es[(size_t)b * E + ch] = v;
    }
    for (int ch = 0; ch < Fd; ++ch) {
        volatile float step = Fd > 1 ? (0.0001f - 0.001f) / (float)(Fd - 1) : 0.f;
        volatile float prod = step * (float)ch;
        const float v = 0.001f + prod;
        for (int64_t b = 0; b < s->B; ++b) us[(size_t)b * Fd + ch] = v;
    }
    DFX_HIP(hipStreamSynchronize(hs));
    DFX_HIP(hipMemcpy(s->buf + s->erb_state, es.data(), es.size() * 4, hipMemcpyHostToDevice));
    DFX_HIP(hipMemcpy(s->buf + s->unit_state, us.data(), us.size() * 4, hipMemcpyHostToDevice));
    if (s->gate_buf) DFX_HIP(hipMemset(s->gate_buf, 0, s->gate_bytes));  // skip counters, c0 windows (zero = the causal padding)
    s->frames = 0;
    s->birth.assign((size_t)s->B, 0);   // (the device copy is part of buf: zeros)
    s->ended.assign((size_t)s->B, 0);
    s->n_ended = 0;
    s->mixed_until = s->warm_until = 0;
    s->flip = 0;
    s->lin_pos = 0;
    s->lin_owns = false;   // (both forms are all zeros now)
    s->feat_owns = false;
    s->hflip = 0;
    s->c0ring_ok = true;   // (zeros = the causal padding in front of the stream)
    s->fresh = true;
    if (s->sr) {
        if (int rc = dfx_stream_resampler_reset(s->up, nullptr, 0, stream)) return rc;
        if (int rc = dfx_stream_resampler_reset(s->dn, nullptr, 0, stream)) return rc;
    }
    return DFX_OK;
}

// df_convp's state of one stream, as both a stream's start (stream_state_rows) and the warm-up of a started stream (DfxStreamPass::warm_rows)
// zero it: the pending sums of an ungated pass, and — per_stream: the handle's passes keep the gated runtime's forms — the per-stream
// delay line in whichever form the handle has (pending sums twice with parity and count, or the window of c0 frames).
static bool stream_convp_rows(const dfx_stream_state *S, bool per_stream, DfxRowClear &R) {
    const dfx_model_cfg &c = S->m->cfg;
    bool ok = true;
    if (S->c0ring_bytes) ok = R.add(S->buf + S->c0ring, (int64_t)stream_c0ring_row_bytes(c), (int64_t)stream_c0ring_row_bytes(c)) && ok;
    if (!per_stream) return ok;
    unsigned char *g = S->gate_buf;
    if (S->g_pend2_ok) {
        ok = R.add(g + S->g_pend2, (int64_t)stream_pend2_row_bytes(c), (int64_t)stream_pend2_row_bytes(c)) && ok;
        ok = R.add(g + S->g_par, 1, 1) && ok;
        ok = R.add(g + S->g_cnt, 4, 4) && ok;
    } else if (c.df_pathway_kernel_size_t > 1) {
        const int64_t wb = (int64_t)(S->H + 1) * c.nb_df * c.conv_ch * 4;
        ok = R.add(g + S->g_c0_win, wb, wb) && ok;
    }
    return ok;
}

// The rows of every state array that a stream's start zeroes, in whichever form currently holds the state (both ring parities, the
// linear windows' history at lin_pos, both GRU buffers, the pending sums, the gate arrays and shadow copies).
static int stream_state_rows(const dfx_stream_state *S, DfxRowClear &R) {
    const dfx_model_cfg &c = S->m->cfg;
    const int64_t B = S->B, H = S->H, Hs = S->H + S->L, E = c.nb_erb, Fd = c.nb_df, ML = S->st->N - S->st->hop, Fp = S->Fp;
    R.n = 0;
    bool ok = true;
    auto add = [&](unsigned char *p, int64_t stride, int64_t bytes, int reps = 1, int64_t rep_stride = 0) { ok = R.add(p, stride, bytes, reps, rep_stride) && ok; };
    for (int i = 0; i < 2; ++i) {
        add(S->buf + S->ana_mem[i], ML * 4, ML * 4);
        add(S->buf + S->syn_mem[i], ML * 4, ML * 4);
        add(S->buf + S->hist_fe[i], H * E * 4, H * E * 4);
        add(S->buf + S->hist_fs[i], H * Fd * 8, H * Fd * 8);
        add(S->buf + S->hist_spec[i], Hs * Fp * 8, Hs * Fp * 8);
    }
    if (S->lin_cap > 0) add(S->buf + S->spec_lin + S->lin_pos * Fp * 8, S->lin_cap * Fp * 8, Hs * Fp * 8);
    if (S->lin_cap > 0 && S->feat_cap > 0) {
        add(S->buf + S->fe_lin + S->lin_pos * E * 4, S->feat_cap * E * 4, H * E * 4);
        add(S->buf + S->fs_lin + S->lin_pos * Fd * 8, S->feat_cap * Fd * 8, H * Fd * 8);
    }
    add(S->buf + S->h_state, 1024, 1024, S->layers, B * 1024);
    add(S->buf + S->h_state2, 1024, 1024, S->layers, B * 1024);
    if (S->gate_buf) {
        unsigned char *g = S->gate_buf;
        add(g + S->g_flags, 1, 1);
        add(g + S->g_counter, 4, 4);
        add(g + S->g_sh_erb, E * 4, E * 4);
        add(g + S->g_sh_unit, Fd * 4, Fd * 4);
        add(g + S->g_sh_h, 1024, 1024, S->layers, B * 1024);
    }
    ok = stream_convp_rows(S, S->gate_buf != nullptr, R) && ok;
    if (!ok) DFX_FAIL(DFX_ERR_UNSUPPORTED, "stream reset: more state arrays than DFX_ROWS_MAX_ENTRIES");
    return DFX_OK;
}

extern "C" int dfx_stream_reset_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, void *stream) {
    if (!s || count < 0 || (count > 0 && !ids)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_reset_streams: null handle or id list");
    const int ch = s->channels;
    const int64_t ns = s->B / ch;
    for (int64_t i = 0; i < count; ++i)
        if (ids[i] < 0 || ids[i] >= ns)
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_reset_streams: stream index %lld is not in [0, %lld)", (long long)ids[i], (long long)ns);
    if (count == 0) return DFX_OK;
    if (int rc = dfx_require_device()) return rc;
    hipStream_t hs = dfx_stream(stream);
    const dfx_model_cfg &c = s->m->cfg;
    const int E = c.nb_erb, Fd = c.nb_df;
    const float erb_step = E > 1 ? (-90.f - -60.f) / (float)(E - 1) : 0.f, unit_step = Fd > 1 ? (0.0001f - 0.001f) / (float)(Fd - 1) : 0.f;
    DfxRowClear R;
    if (int rc = stream_state_rows(s, R)) return rc;
    for (int64_t i0 = 0; i0 < count; i0 += DFX_RESET_IDS) {
        DfxRowIds I;
        I.n = (int)(count - i0 < DFX_RESET_IDS ? count - i0 : DFX_RESET_IDS);
        for (int i = 0; i < I.n; ++i) I.id[i] = (int)ids[i0 + i];
        dfx_launch(dfx_k_stream_reset_rows, dim3((unsigned)(I.n * ch), 4), dim3(256), 0, hs, R, I, ch, reinterpret_cast<float *>(s->buf + s->erb_state), E,
                   erb_step, reinterpret_cast<float *>(s->buf + s->unit_state), Fd, unit_step, reinterpret_cast<int64_t *>(s->buf + s->birth_dev), s->frames);
        DFX_LAUNCH_CHECK();
    }
    for (int64_t i = 0; i < count; ++i)
        for (int k = 0; k < ch; ++k) {
            const size_t r = (size_t)(ids[i] * ch + k);
            s->birth[r] = s->frames;
            s->n_ended -= s->ended[r], s->ended[r] = 0;
        }
    if (s->sr) {   // the streams' rows of both converters start over too
        std::vector<int64_t> rows((size_t)count * ch);
        for (int64_t i = 0; i < count; ++i)
            for (int k = 0; k < ch; ++k) rows[(size_t)(i * ch + k)] = ids[i] * ch + k;
        if (int rc = dfx_stream_resampler_reset(s->up, rows.data(), (int64_t)rows.size(), stream)) return rc;
        if (int rc = dfx_stream_resampler_reset(s->dn, rows.data(), (int64_t)rows.size(), stream)) return rc;
    }
    if (s->frames > 0) {   // (frames == 0: every stream of the handle is at its start anyway)
        s->mixed_until = s->frames + s->H + s->L;
        s->warm_until = s->frames + s->L;
    }
    return DFX_OK;
}

extern "C" int dfx_stream_frames(const dfx_stream_state *s, int64_t *frames_out) {
    if (!s || !frames_out) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_frames: null argument");
    const int64_t ns = s->B / s->channels;
    for (int64_t k = 0; k < ns; ++k) frames_out[k] = s->frames - s->birth[(size_t)(k * s->channels)];
    return DFX_OK;
}

// tract.rs:658-672 / RuntimeParams::with_thresholds (:160-170).  Gating needs the stream to be at a reset point only in the sense
// that the decoders' delay lines start empty when it is switched on.
extern "C" int dfx_stream_set_thresholds(dfx_stream_state *s, float min_db_thresh, float max_db_erb_thresh, float max_db_df_thresh) {
    if (!s) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_thresholds: null handle");
    s->thr[0] = min_db_thresh;
    s->thr[1] = max_db_erb_thresh;
    s->thr[2] = max_db_df_thresh;
    for (int64_t b = 0; b < s->B; ++b)
        for (int j = 0; j < 3; ++j) s->row_thr[(size_t)b * 3 + j] = s->thr[j];
    s->thr_rows = false;   // uniform again: passes take the scalars
    return DFX_OK;
}

// RuntimeParams::n_ch / with_mask_reduce (tract.rs:119-176): rows [k*ch, (k+1)*ch) are the channels of stream k
extern "C" int dfx_stream_set_channels(dfx_stream_state *s, int channels, int reduce_mask) {
    if (!s || channels < 1 || s->B % channels != 0 || reduce_mask < 0 || reduce_mask > 2)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_channels: channels must divide the number of rows; reduce_mask 0 none, 1 max, 2 mean");
    s->channels = channels;
    s->reduce_mask = reduce_mask;
    return DFX_OK;
}

// the per-stream state forms (flags, counters, shadow copies, df_convp's per-stream delay line) of gated and of pausable handles
static int stream_gate_alloc(dfx_stream_state *s, const char *who) {
    const dfx_model_cfg &c = s->m->cfg;
    if (c.df_lookahead > 5) DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: lookahead > 5 hops is not supported", who);
    if (c.df_pathway_kernel_size_t > 5) DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: df_pathway_kernel_size_t > 5 is not supported", who);
    if (!s->gate_buf) {
        const int64_t B = s->B, T = s->H + 1;
        size_t off = 0;
        auto take = [&](size_t bytes) {
            size_t o = off;
            off += (bytes + 255) & ~(size_t)255;
            return o;
        };
        s->g_flags = take((size_t)B);
        s->g_counter = take((size_t)B * 4);
        s->g_sh_erb = take((size_t)B * c.nb_erb * 4);
        s->g_sh_unit = take((size_t)B * c.nb_df * 4);
        s->g_sh_h = take((size_t)s->layers * B * 256 * 4);
        {   // df_convp's state of a gated handle: pending sums (fp16-split models; 2 x what the ungated handle keeps) or the window of c0 frames
            const int kt = c.df_pathway_kernel_size_t;
            s->g_pend2_ok = kt >= 2 && s->m->can.c0_h3;
            if (s->g_pend2_ok) {
                s->g_pend2 = take((size_t)B * stream_pend2_row_bytes(c));
                s->g_par = take((size_t)B);
                s->g_cnt = take((size_t)B * 4);
            }
            s->g_c0_win = take(kt > 1 && !s->g_pend2_ok ? (size_t)B * T * c.nb_df * c.conv_ch * 4 : 256);
        }
        s->g_mask = take((size_t)B * T * c.nb_erb * 4);                       // dfx_stream_process_raw: the pass's mask / coefficients
        s->g_coefs = take((size_t)B * c.df_order * T * c.nb_df * 8);
        s->g_sh_counter = take((size_t)B * 4);
        s->gate_bytes = off;
        if (hipMalloc(reinterpret_cast<void **>(&s->gate_buf), off) != hipSuccess) {
            s->gate_buf = nullptr;
            DFX_FAIL(DFX_ERR_ALLOC, "%s: device allocation of %zu bytes failed", who, off);
        }
        DFX_HIP(hipMemset(s->gate_buf, 0, off));
    }
    return DFX_OK;
}

extern "C" int dfx_stream_set_gating(dfx_stream_state *s, int enable) {
    if (!s) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_gating: null handle");
    if (!enable) {
        s->gated = false;
        return DFX_OK;
    }
    if (int rc = stream_gate_alloc(s, "dfx_stream_set_gating")) return rc;
    s->gated = true;
    return DFX_OK;
}

extern "C" int dfx_stream_set_pausable(dfx_stream_state *s, int enable) {
    if (!s) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_pausable: null handle");
    if (!s->fresh) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_pausable: only at a reset point (no hop consumed since create / dfx_stream_reset)");
    if (enable)
        if (int rc = stream_gate_alloc(s, "dfx_stream_set_pausable")) return rc;
    s->pausable = enable != 0;
    return DFX_OK;
}

extern "C" int dfx_stream_frame_length(const dfx_stream_state *s) { return s ? (s->sr ? (int)s->hop_native : s->st->hop) : 0; }
extern "C" int dfx_stream_delay_frames(const dfx_stream_state *s) { return s ? s->L : 0; }

extern "C" int dfx_stream_set_atten_lim(dfx_stream_state *s, float lim_db) {
    if (!s) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_atten_lim: null handle");
    const float lim = fabsf(lim_db);  // tract.rs:387-398
    if (lim >= 100.f) s->lim = 0.f;
    else if (lim < 0.01f) s->lim = 1.f;
    else s->lim = powf(10.f, -lim / 20.f);
    s->row_lim_db.assign((size_t)s->B, lim >= 100.f ? 100.f : lim);
    s->lim_rows = false;   // uniform again: passes take the scalar (lim == 1: the undelayed pass-through, a handle-wide mode)
    return DFX_OK;
}

// The handle's limit by enhance()'s rule instead of the runtime's (enhance.py:238-240 as dfx_enhance applies it, dfx_model_enhance.h:170-174): 0 = no
// limit, every other value mixes with 10^(-|dB|/20) kept below 1 — no undelayed pass-through for tiny values, no "off" from 100 dB on.  What a
// driver needs whose streams are the clips of an enhance() call (enhance_long).
extern "C" int dfx_stream_set_atten_lim_enhance(dfx_stream_state *s, float atten_lim_db) {
    if (!s || std::isnan(atten_lim_db)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_atten_lim_enhance: null handle or NaN");
    float lim = 0.f;
    if (atten_lim_db != 0.f) {
        lim = powf(10.f, -fabsf(atten_lim_db) / 20.f);
        if (lim >= 1.f) lim = 0.99999994f;
    }
    s->lim = lim;
    // dfx_stream_get_settings reports what is in force: |dB| as given — from 100 on a real limit here, not the runtime's "off" — and 100 for "no limit"
    s->row_lim_db.assign((size_t)s->B, atten_lim_db == 0.f ? 100.f : fabsf(atten_lim_db));
    s->lim_rows = false;
    return DFX_OK;
}

extern "C" int dfx_stream_set_post_filter_beta(dfx_stream_state *s, float beta) {
    if (!s || beta < 0.f) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_post_filter_beta: bad arguments");
    s->pf_beta = beta;
    s->row_beta.assign((size_t)s->B, beta);
    s->beta_rows = false;
    return DFX_OK;
}

// ---- the same three settings for single streams (in the reference they are properties of one DfTract, i.e. of one caller) ----------------
// Linear limit of a per-stream |dB|: like dfx_stream_set_atten_lim, except that |dB| < 0.01 does not select the handle's undelayed
// pass-through (a handle-wide mode: the network would idle for everybody) but mixes with the largest float below 1, as dfx_enhance does
// (dfx_model_enhance.h:161-162): the stream's noisy signal comes back delayed like everybody's, and its state keeps advancing.
static float stream_row_lim(float lim_db_abs) {
    if (lim_db_abs >= 100.f) return 0.f;
    if (lim_db_abs < 0.01f) return 0.99999994f;
    const float lim = powf(10.f, -lim_db_abs / 20.f);
    return lim < 1.f ? lim : 0.99999994f;
}

// which: 0 attenuation limit (W = 1), 1 post-filter beta (W = 1), 2 thresholds (W = 3).  Validates everything before anything changes; then
// — all on `stream`, nothing waits for the device — the setting's device array is brought up to date if the handle was uniform in it (every
// row takes the handle's value), and the named streams' rows are written, DFX_SET_IDS streams per launch.
template <int W>
static int stream_set_rows(dfx_stream_state *s, const char *who, int which, const int64_t *ids, int64_t count, const float *vals, void *stream) {
    if (!s || count < 0 || (count > 0 && (!ids || !vals))) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: null handle or array", who);
    const int ch = s->channels;
    const int64_t ns = s->B / ch, B = s->B;
    for (int64_t i = 0; i < count; ++i) {
        if (ids[i] < 0 || ids[i] >= ns) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: stream index %lld is not in [0, %lld)", who, (long long)ids[i], (long long)ns);
        for (int j = 0; j < W; ++j)
            if (std::isnan(vals[i * W + j])) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: value %d of entry %lld is NaN", who, j, (long long)i);
        if (which == 1 && vals[i] < 0.f) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: beta of entry %lld is negative", who, (long long)i);
    }
    if (count == 0) return DFX_OK;
    if (int rc = dfx_require_device()) return rc;
    hipStream_t hs = dfx_stream(stream);
    if (!s->set_buf) {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        s->sb_lim = 0, s->sb_beta = al((size_t)B * 4), s->sb_thr = s->sb_beta + al((size_t)B * 4);
        const size_t bytes = s->sb_thr + al((size_t)B * 12);
        if (hipMalloc(reinterpret_cast<void **>(&s->set_buf), bytes) != hipSuccess) {
            s->set_buf = nullptr;
            DFX_FAIL(DFX_ERR_ALLOC, "%s: device allocation of %zu bytes failed", who, bytes);
        }
    }
    float *dst = reinterpret_cast<float *>(s->set_buf + (which == 0 ? s->sb_lim : which == 1 ? s->sb_beta : s->sb_thr));
    bool &on = which == 0 ? s->lim_rows : which == 1 ? s->beta_rows : s->thr_rows;
    if (!on) {   // uniform so far: every row of the device array takes the handle's value (W fills of stride W)
        const dfx_model_cfg &c = s->m->cfg;
        // (a handle in pass-through mode leaves it: its other streams mix like a per-stream |dB| < 0.01)
        if (which == 0 && s->lim == 1.f) s->lim = stream_row_lim(0.f);
        const float uni[3] = {which == 0 ? s->lim : which == 1 ? (s->pf_beta >= 0.f ? s->pf_beta : (c.mask_pf ? c.pf_beta : 0.f)) : s->thr[0], s->thr[1], s->thr[2]};
        for (int j = 0; j < W; ++j) {
            dfx_launch(dfx_k_fill_rows, dim3((unsigned)nn_grid(dfx_ceil_div(B, 256), 16)), dim3(256), 0, hs, dst + j, (int64_t)W, (int64_t)1, B, uni[j]);
            DFX_LAUNCH_CHECK();
        }
    }
    // the host's copy, in the caller's order (duplicate ids: the last occurrence wins) ...
    std::vector<float> &host = which == 0 ? s->row_lim_db : which == 1 ? s->row_beta : s->row_thr;
    for (int64_t i = 0; i < count; ++i)
        for (int k = 0; k < ch; ++k)
            for (int j = 0; j < W; ++j) {
                float v = vals[i * W + j];
                if (which == 0) v = fabsf(v) >= 100.f ? 100.f : fabsf(v);
                host[(size_t)(ids[i] * ch + k) * W + j] = v;
            }
    // ... and from it the device rows, every named stream once
    std::vector<unsigned char> seen((size_t)ns, 0);
    DfxRowVals<W> V;
    V.n = 0;
    auto flush = [&]() -> int {
        if (V.n == 0) return DFX_OK;
        dfx_launch(dfx_k_stream_set_rows<W>, dim3((unsigned)dfx_ceil_div((int64_t)V.n * ch, 256)), dim3(256), 0, hs, V, ch, dst, B);
        DFX_LAUNCH_CHECK();
        V.n = 0;
        return DFX_OK;
    };
    for (int64_t i = 0; i < count; ++i) {
        if (seen[(size_t)ids[i]]) continue;
        seen[(size_t)ids[i]] = 1;
        V.id[V.n] = (int)ids[i];
        for (int j = 0; j < W; ++j) {
            const float v = host[(size_t)(ids[i] * ch) * W + j];
            V.v[V.n * W + j] = which == 0 ? stream_row_lim(v) : v;
        }
        if (++V.n == DFX_SET_IDS)
            if (int rc = flush()) return rc;
    }
    if (int rc = flush()) return rc;
    on = true;
    return DFX_OK;
}

// df_set_atten_lim (capi.rs:136-144, tract.rs:387-398) of single streams
extern "C" int dfx_stream_set_atten_lim_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const float *lim_db, void *stream) {
    return stream_set_rows<1>(s, "dfx_stream_set_atten_lim_streams", 0, ids, count, lim_db, stream);
}
// df_set_post_filter_beta (capi.rs:146-156) of single streams
extern "C" int dfx_stream_set_post_filter_beta_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const float *beta, void *stream) {
    return stream_set_rows<1>(s, "dfx_stream_set_post_filter_beta_streams", 1, ids, count, beta, stream);
}
// RuntimeParams::with_thresholds (tract.rs:160-170) of single streams
extern "C" int dfx_stream_set_thresholds_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const float *thr, void *stream) {
    return stream_set_rows<3>(s, "dfx_stream_set_thresholds_streams", 2, ids, count, thr, stream);
}
// what was set, from the host's copy: [streams / channels][5] = |lim dB| (100: off), beta, min_db, max_db_erb, max_db_df
extern "C" int dfx_stream_get_settings(const dfx_stream_state *s, float *out_host) {
    if (!s || !out_host) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_get_settings: null argument");
    const int64_t ns = s->B / s->channels;
    for (int64_t k = 0; k < ns; ++k) {
        const size_t r = (size_t)(k * s->channels);
        out_host[k * 5 + 0] = s->row_lim_db[r];
        out_host[k * 5 + 1] = s->row_beta[r];
        for (int j = 0; j < 3; ++j) out_host[k * 5 + 2 + j] = s->row_thr[r * 3 + j];
    }
    return DFX_OK;
}

// ---- what a pass (DfxStreamPass) and the features-only pass (dfx_stream_process_raw) share: each launch below has this one spelling -------
static inline float *stream_fp(const dfx_stream_state *S, size_t o) { return reinterpret_cast<float *>(S->buf + o); }
static inline float *stream_gp(const dfx_stream_state *S, size_t o) { return reinterpret_cast<float *>(S->gate_buf + o); }
// the buffer that holds the GRU states (other: the one the one-step kernel writes, dfx_k_gru_step_h3)
static inline float *stream_h(const dfx_stream_state *S, bool other = false) { return stream_fp(S, (S->hflip != 0) != other ? S->h_state2 : S->h_state); }

// The row copies of one array that a pass takes; whoever holds the list decides which stream it is enqueued on.
struct DfxCopyList {
    struct Rows { const float *src; int64_t src_stride, src_len, src_off; float *dst; int64_t dst_stride, len; } c[4];
    int n = 0;
    void add(const float *src, int64_t src_stride, int64_t src_len, int64_t src_off, float *dst, int64_t dst_stride, int64_t len) {
        c[n++] = Rows{src, src_stride, src_len, src_off, dst, dst_stride, len};
    }
    int emit(int64_t B, hipStream_t on) {
        for (int i = 0; i < n; ++i)
            if (int r = stream_copy_rows(c[i].src, c[i].src_stride, c[i].src_len, c[i].src_off, c[i].dst, c[i].dst_stride, c[i].len, B, on)) return r;
        n = 0;
        return DFX_OK;
    }
};

// Hand-over from the linear windows to the ring form: the windows' last frames become the ring form's history (current parity), listed
// in the arrays' copy lists.  The feature windows alone (spec: false) when only they change form: the pass-through, whose features do not
// advance; all three for a path that keeps every window in ring form (dfx_stream_process_raw).
static void stream_to_ring(dfx_stream_state *S, bool spec, DfxCopyList &cp_spec, DfxCopyList &cp_fe, DfxCopyList &cp_fs) {
    const int64_t H = S->H, Hs = S->H + S->L, E = S->m->cfg.nb_erb, D2 = S->m->cfg.nb_df * 2, F2 = S->Fp * 2, capf = S->feat_cap;
    if (S->feat_owns) {
        cp_fe.add(stream_fp(S, S->fe_lin), capf * E, capf * E, S->lin_pos * E, stream_fp(S, S->hist_fe[S->flip]), H * E, H * E);
        cp_fs.add(stream_fp(S, S->fs_lin), capf * D2, capf * D2, S->lin_pos * D2, stream_fp(S, S->hist_fs[S->flip]), H * D2, H * D2);
        S->feat_owns = false;
    }
    if (spec && S->lin_owns) {
        cp_spec.add(stream_fp(S, S->spec_lin), S->lin_cap * F2, S->lin_cap * F2, S->lin_pos * F2, stream_fp(S, S->hist_spec[S->flip]), Hs * F2, Hs * F2);
        S->lin_owns = false;
    }
}

// One step of a history ring: window = [history ; n new frames, the first `skip` of them as zeros], the next call's history (other
// parity) = its last h frames.
static int stream_ring_step(const dfx_stream_state *S, const size_t *hist, const float *nw, float *work, int64_t h, int64_t n, int64_t row, int64_t skip,
                            hipStream_t on) {
    DfxKScope ks(DFX_K_COPY_ROWS, on);
    dfx_launch(dfx_k_ring_step, dim3((unsigned)nn_grid(dfx_ceil_div(S->B * (h + n) * row, 256), 16)), dim3(256), 0, on, (const float *)stream_fp(S, hist[S->flip]),
               nw, work, stream_fp(S, hist[S->flip ^ 1]), S->B, h, n, row, skip);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}

// The gate of a pass over the handle's per-stream forms.  silence: the handle is gated (else pausable only: every stage runs on every hop).
static void stream_fill_gate(const dfx_stream_state *S, bool silence, DfxGate &gate) {
    gate.channels = S->channels;
    gate.flags = S->gate_buf + S->g_flags;
    gate.thr[0] = S->thr[0], gate.thr[1] = S->thr[1], gate.thr[2] = S->thr[2];
    if (!silence) gate.thr[0] = -INFINITY, gate.thr[1] = gate.thr[2] = INFINITY;
    else if (S->thr_rows) gate.thr_rows = reinterpret_cast<const float *>(S->set_buf + S->sb_thr), gate.thr[0] = gate.thr[1] = gate.thr[2] = 0.f;
    gate.c0_win = stream_gp(S, S->g_c0_win);
    if (S->g_pend2_ok) gate.pend2 = S->gate_buf + S->g_pend2, gate.par = S->gate_buf + S->g_par, gate.cnt = reinterpret_cast<int *>(S->gate_buf + S->g_cnt);
}

// After a gated network pass over T frames: the DF decoder's delay line moves where that decoder ran.
static int stream_commit_delay_line(const dfx_stream_state *S, int64_t T, hipStream_t s) {
    const dfx_model_cfg &c = S->m->cfg;
    if (c.df_pathway_kernel_size_t <= 1) return DFX_OK;
    const unsigned char *gflags = S->gate_buf + S->g_flags;
    if (S->g_pend2_ok)
        dfx_launch(dfx_k_gate_pend_commit, dim3((unsigned)dfx_ceil_div(S->B, 256)), dim3(256), 0, s, gflags, S->gate_buf + S->g_par,
                   reinterpret_cast<int *>(S->gate_buf + S->g_cnt), S->B);
    else
        dfx_launch(dfx_k_gate_c0_shift, dim3((unsigned)S->B, 4), dim3(256), 0, s, gflags, stream_gp(S, S->g_c0_win), S->B, T, c.df_pathway_kernel_size_t,
                   (int64_t)c.nb_df * c.conv_ch);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}

// Shadow copies of the state a gated pass updates in place, so that the streams that turn out not to advance (frozen, or a decoder stage
// skipped) can be given their state back after the pass.  h: the GRU states too (the layers run in place).
static int stream_shadow_state(const dfx_stream_state *S, bool h, hipStream_t s) {
    const dfx_model_cfg &c = S->m->cfg;
    DFX_HIP(hipMemcpyAsync(stream_gp(S, S->g_sh_erb), stream_fp(S, S->erb_state), (size_t)S->B * c.nb_erb * 4, hipMemcpyDeviceToDevice, s));
    DFX_HIP(hipMemcpyAsync(stream_gp(S, S->g_sh_unit), stream_fp(S, S->unit_state), (size_t)S->B * c.nb_df * 4, hipMemcpyDeviceToDevice, s));
    if (h) DFX_HIP(hipMemcpyAsync(stream_gp(S, S->g_sh_h), stream_h(S), (size_t)S->layers * S->B * 256 * 4, hipMemcpyDeviceToDevice, s));
    return DFX_OK;
}

// The double-buffered arrays that a path does not touch keep their contents across the parity flip.
static int stream_carry_parity(const dfx_stream_state *S, bool ana, bool syn, bool feat, bool spec, hipStream_t s) {
    const dfx_model_cfg &c = S->m->cfg;
    const size_t B = (size_t)S->B, ML = (size_t)(S->st->N - S->st->hop);
    const int f = S->flip;
    if (ana) DFX_HIP(hipMemcpyAsync(stream_fp(S, S->ana_mem[f ^ 1]), stream_fp(S, S->ana_mem[f]), B * ML * 4, hipMemcpyDeviceToDevice, s));
    if (syn) DFX_HIP(hipMemcpyAsync(stream_fp(S, S->syn_mem[f ^ 1]), stream_fp(S, S->syn_mem[f]), B * ML * 4, hipMemcpyDeviceToDevice, s));
    if (feat) {
        DFX_HIP(hipMemcpyAsync(stream_fp(S, S->hist_fe[f ^ 1]), stream_fp(S, S->hist_fe[f]), B * S->H * c.nb_erb * 4, hipMemcpyDeviceToDevice, s));
        DFX_HIP(hipMemcpyAsync(stream_fp(S, S->hist_fs[f ^ 1]), stream_fp(S, S->hist_fs[f]), B * S->H * c.nb_df * 8, hipMemcpyDeviceToDevice, s));
    }
    if (spec) DFX_HIP(hipMemcpyAsync(stream_fp(S, S->hist_spec[f ^ 1]), stream_fp(S, S->hist_spec[f]), B * (S->H + S->L) * S->Fp * 8, hipMemcpyDeviceToDevice, s));
    return DFX_OK;
}

// One pass of n hops over a handle: one call's kernels, enqueued on s (and the model's auxiliary streams).  It does not advance the handle's
// counters (stream_process_impl).  x / y / lsnr_out rows are strided (xs, ys, ls): a call of several passes walks the caller's arrays.
// plan() decides everything and does the host bookkeeping of the three windows; the steps after it enqueue, in the order stream_body runs them.
struct DfxStreamPass {
    // ---- what stream_body was handed
    dfx_stream_state *S;
    const float *x;
    int64_t n;
    float *y, *lsnr_out;
    hipStream_t s;
    int64_t xs, ys, ls;
    bool p_mixed, p_warm;   // streams that started over on their own: one that takes part is younger than the window / than the lookahead
    const dfx_model_cfg &c;
    // ---- the plan (plan())
    const dfx_model *m;
    const dfx_state *st;
    int64_t B, H, L, Hs, E, Fd, D2, hop, ML, Fp, F2, capf, T, a0, skip, lin_pos0;
    bool silence, gated, bypass, lin, flin, mixed, warm, step_all;
    unsigned char *gflags;
    int *gcount;
    float *am_in, *am_out, *sm_in, *sm_out, *new_spec, *new_fe, *new_fs, *work_fe, *work_fs, *work_spec, *out_spec;
    const float *spec_win, *fe_win, *fs_win;   // the windows the network reads ...
    int64_t spec_win_T, feat_T;                // ... and their clip strides in frames (feat_T 0: T)
    float *norm_fe, *norm_fs;                  // where the normalised features of the new hops go
    int64_t norm_fe_cs, norm_fs_cs;
    DfxCopyList cp_spec, cp_fe, cp_fs;         // the copies of this pass, by array
    // ---- what the enqueue has done
    bool stepped = false, erb_done = false, side_done = false;

    float *fp(size_t o) const { return stream_fp(S, o); }
    float *gp(size_t o) const { return stream_gp(S, o); }

    int plan() {
        m = S->m, st = S->st;
        B = S->B, H = S->H, L = S->L, Hs = H + L, E = c.nb_erb, Fd = c.nb_df, D2 = Fd * 2, hop = st->hop, ML = st->N - hop;
        Fp = S->Fp, F2 = Fp * 2;   // the handle's spectra have rows of Fp >= F bins
        capf = S->feat_cap, T = H + n, a0 = S->frames;
        // per-stream state forms: gated handles, and pausable ones (there `silence` — the silent-input test and the stage decisions — may be off)
        silence = S->gated && S->gate_buf, gated = (S->gated || S->pausable) && S->gate_buf;
        if (gated && n != 1) DFX_FAIL(DFX_ERR_INVALID_ARG, "gated streaming passes carry one hop");
        gflags = gated ? S->gate_buf + S->g_flags : nullptr;
        gcount = gated ? reinterpret_cast<int *>(S->gate_buf + S->g_counter) : nullptr;
        bypass = S->lim == 1.f;   // the pass-through (tract.rs:540-543)
        // ---- windows: [history ; new].  Net position p uses the features of hop p + L, so the hops of this call are the positions
        // a0 - L .. a0 + n - 1 - L; positions < 0 do not exist: their features are zero for the taps of later positions (the causal
        // padding of pad_feat, deepfilternet3.py:357-361) and they are not computed.
        skip = a0 < L ? ((L - a0) < n ? (L - a0) : n) : 0;
        // one new hop, plain launches: every GRU layer is ONE launch (projection + recurrence + gates) that leaves the new states in the
        // other buffer (several new hops: the projection and the recurrence kernel of the batch path, in place)
        step_all = n - skip == 1;
        // streams that started over on their own (dfx_stream_reset_streams): mixed — one of them is still younger than the window, the pass takes
        // t_zero per stream; warm — one of them is younger than the lookahead (the caller passes one hop at a time then): dfx_k_stream_warm
        mixed = !bypass && skip < n && p_mixed, warm = mixed && p_warm;
        if (warm && n != 1) DFX_FAIL(DFX_ERR_INVALID_ARG, "warm-up hops of a reset stream are passed one at a time");
        am_in = fp(S->ana_mem[S->flip]), am_out = fp(S->ana_mem[S->flip ^ 1]);
        sm_in = fp(S->syn_mem[S->flip]), sm_out = fp(S->syn_mem[S->flip ^ 1]);
        new_spec = fp(S->new_spec), new_fe = fp(S->new_fe), new_fs = fp(S->new_fs);
        work_fe = fp(S->work_fe), work_fs = fp(S->work_fs), work_spec = fp(S->work_spec), out_spec = fp(S->out_spec);
        plan_windows();
        return DFX_OK;
    }

    // Host bookkeeping of the three windows for this pass: which form owns the state, where the windows are, the copies the pass needs
    // (listed in cp_spec / cp_fe / cp_fs; erb_window / df_window / spec_window enqueue them).  Every change of lin_pos / lin_owns / feat_owns
    // of a pass is made here (this form is never replayed from a graph nor walked hop by hop by the caller).
    void plan_windows() {
        // Rolling spectra: linear (sliding window, see dfx_stream_state::spec_lin) or ring; a handle has one of them for good (lin), so only
        // dfx_stream_process_raw ever takes the state back to the ring form.
        lin = S->lin_cap > 0;
        // The feature windows of the encoder take the same form when the kernels that read them accept a clip stride (the fp16-split DF
        // encoder: DfxC01hArgs::feat_T): [B, feat_cap, E] and [B, feat_cap, Fd, 2] with the same slack as the spectra, so that all three
        // windows sit at lin_pos and go back to the front in the same call.  feat_owns: the linear form holds the feature history.
        const bool feat_lin_ok = lin && capf > 0 && m->can.c0_h3;
        flin = feat_lin_ok && !bypass && skip == 0;   // (warm-up hops zero their features: the ring step does that)
        // (pass-through: the features do not advance, their history waits in the ring form)
        if (!flin) stream_to_ring(S, false, cp_spec, cp_fe, cp_fs);
        spec_win = work_spec, spec_win_T = Hs + n;
        if (lin) {
            float *L0 = fp(S->spec_lin);
            const int64_t cap = S->lin_cap;
            if (!S->lin_owns) {   // the ring form's history becomes the window's first Hs frames
                cp_spec.add(fp(S->hist_spec[S->flip]), Hs * F2, Hs * F2, 0, L0, cap * F2, Hs * F2);
                S->lin_pos = 0;
                S->lin_owns = true;
            } else if (S->lin_pos + Hs + n > cap) {   // the windows have reached the end: their last frames go back to the front (no overlap: lin_pos >= Hs)
                cp_spec.add(L0, cap * F2, cap * F2, S->lin_pos * F2, L0, cap * F2, Hs * F2);
                if (S->feat_owns) {
                    cp_fe.add(fp(S->fe_lin), capf * E, capf * E, S->lin_pos * E, fp(S->fe_lin), capf * E, H * E);
                    cp_fs.add(fp(S->fs_lin), capf * D2, capf * D2, S->lin_pos * D2, fp(S->fs_lin), capf * D2, H * D2);
                }
                S->lin_pos = 0;
            }
            cp_spec.add(new_spec, n * F2, n * F2, 0, L0 + (S->lin_pos + Hs) * F2, cap * F2, n * F2);
            spec_win = L0 + S->lin_pos * F2, spec_win_T = cap;
        }
        fe_win = work_fe, fs_win = work_fs, feat_T = 0;
        norm_fe = new_fe, norm_fs = new_fs, norm_fe_cs = norm_fs_cs = 0;
        if (flin) {
            float *Lfe = fp(S->fe_lin), *Lfs = fp(S->fs_lin);
            if (!S->feat_owns) {   // the ring form's history becomes the windows' first H frames
                cp_fe.add(fp(S->hist_fe[S->flip]), H * E, H * E, 0, Lfe + S->lin_pos * E, capf * E, H * E);
                cp_fs.add(fp(S->hist_fs[S->flip]), H * D2, H * D2, 0, Lfs + S->lin_pos * D2, capf * D2, H * D2);
                S->feat_owns = true;
            }
            fe_win = Lfe + S->lin_pos * E, fs_win = Lfs + S->lin_pos * D2;
            feat_T = capf;
            if (n < 16) {   // the norms write the new frames straight into the windows (no append copies)
                norm_fe = Lfe + (S->lin_pos + H) * E, norm_fs = Lfs + (S->lin_pos + H) * D2;
                norm_fe_cs = capf * E, norm_fs_cs = capf * D2;
            } else {
                cp_fe.add(new_fe, n * E, n * E, 0, Lfe + (S->lin_pos + H) * E, capf * E, n * E);
                cp_fs.add(new_fs, n * D2, n * D2, 0, Lfs + (S->lin_pos + H) * D2, capf * D2, n * D2);
            }
        }
        lin_pos0 = S->lin_pos;   // where this pass's windows are
        if (lin) S->lin_pos += n;
    }

    // pausable handles: this pass's paused rows are flagged behind dfx_k_gate_pre (bump: the hops by which the handle's count will advance)
    int pause_rows(int bump) {
        if (!S->pausable || (silence && !S->any_paused)) return DFX_OK;
        const int ch = S->channels;
        const int64_t ns = B / ch;
        for (int64_t k0 = 0; k0 < ns; k0 += DFX_PAUSE_STREAMS) {
            DfxPauseMask P;
            P.first = (int)k0, P.n = (int)(ns - k0 < DFX_PAUSE_STREAMS ? ns - k0 : DFX_PAUSE_STREAMS);
            memset(P.bits, 0, sizeof(P.bits));
            bool any = false;
            if (S->any_paused)
                for (int k = 0; k < P.n; ++k)
                    if (S->paused[(size_t)(k0 + k)]) P.bits[k >> 5] |= 1u << (k & 31), any = true;
            if (!any && silence) continue;
            dfx_launch(dfx_k_stream_pause, dim3((unsigned)dfx_ceil_div((int64_t)P.n * ch, 256)), dim3(256), 0, s, P, ch, gflags, (int)!silence, gcount,
                       silence ? (const int *)reinterpret_cast<int *>(S->gate_buf + S->g_sh_counter) : (const int *)nullptr,
                       reinterpret_cast<int64_t *>(S->buf + S->birth_dev), bump);
            DFX_LAUNCH_CHECK();
        }
        return DFX_OK;
    }

    // Per-stream forms only: the silent-input test of the pass (gated handles; tract.rs:513-525), the rows that sit it out, and — unless the
    // pass-through follows, which leaves that state alone — the shadow copies of the in-place state.
    int open_gate() {
        if (!gated) return DFX_OK;
        if (silence) {
            if (S->pausable && S->any_paused)
                DFX_HIP(hipMemcpyAsync(S->gate_buf + S->g_sh_counter, S->gate_buf + S->g_counter, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
            if (int r = launch_gate_pre(x, xs, (int)hop, B, gcount, gflags, S->channels, s)) return r;
        }
        if (int r = pause_rows(bypass ? 0 : 1)) return r;
        // (the GRU states: only when the layers run in place — the one-step kernel leaves the old states in the other buffer)
        return bypass ? DFX_OK : stream_shadow_state(S, !step_all, s);
    }

    // who keeps which state (dfx_k_gate_commit), then the frozen streams' answer and the skip counters
    int close_gate(const DfxGateTable &G, bool undecided) {
        dfx_launch(dfx_k_gate_commit, dim3((unsigned)B), dim3(128), 0, s, G, (const unsigned char *)gflags, B);
        DFX_LAUNCH_CHECK();
        dfx_launch(dfx_k_gate_finish, dim3((unsigned)B), dim3(128), 0, s, (const unsigned char *)gflags, gcount, y, ys, (int)hop, lsnr_out, ls, B, (int)undecided);
        DFX_LAUNCH_CHECK();
        return DFX_OK;
    }

    // tract.rs:509-543 with atten_lim == 1: the silent-input counter, the STFT analysis and the rolling spectra still advance (so
    // that switching the limit back mid-stream continues from the right history); features, network and synthesis do not run, the
    // hop is passed through undelayed with lsnr = 35 — unless the stream has been silent for more than 5 hops (zeros, -15).
    int pass_through() {
        int rc;
        if ((rc = dfx_launch_analysis(st, x, B, n * hop, xs, am_in, am_out, new_spec, nullptr, s, -1, Fp))) return rc;
        if ((rc = erb_window(s)) || (rc = df_window(s)) || (rc = spec_window(s))) return rc;
        if ((rc = stream_carry_parity(S, false, true, true, false, s))) return rc;
        if ((rc = stream_copy_rows(x, xs, n * hop, 0, y, ys, n * hop, B, s))) return rc;
        if (lsnr_out) {
            dfx_launch(dfx_k_fill_rows, dim3((unsigned)nn_grid(dfx_ceil_div(B * n, 256), 16)), dim3(256), 0, s, lsnr_out, ls, n, B, 35.f);
            DFX_LAUNCH_CHECK();
        }
        if (!gated) return DFX_OK;
        // frozen streams: zeros / -15, and their analysis memory and rolling spectra stay where they were
        DfxGateTable G;
        G.n = 0;
        G.add(am_out, am_in, ML, DFX_GATE_FROZEN, DFX_GATE_FROZEN);
        if (!lin) G.add(fp(S->hist_spec[S->flip ^ 1]), fp(S->hist_spec[S->flip]), Hs * F2, DFX_GATE_FROZEN, DFX_GATE_FROZEN);   // (linear window: dfx_k_gate_hold)
        return close_gate(G, true /* no stage decision was taken */);
    }

    // ---- STFT + features of the n new hops (state: analysis memory, running means)
    int features() {
        int rc;
        if ((rc = dfx_launch_analysis(st, x, B, n * hop, xs, am_in, nullptr, new_spec, new_fe, s, -1, Fp))) return rc;   // (am_out: spec_window)
        if ((rc = dfx_launch_norm_scan(new_fe, norm_fe, (int)E, new_spec, Fp, norm_fs, (int)Fd, B, n, c.norm_alpha, fp(S->erb_state), fp(S->unit_state), s,
                                       norm_fe_cs, norm_fs_cs)))
            return rc;
        if (skip > 0) DFX_HIP(hipMemsetAsync(out_spec, 0, (size_t)B * n * Fp * 8, s));  // warm-up hops: zero spectra (tract.rs rolling buffers)
        return S->pass_ends ? end_rows() : DFX_OK;
    }

    // Clips that end inside this pass (dfx_stream_process_ends): rule (2) of dfx_enhance_varlen (dfx_model_enhance.h:40-48) — behind a row's last
    // frame its spectrum and its normalised features are zeros, MF.DF's padding (multiframe.py:72-76) and pad_feat's (deepfilternet3.py:359,409-410)
    // — applied where the analysis and the norm scan have just written the new frames: new_spec (every window copy of the pass reads it later) and
    // norm_fe / norm_fs, i.e. the new_* rows or, when the norms write straight into them, the linear windows.  A stream pass makes no pre-split
    // copy of feat_spec.  The counts reach keep [B] as kernel arguments; one dfx_k_zero_tails launch does the rest.
    int end_rows() {
        int64_t *keep = reinterpret_cast<int64_t *>(S->buf + S->keep_dev);
        for (int64_t r0 = 0; r0 < B; r0 += DFX_END_ROWS) {
            DfxEndRows A;
            A.keep = keep, A.row0 = r0;
            A.n = (int)(B - r0 < DFX_END_ROWS ? B - r0 : DFX_END_ROWS);
            for (int i = 0; i < A.n; ++i) A.cnt[i] = S->pass_keep[(size_t)(r0 + i)];
            dfx_launch(dfx_k_stream_end_rows, dim3((unsigned)dfx_ceil_div((int64_t)A.n, 256)), dim3(256), 0, s, A);
            DFX_LAUNCH_CHECK();
        }
        DfxTails t;
        t.add(new_spec, n * F2, n * F2, F2);
        t.add(norm_fe, norm_fe_cs ? norm_fe_cs : n * E, n * E, E);
        t.add(norm_fs, norm_fs_cs ? norm_fs_cs : n * D2, n * D2, D2);
        return dfx_launch_zero_tails(t, keep, B, s);
    }

    // ---- the three windows' enqueue steps.  What only the DF branch needs (the DF feature window) is enqueued on that branch's stream
    // (DfxStreamCtx::df_pre), what only the final deep filter or the NEXT call needs (the spectrum window, the analysis memory) behind df_convp
    // on its stream (DfxStreamCtx::df_post) — in front of the encoder these four small launches were 40 us of a 520 us hop at 4096 streams.
    // A pass that runs no network (warm-up hops, the pass-through) enqueues them itself.
    int hold(float *win, int64_t cap, int64_t row, int64_t h, hipStream_t on) {   // frozen streams keep their history (dfx_k_gate_hold)
        dfx_launch(dfx_k_gate_hold, dim3((unsigned)B, (unsigned)(row > 1024 ? 4 : 1)), dim3(256), 0, on, (const unsigned char *)gflags, win, cap, row, lin_pos0, h, B);
        DFX_LAUNCH_CHECK();
        return DFX_OK;
    }
    int feat_window(DfxCopyList &cp, const size_t *hist, const float *nw, float *work, float *lin_buf, int64_t row, hipStream_t on) {
        if (int r = cp.emit(B, on)) return r;
        if (bypass) return DFX_OK;
        if (!flin) return stream_ring_step(S, hist, nw, work, H, n, row, skip, on);
        return gated ? hold(lin_buf, capf, row, H, on) : DFX_OK;
    }
    int erb_window(hipStream_t on) {
        erb_done = true;
        return feat_window(cp_fe, S->hist_fe, new_fe, work_fe, fp(S->fe_lin), E, on);
    }
    int df_window(hipStream_t on) { return feat_window(cp_fs, S->hist_fs, new_fs, work_fs, fp(S->fs_lin), D2, on); }
    int spec_window(hipStream_t on) {
        side_done = true;
        if (int r = cp_spec.emit(B, on)) return r;
        if (!lin)
            if (int r = stream_ring_step(S, S->hist_spec, new_spec, work_spec, Hs, n, F2, 0, on)) return r;
        if (gated && lin)
            if (int r = hold(fp(S->spec_lin), S->lin_cap, F2, Hs, on)) return r;
        return bypass ? DFX_OK : dfx_launch_analysis_mem(st, x, B, n * hop, xs, am_in, am_out, on);   // (the pass-through's analysis wrote am_out)
    }

    int network() {
        DfxStreamCtx sc;
        sc.H = H + skip;
        const int64_t pos0 = Hs - a0;  // local index of net position 0
        sc.t_zero = pos0 > 0 ? pos0 : 0;
        if (mixed) {
            int *tz = reinterpret_cast<int *>(S->buf + S->tz_rows);
            dfx_launch(dfx_k_stream_tzero, dim3((unsigned)dfx_ceil_div(B, 256)), dim3(256), 0, s, (const int64_t *)reinterpret_cast<int64_t *>(S->buf + S->birth_dev),
                       a0, Hs, tz, B);
            DFX_LAUNCH_CHECK();
            sc.t_zero_rows = tz;
        }
        sc.spec_T = spec_win_T;
        sc.spec_stride = Fp;
        sc.feat_T = feat_T;
        sc.h_state = stream_h(S);
        sc.h_next = step_all ? stream_h(S, true) : nullptr;
        stepped = step_all;
        if (step_all && !gated && S->c0ring_bytes) {   // df_convp from its pending sums (dfx_k_df_convp_step; a gated handle keeps its per-stream delay line)
            const int ns = c.df_pathway_kernel_size_t - 1;
            sc.c0ring = S->buf + S->c0ring;
            sc.c0slot = (int)((((a0 + skip - L) % ns) + ns) % ns);
            sc.c0rebuild = !S->c0ring_ok;
        }
        sc.erb_pre = [this](hipStream_t on) { return erb_window(on); };
        sc.df_pre = [this](hipStream_t on) { return df_window(on); };
        sc.df_post = [this](hipStream_t on) { return spec_window(on); };
        sc.pf_beta = S->pf_beta;
        if (S->lim_rows) sc.lim_rows = reinterpret_cast<const float *>(S->set_buf + S->sb_lim);     // per-stream settings: the finishing kernel
        if (S->beta_rows) sc.beta_rows = reinterpret_cast<const float *>(S->set_buf + S->sb_beta);  //   takes each row's own values
        sc.out = out_spec;  // local frame t of clip b lands at out_spec[(b*n + t - H) * Fp]
        sc.out_T = n;
        sc.out_toff = H;
        sc.channels = S->channels;
        sc.reduce_mask = S->reduce_mask;
        DfxGate gate;
        if (gated) {
            stream_fill_gate(S, silence, gate);
            sc.gate = &gate;
        }
        float *ws = reinterpret_cast<float *>(((uintptr_t)(S->buf + S->model_ws) + 255) & ~(uintptr_t)255);
        if (int rc = forward_conv_ch(c.conv_ch, m, st->bands, spec_win, fe_win, fs_win, B, T, S->lim, nullptr, nullptr, fp(S->lsnr), nullptr, ws, s, &m->lanes[0], false, nullptr, &sc))
            return rc;
        if (stepped) S->hflip ^= 1;   // (like lin_pos: this form is neither replayed from a graph nor walked hop by hop by the caller)
        S->c0ring_ok = sc.c0ring_used;   // any pass that did not go through the step kernel (several hops, gated, run_df off) leaves the sums behind
        return gated ? stream_commit_delay_line(S, T, s) : DFX_OK;
    }

    // the streams of this pass that have no net position yet: zero features, network state and enhanced spectrum
    int warm_rows() {
        DfxRowClear R;
        R.n = 0;
        bool ok = R.add(out_spec, Fp * 8, Fp * 8);
        if (flin) {
            ok = R.add(fp(S->fe_lin) + (lin_pos0 + H) * E, capf * E * 4, E * 4) && ok;
            ok = R.add(fp(S->fs_lin) + (lin_pos0 + H) * D2, capf * D2 * 4, D2 * 4) && ok;
        } else {
            ok = R.add(fp(S->hist_fe[S->flip ^ 1]) + (H - 1) * E, H * E * 4, E * 4) && ok;
            ok = R.add(fp(S->hist_fs[S->flip ^ 1]) + (H - 1) * D2, H * D2 * 4, D2 * 4) && ok;
        }
        ok = R.add(stream_h(S), 1024, 1024, S->layers, B * 1024) && ok;   // (the buffer that holds the states after this pass)
        if (gated) ok = R.add(gflags, 1, 1) && ok;
        ok = stream_convp_rows(S, gated, R) && ok;
        if (!ok) DFX_FAIL(DFX_ERR_UNSUPPORTED, "stream warm-up: more state arrays than DFX_ROWS_MAX_ENTRIES");
        const int *tz = reinterpret_cast<int *>(S->buf + S->tz_rows);
        if (S->pausable) dfx_launch(dfx_k_stream_warm_active, dim3((unsigned)B, 2), dim3(256), 0, s, R, tz, (int)H, gcount, (const unsigned char *)gflags, B);
        else dfx_launch(dfx_k_stream_warm, dim3((unsigned)B, 2), dim3(256), 0, s, R, tz, (int)H, gcount, B);
        DFX_LAUNCH_CHECK();
        return DFX_OK;
    }

    int finish() {
        int rc;
        if (!erb_done && (rc = erb_window(s))) return rc;                              // (no forward pass ran: warm-up hops)
        if (!side_done && ((rc = df_window(s)) || (rc = spec_window(s)))) return rc;
        // ---- ISTFT of the n enhanced hops (state: overlap-add memory)
        if ((rc = dfx_launch_synthesis(st, out_spec, B, n, sm_in, sm_out, y, ys, 0, n * hop, s, 0, -1, Fp))) return rc;
        if (lsnr_out) {  // the window's lsnr is [B, T]: take the n new frames (the entries of warm-up hops are not meaningful)
            if ((rc = stream_copy_rows(fp(S->lsnr), T, T, H, lsnr_out, ls, n, B, s))) return rc;
        }
        if (!gated) return DFX_OK;
        DfxGateTable G;
        G.n = 0;
        const unsigned char FZ = DFX_GATE_FROZEN;
        G.add(am_out, am_in, ML, FZ, FZ);
        G.add(sm_out, sm_in, ML, FZ, FZ);
        if (!flin) {   // (linear windows: dfx_k_gate_hold)
            G.add(fp(S->hist_fe[S->flip ^ 1]), fp(S->hist_fe[S->flip]), H * E, FZ, FZ);
            G.add(fp(S->hist_fs[S->flip ^ 1]), fp(S->hist_fs[S->flip]), H * D2, FZ, FZ);
        }
        if (!lin) G.add(fp(S->hist_spec[S->flip ^ 1]), fp(S->hist_spec[S->flip]), Hs * F2, FZ, FZ);
        G.add(fp(S->erb_state), gp(S->g_sh_erb), E, FZ, FZ);
        G.add(fp(S->unit_state), gp(S->g_sh_unit), Fd, FZ, FZ);
        const int nenc = (int)m->enc_gru.size(), ndec = (int)m->dec_gru.size();
        for (int l = 0; l < S->layers; ++l) {
            float *h = stream_h(S) + (int64_t)l * B * 256;
            const float *hs = (stepped ? stream_h(S, true) : gp(S->g_sh_h)) + (int64_t)l * B * 256;   // the states before this pass
            if (l < nenc) G.add(h, hs, 256, FZ, FZ);
            else if (l < nenc + ndec) G.add(h, hs, 256, DFX_GATE_GAINS, 0);   // stage 1 did not run (frozen streams included)
            else G.add(h, hs, 256, DFX_GATE_DF, 0);                           // stage 2 did not run
        }
        return close_gate(G, skip >= n);
    }
};

static int stream_body(dfx_stream_state *S, const float *x, int64_t n, float *y, float *lsnr_out, hipStream_t s, int64_t xs, int64_t ys, int64_t ls,
                       bool p_mixed, bool p_warm) {
    DfxStreamPass p{S, x, n, y, lsnr_out, s, xs, ys, ls, p_mixed, p_warm, S->m->cfg};
    int rc;
    if ((rc = dfx_ws_fill(S->m, S->buf + S->model_ws, S->model_ws_bytes, s))) return rc;
    if ((rc = p.plan()) || (rc = p.open_gate())) return rc;
    if (p.bypass) return p.pass_through();
    if ((rc = p.features())) return rc;
    if (p.skip < n && ((rc = p.network()) || (p.warm && (rc = p.warm_rows())))) return rc;
    return p.finish();
}

// Faults raised by kernels (dfx_model::h_err): a call reports what earlier passes on the model raised before it starts its own, and — with
// DFX_CHECK_EVERY_PASS=1 — waits for its own pass and reports that too.
static int stream_call_end(const dfx_model *m, hipStream_t s) {
    if (!m->check_every_pass) return DFX_OK;
    DFX_HIP(hipStreamSynchronize(s));
    return model_poll(m);
}
static int stream_process_impl(dfx_stream_state *S, const float *x, int64_t n, float *y, float *lsnr_out, hipStream_t s);
// ---- streaming at the caller's rate, on 16-bit PCM and on G.711 codes ------------------------------------------------------------------
static int stream_stage_alloc(dfx_stream_state *S) {   // the model-rate staging rows [B, nmax * hop]
    if (S->stage_in) return DFX_OK;
    const size_t bytes = (size_t)S->B * S->nmax * S->st->hop * 4;
    if (hipMalloc(reinterpret_cast<void **>(&S->stage_in), bytes) != hipSuccess) DFX_FAIL(DFX_ERR_ALLOC, "dfx_stream: staging rows of %zu bytes", bytes);
    if (hipMalloc(reinterpret_cast<void **>(&S->stage_out), bytes) != hipSuccess) {
        (void)hipFree(S->stage_in);
        S->stage_in = nullptr;
        DFX_FAIL(DFX_ERR_ALLOC, "dfx_stream: staging rows of %zu bytes", bytes);
    }
    return DFX_OK;
}

extern "C" int dfx_stream_set_sample_rate(dfx_stream_state *S, int sr, int lowpass_filter_width, double rolloff, int method, double beta) {
    if (!S || sr <= 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_sample_rate: null handle or bad rate");
    if (!S->fresh) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_set_sample_rate: the handle has consumed hops (set the rate before the first process call, or at a dfx_stream_reset)");
    const int msr = S->st->sr, hop = S->st->hop;
    int64_t g = sr, b = msr;
    while (b) {
        const int64_t t = g % b;
        g = b, b = t;
    }
    const int q = (int)(msr / g);
    if (sr != msr && hop % q)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_set_sample_rate: at %d Hz the model's hop of %d samples (%d Hz) is not a whole number of resampler frames (the hop must be a multiple of %d)",
                 sr, hop, msr, q);
    if (int rc = dfx_require_device()) return rc;
    stream_rate_clear(S);
    if (sr == msr) return DFX_OK;
    const int64_t h = (int64_t)hop / q * (sr / g);
    int rc;
    if ((rc = dfx_resampler_create(sr, msr, lowpass_filter_width, rolloff, method, beta, &S->rs_up)) ||
        (rc = dfx_resampler_create(msr, sr, lowpass_filter_width, rolloff, method, beta, &S->rs_dn)) ||
        (rc = dfx_stream_resampler_create(S->rs_up, S->B, (int64_t)S->nmax * h, &S->up)) ||
        (rc = dfx_stream_resampler_create(S->rs_dn, S->B, (int64_t)S->nmax * hop, &S->dn)) || (rc = stream_stage_alloc(S))) {
        stream_rate_clear(S);
        return rc;
    }
    if (hipMalloc(&S->thru_tmp, (size_t)S->B * S->nmax * h * 4) != hipSuccess) {
        stream_rate_clear(S);
        DFX_FAIL(DFX_ERR_ALLOC, "dfx_stream_set_sample_rate: device allocation failed");
    }
    S->sr = sr, S->hop_native = h;
    S->rs_width = lowpass_filter_width, S->rs_method = method, S->rs_rolloff = rolloff, S->rs_beta = beta;
    return DFX_OK;
}
extern "C" int dfx_stream_sample_rate(const dfx_stream_state *S) { return S ? (S->sr ? S->sr : S->st->sr) : 0; }
extern "C" int64_t dfx_stream_resample_delay(const dfx_stream_state *S) {
    if (!S || !S->sr) return 0;
    int64_t pu = 0, pd = 0;
    (void)dfx_stream_resampler_delay(S->up, &pu, nullptr);
    (void)dfx_stream_resampler_delay(S->dn, nullptr, &pd);   // (the down-sampler's delay in ITS output samples: the caller's rate)
    return pu + pd;
}

// The pass between the converters (a rate is set) or between the PCM / G.711 kernels (16-bit PCM or codes at the model's rate): x -> stage_in
// -> the model-rate pass, unchanged -> stage_out -> y, all on the caller's stream.  fmt: the DFX_FMT_* of x and y, a property of the call.
static int stream_process_staged(dfx_stream_state *S, const void *x, int64_t n, void *y, int fmt, float *lsnr_out, hipStream_t s) {
    const int64_t B = S->B, T = n * S->st->hop;
    const bool g711 = fmt == DFX_FMT_ULAW || fmt == DFX_FMT_ALAW;
    const int law = fmt - DFX_FMT_ULAW + DFX_G711_ULAW;                   // (of a G.711 call)
    const size_t sample = fmt == DFX_FMT_F32 ? 4 : (fmt == DFX_FMT_PCM16 ? 2 : 1);
    const int quiet = g711 ? (law == DFX_G711_ULAW ? 0xFF : 0xD5) : 0;             // the byte a row of silence is filled with
    // (the handle-wide pass-through: the model-rate pass hands stage_in through and moves its STFT memory)
    const bool thru = S->lim == 1.f;
    int rc;
    const unsigned char *act = nullptr;
    if (S->any_paused && (S->sr || (g711 && thru))) {   // a paused stream's rows sit both converters out
        const int ch = S->channels;
        S->row_active.resize((size_t)B);
        for (int64_t r = 0; r < B; ++r) S->row_active[(size_t)r] = !S->paused[(size_t)(r / ch)];
        act = S->row_active.data();
    }
    // the caller's own samples back, as they came (G.711: the bytes, not a re-encoding — 0x7F stays 0x7F); a paused stream's rows: silence
    auto hand_back = [&](size_t row) -> int {
        DFX_HIP(hipMemcpyAsync(y, x, (size_t)B * row, hipMemcpyDeviceToDevice, s));
        for (int64_t r = 0; act && r < B; ++r)
            if (!act[r]) DFX_HIP(hipMemsetAsync(static_cast<unsigned char *>(y) + (size_t)r * row, quiet, row, s));
        return DFX_OK;
    };
    if (!S->sr) {
        if (g711) {
            if ((rc = dfx_g711_decode(static_cast<const uint8_t *>(x), law, B * T, S->stage_in, 0, s))) return rc;
            if ((rc = stream_process_impl(S, S->stage_in, n, S->stage_out, lsnr_out, s))) return rc;
            if (thru) return hand_back((size_t)T);
            return dfx_g711_encode(S->stage_out, 0, law, B * T, static_cast<uint8_t *>(y), s);
        }
        if ((rc = dfx_pcm16_to_f32(static_cast<const int16_t *>(x), B * T, S->stage_in, s))) return rc;
        if ((rc = stream_process_impl(S, S->stage_in, n, S->stage_out, lsnr_out, s))) return rc;
        return dfx_f32_to_pcm16(S->stage_out, B * T, static_cast<int16_t *>(y), s);
    }
    const int64_t Tn = n * S->hop_native;
    // (in the pass-through the down-sampler's history follows the model-rate rows, its output is dropped and the caller gets its own samples back)
    if ((rc = dfx_stream_resampler_process(S->up, x, fmt, Tn, Tn, S->stage_in, DFX_FMT_F32, T, act, s))) return rc;
    if ((rc = stream_process_impl(S, S->stage_in, n, S->stage_out, lsnr_out, s))) return rc;
    if ((rc = dfx_stream_resampler_process(S->dn, S->stage_out, DFX_FMT_F32, T, T, thru ? S->thru_tmp : y, thru ? DFX_FMT_F32 : fmt, Tn, act, s))) return rc;
    if (thru) return hand_back((size_t)Tn * sample);
    return DFX_OK;
}

// valid (dfx_stream_process_ends; host [B] or null): the hops of this call that lie inside each row's clip.
static int stream_process_any(dfx_stream_state *S, const void *x, int64_t n, void *y, int fmt, float *lsnr_out, const unsigned char *active,
                              void *stream, const int64_t *valid = nullptr) {
    if (!S || n <= 0 || n > S->nmax || !x || !y) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process: bad arguments (1 <= n_frames <= max_frames)");
    if (active && !S->pausable) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_active: a mask needs a pausable handle (dfx_stream_set_pausable)");
    if (S->lim == 1.f) valid = nullptr;   // (the handle-wide pass-through runs no network: nothing reads the frames behind an end)
    bool ends = false;
    for (int64_t b = 0; valid && b < S->B; ++b) {
        if (valid[b] < 0 || valid[b] > n)
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_ends: valid_hops[%lld] = %lld is not in [0, n_frames = %lld]", (long long)b, (long long)valid[b], (long long)n);
        if (S->ended[(size_t)b] && valid[b] != 0)
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_ends: stream %lld has ended (valid_hops must be 0 until dfx_stream_reset_streams), got %lld", (long long)b,
                     (long long)valid[b]);
        ends |= valid[b] < n;
    }
    if (int rc = dfx_require_device()) return rc;
    if (int rc = model_poll(S->m)) return rc;
    hipStream_t s = dfx_stream(stream);
    S->any_paused = false;
    if (S->pausable) {   // the mask of this call, on the host: it reaches the kernels as arguments (dfx_k_stream_pause)
        const size_t ns = (size_t)(S->B / S->channels);
        S->paused.assign(ns, 0);
        for (size_t k = 0; active && k < ns; ++k)
            if (!active[k]) S->paused[k] = 1, S->any_paused = true;
    }
    const bool staged = S->sr != 0 || fmt != DFX_FMT_F32;
    if (staged)
        if (int rc = stream_stage_alloc(S)) return rc;
    {
        DfxTurn turn(S->m, s, false);   // (the enqueue lock only: a hop starts no persistent phase)
        S->fresh = false;
        S->call_valid = ends ? valid : nullptr;   // (no row ends in this call: it enqueues what a call without counts enqueues)
        const int rc = staged ? stream_process_staged(S, x, n, y, fmt, lsnr_out, s)
                              : stream_process_impl(S, static_cast<const float *>(x), n, static_cast<float *>(y), lsnr_out, s);
        S->call_valid = nullptr;
        if (rc) return rc;
        for (int64_t b = 0; ends && b < S->B; ++b)
            if (valid[b] < n && !S->ended[(size_t)b]) S->ended[(size_t)b] = 1, ++S->n_ended;
    }
    return stream_call_end(S->m, s);
}
// Clips that end inside a call: valid_hops[b] = v (host, [streams]) says that the first v hops of this call are the last frames of row b's clip;
// the frames behind them — in this call and in every later one, until the row is reset — are MF.DF's and pad_feat's zero padding behind a clip
// (multiframe.py:72-76, deepfilternet3.py:359,409-410), as in dfx_enhance_varlen, so that the row's output is dfx_enhance(pad=0) of exactly its
// own frames, delayed, its last `lookahead` frames included.
extern "C" int dfx_stream_process_ends(dfx_stream_state *S, const void *x, int x_format, int64_t n, void *y, float *lsnr_out, const int64_t *valid_hops,
                                       void *stream) {
    if (!S) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_ends: null handle");
    if (x_format != DFX_FMT_F32 && x_format != DFX_FMT_PCM16)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_ends: x_format %d (DFX_FMT_F32 or DFX_FMT_PCM16)", x_format);
    if (S->gated || S->pausable || S->channels > 1 || S->sr)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_process_ends: not on a gated or pausable handle, with channels > 1 or at a caller's sample rate");
    return stream_process_any(S, x, n, y, x_format, lsnr_out, nullptr, stream, valid_hops);
}
// The device bytes dfx_stream_create(m, st, streams, max_frames) allocates for a handle without a sample rate: its state and window buffer, and the
// two staging rows [streams, max_frames * hop] that the first 16-bit PCM (or G.711) call adds.  No device access.
extern "C" int dfx_stream_memory_bytes(const dfx_model *m, const dfx_state *st, int64_t streams, int max_frames, int64_t *bytes) {
    if (!bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_memory_bytes: bad arguments");
    if (int rc = stream_create_check(m, st, streams, max_frames, "dfx_stream_memory_bytes")) return rc;
    dfx_stream_state s;
    s.m = m, s.st = st, s.B = streams, s.nmax = max_frames;
    stream_layout(&s);
    *bytes = (int64_t)s.bytes + 2 * (int64_t)((size_t)streams * max_frames * st->hop * 4);
    return DFX_OK;
}
extern "C" int dfx_stream_process_active(dfx_stream_state *S, const float *x, int64_t n, float *y, float *lsnr_out, const unsigned char *active,
                                         void *stream) {
    return stream_process_any(S, x, n, y, DFX_FMT_F32, lsnr_out, active, stream);
}
extern "C" int dfx_stream_process(dfx_stream_state *S, const float *x, int64_t n, float *y, float *lsnr_out, void *stream) {
    return stream_process_any(S, x, n, y, DFX_FMT_F32, lsnr_out, nullptr, stream);
}
extern "C" int dfx_stream_process_pcm16(dfx_stream_state *S, const int16_t *x, int64_t n, int16_t *y, float *lsnr_out, const unsigned char *active,
                                        void *stream) {
    return stream_process_any(S, x, n, y, DFX_FMT_PCM16, lsnr_out, active, stream);
}
extern "C" int dfx_stream_process_g711(dfx_stream_state *S, const uint8_t *x, int law, int64_t n, uint8_t *y, float *lsnr_out, const unsigned char *active,
                                       void *stream) {
    if (law != DFX_G711_ULAW && law != DFX_G711_ALAW) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_g711: law %d (DFX_G711_ULAW or DFX_G711_ALAW)", law);
    return stream_process_any(S, x, n, y, law - DFX_G711_ULAW + DFX_FMT_ULAW, lsnr_out, active, stream);
}
// A call of n hops as passes.  A hop is passed on its own while the handle keeps per-stream forms (gated, pausable: the stage decisions of
// hop i shape the state hop i+1 starts from) or sits inside the warm-up of a stream that started over on its own
// (dfx_stream_reset_streams); otherwise the rest of the call is one pass.
static int stream_process_impl(dfx_stream_state *S, const float *x, int64_t n, float *y, float *lsnr_out, hipStream_t s) {
    const bool advances = S->lim != 1.f;  // the pass-through case (tract.rs:540-543) moves the STFT memory and the rolling spectra only
    const bool per_stream = (S->gated || S->pausable) && S->gate_buf;
    const int ch = S->channels;
    const int64_t hop = S->st->hop, ns = S->B / ch, Hs = S->H + S->L;
    for (int64_t done = 0, k; done < n; done += k) {
        k = per_stream || (advances && S->frames < S->warm_until) ? 1 : n - done;
        bool mixed = S->frames < S->mixed_until, warm = S->frames < S->warm_until;
        if (S->pausable) {
            // Whether a pass takes the per-row t_zero (a stream younger than the window and than the handle) and the warm-up (younger than the
            // lookahead) follows the ages of the streams that take part: a young stream that sits out keeps nobody in those forms.
            mixed = warm = false;
            for (int64_t i = 0; i < ns; ++i) {
                const int64_t born = S->birth[(size_t)(i * ch)], age = S->frames - born;
                if (S->paused[(size_t)i] || born == 0 || age >= Hs) continue;
                mixed = true;
                if (age < S->L) warm = true;
            }
        }
        S->pass_ends = false;
        if ((S->call_valid || S->n_ended) && advances) {   // the hops of this pass that lie inside each row's clip: valid_hops less the hops of the earlier passes
            S->pass_keep.resize((size_t)S->B);
            for (int64_t b = 0; b < S->B; ++b) {
                const int64_t v = S->ended[(size_t)b] ? 0 : (S->call_valid ? S->call_valid[b] - done : k);
                S->pass_keep[(size_t)b] = (int)(v < 0 ? 0 : (v > k ? k : v));
                S->pass_ends |= v < k;
            }
        }
        if (int rc = stream_body(S, x + done * hop, k, y + done * hop, lsnr_out ? lsnr_out + done : nullptr, s, n * hop, n * hop, n, mixed, warm)) return rc;
        if (advances) {
            S->frames += k;
            // after the pass the paused streams' births follow the handle's count (dfx_k_stream_pause did the same)
            for (int64_t i = 0; S->any_paused && i < ns; ++i)
                if (S->paused[(size_t)i])
                    for (int j = 0; j < ch; ++j) S->birth[(size_t)(i * ch + j)] += k;
        }
        S->flip ^= 1;
    }
    return DFX_OK;
}

// DfTract::process_raw (tract.rs:441-507; exported as df_process_frame_raw, capi.rs:172-210): one *spectral* frame per stream in, the
// raw ERB gains and deep-filter coefficients of that pass out — features with the running means, encoder, stage decisions, the
// decoders that the decision selects (their state only moves when they run).  No STFT, no deep filtering, no synthesis, and (like the
// reference) neither the rolling spectra nor the silent-input counter are touched.  Needs gating (dfx_stream_set_gating); a handle
// should be driven either by dfx_stream_process or by this function, not by both.
//   spec [streams, F][2] -> gains [streams, nb_erb], coefs [streams, df_order, nb_df][2], stages [streams]: bit 1 (2) = gains present
//   (the network's mask, or zeros when lsnr < min_db_thresh), bit 3 (8) = coefficients present; a caller maps absent to NULL.
extern "C" int dfx_stream_process_raw(dfx_stream_state *S, const float *spec, float *gains, float *coefs, unsigned char *stages, float *lsnr_out,
                                      void *stream) {
    if (!S || !spec || !gains || !coefs || !stages) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_raw: null argument");
    if (!S->gated || !S->gate_buf) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_process_raw: switch gating on first (dfx_stream_set_gating)");
    if (S->frames < S->mixed_until)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_process_raw: a stream reset by dfx_stream_reset_streams is younger than the window (the raw path has one start for all streams)");
    if (S->pausable)   // (a stream that sat calls out is younger than the handle in the same way)
        for (int64_t k = 0; k < S->B; ++k)
            if (S->birth[(size_t)k] != 0 && S->frames - S->birth[(size_t)k] < S->H + S->L)
                DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_stream_process_raw: a stream that was reset or paused is younger than the window (the raw path has one start for all streams)");
    if (int rc = dfx_require_device()) return rc;
    if (int rc = model_poll(S->m)) return rc;
    hipStream_t s = dfx_stream(stream);
    DfxTurn turn(S->m, s, false);   // (the enqueue lock)
    S->fresh = false;
    const dfx_model *m = S->m;
    if (int rc = dfx_ws_fill(m, S->buf + S->model_ws, S->model_ws_bytes, s)) return rc;
    const dfx_state *st = S->st;
    const dfx_model_cfg &c = m->cfg;
    const int64_t B = S->B, H = S->H, L = S->L, Hs = H + L, F = st->N / 2 + 1, E = c.nb_erb, Fd = c.nb_df;
    const int64_t n = 1, T = H + n, a0 = S->frames;
    const int O = c.df_order;
    unsigned char *gflags = S->gate_buf + S->g_flags;
    int rc;
    // this path keeps the windows in ring form: if an earlier call on the handle left them in the linear buffers, their last frames
    // become the ring form's history first
    DfxCopyList cp_spec, cp_fe, cp_fs;
    stream_to_ring(S, true, cp_spec, cp_fe, cp_fs);
    if ((rc = cp_fe.emit(B, s)) || (rc = cp_fs.emit(B, s)) || (rc = cp_spec.emit(B, s))) return rc;
    DFX_HIP(hipMemsetAsync(gflags, 0, (size_t)B, s));  // no silent-input test on this path (tract.rs:441: process_raw starts at the features)
    if ((rc = stream_shadow_state(S, true, s))) return rc;
    // features of the given spectra (state: the running means): erb (dB) -> mean norm, low bins -> unit norm (lib.rs:206-217)
    float *new_fe = stream_fp(S, S->new_fe), *new_fs = stream_fp(S, S->new_fs);   // (the caller's dense [B, F] spectra are read in place)
    if ((rc = dfx_erb(st->bands, spec, B, 1, new_fe, s))) return rc;
    if ((rc = dfx_launch_norm_scan(new_fe, new_fe, (int)E, spec, F, new_fs, (int)Fd, B, n, c.norm_alpha, stream_fp(S, S->erb_state),
                                   stream_fp(S, S->unit_state), s)))
        return rc;
    const int64_t skip = a0 < L ? 1 : 0;
    float *work_fe = stream_fp(S, S->work_fe), *work_fs = stream_fp(S, S->work_fs);
    if ((rc = stream_ring_step(S, S->hist_fe, new_fe, work_fe, H, n, E, skip, s)) || (rc = stream_ring_step(S, S->hist_fs, new_fs, work_fs, H, n, Fd * 2, skip, s)))
        return rc;
    if ((rc = stream_carry_parity(S, true, true, false, true, s))) return rc;
    float *mask = stream_gp(S, S->g_mask), *cbuf = stream_gp(S, S->g_coefs);
    if (!skip) {
        DfxStreamCtx sc;
        sc.H = H;
        const int64_t pos0 = Hs - a0;
        sc.t_zero = pos0 > 0 ? pos0 : 0;
        sc.spec_T = Hs + n;
        sc.spec_stride = S->Fp;
        sc.h_state = stream_h(S);
        sc.pf_beta = 0.f;
        sc.out = stream_fp(S, S->out_spec);  // the deep-filter kernel still runs (on whatever the spectrum window holds); its output is not used
        sc.out_T = n;
        sc.out_toff = H;
        sc.channels = S->channels;
        sc.reduce_mask = S->reduce_mask;
        DfxGate gate;
        stream_fill_gate(S, true, gate);
        sc.gate = &gate;
        float *ws = reinterpret_cast<float *>(((uintptr_t)(S->buf + S->model_ws) + 255) & ~(uintptr_t)255);
        if ((rc = forward_conv_ch(c.conv_ch, m, st->bands, stream_fp(S, S->work_spec), work_fe, work_fs, B, T, 0.f, nullptr, mask, stream_fp(S, S->lsnr), cbuf, ws, s, &m->lanes[0], false, nullptr, &sc)))
            return rc;
        if ((rc = stream_commit_delay_line(S, T, s))) return rc;
        // the newest frame's mask row and coefficient rows (coefficients are [B, O, T, F'][2]: one strided row per (stream, tap))
        if ((rc = stream_copy_rows(mask, T * E, T * E, (T - 1) * E, gains, E, E, B, s))) return rc;
        if ((rc = stream_copy_rows(cbuf, T * Fd * 2, T * Fd * 2, (T - 1) * Fd * 2, coefs, Fd * 2, Fd * 2, B * O, s))) return rc;
        if (lsnr_out && (rc = stream_copy_rows(stream_fp(S, S->lsnr), T, T, H, lsnr_out, 1, 1, B, s))) return rc;
        // decoder states of the stages that did not run go back to what they were
        DfxGateTable G;
        G.n = 0;
        const int nenc = (int)m->enc_gru.size(), ndec = (int)m->dec_gru.size();
        for (int l = nenc; l < S->layers; ++l)
            G.add(stream_h(S) + (int64_t)l * B * 256, stream_gp(S, S->g_sh_h) + (int64_t)l * B * 256, 256, l < nenc + ndec ? DFX_GATE_GAINS : DFX_GATE_DF, 0);
        dfx_launch(dfx_k_gate_commit, dim3((unsigned)B), dim3(128), 0, s, G, (const unsigned char *)gflags, B);
        DFX_LAUNCH_CHECK();
    } else if (lsnr_out) {
        dfx_launch(dfx_k_fill_rows, dim3((unsigned)nn_grid(dfx_ceil_div(B, 256), 16)), dim3(256), 0, s, lsnr_out, (int64_t)1, (int64_t)1, B, -15.f);
        DFX_LAUNCH_CHECK();
    }
    // stages: bit 2 = gains exist (the network's mask, or zeros below min_db_thresh: the reference returns Some(zeros) there,
    // tract.rs:485-486), bit 8 = coefficients exist
    dfx_launch(dfx_k_gate_stages, dim3((unsigned)dfx_ceil_div(B, 256)), dim3(256), 0, s, (const unsigned char *)gflags, stages, B);
    DFX_LAUNCH_CHECK();
    S->frames += 1;
    S->flip ^= 1;
    return stream_call_end(m, s);
}

// Batch-chunk pipelining: the GRU chain of a chunk is a long latency chain on a handful of CUs, so dfx_enhance splits the
// batch into up to DFX_MAX_LANES chunks (multiples of the 16 clips a GRU workgroup owns), each with its own streams; the
// chip-filling "front" (features, encoder convolutions) of chunk c+1 is released when chunk c has enqueued its front, and
// then overlaps chunk c's GRU chain; the tails overlap likewise.  Chunks are independent clips, so results do not change.
