// DeepFilterNet3 model handle: tensor manifest, BatchNorm folding + weight re-layout, workspace planning and the kernel
// sequence of DfNet.forward (deepfilternet3.py:389-456) and enhance() (enhance.py:206-250).
#include "dfx_manifest.h"
#include "dfx_nn_kernels.h"

#include <cmath>
#include <functional>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

// ------------------------------------------------------------------------------------------------ cfg validation
static int check_cfg(const dfx_model_cfg *c) {
    if (!c) DFX_FAIL(DFX_ERR_INVALID_ARG, "null model cfg");
    if (c->conv_ch != 16 && c->conv_ch != 32 && c->conv_ch != 64)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "conv_ch=%d: the HIP kernels are instantiated for 16, 32, 64", c->conv_ch);
    if (c->emb_hidden_dim != 256 || c->df_hidden_dim != 256) DFX_FAIL(DFX_ERR_UNSUPPORTED, "GRU hidden size must be 256");
    if (c->nb_erb <= 0 || c->nb_erb % 8 || c->nb_erb > 64) DFX_FAIL(DFX_ERR_UNSUPPORTED, "nb_erb must be a multiple of 8, <= 64");
    // the ERB decoder's last two layers run frame-resident (dfx_k_erb_dec10) at every shape these bounds accept: nb_erb is even and two workgroups
    // fit the LDS at the largest one.  Widening either bound means bringing the layer-by-layer end (convt1, then conv0_out) back.
    static_assert(2 * DFX_DEC10_SMEM(64, 64) <= 160 * 1024, "conv_ch <= 64, nb_erb <= 64: dfx_k_erb_dec10 must fit every accepted shape");
    if (c->nb_df <= 0 || c->nb_df % 2 || c->nb_df > c->fft_size / 2 + 1) DFX_FAIL(DFX_ERR_UNSUPPORTED, "nb_df must be even and <= F");
    if (c->df_order <= 0 || c->df_order > 16 || c->df_lookahead < 0 || c->df_lookahead >= c->df_order)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "need 0 <= df_lookahead < df_order <= 16");
    if (c->conv_lookahead < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "conv_lookahead < 0");
    if (c->emb_num_layers < 2 || c->df_num_layers < 1) DFX_FAIL(DFX_ERR_UNSUPPORTED, "emb_num_layers >= 2 and df_num_layers >= 1 required");
    if (c->df_pathway_kernel_size_t < 1 || c->df_pathway_kernel_size_t > 8) DFX_FAIL(DFX_ERR_UNSUPPORTED, "df_pathway_kernel_size_t must be 1..8");
    const int emb = c->conv_ch * c->nb_erb / 4;
    auto div_ok = [&](int I, int H, int G) { return G > 0 && I % G == 0 && H % G == 0 && (I / G) % 4 == 0 && (H / G) % 4 == 0; };
    if (!div_ok(c->conv_ch * c->nb_df / 2, emb, c->enc_lin_groups)) DFX_FAIL(DFX_ERR_UNSUPPORTED, "enc_linear_groups=%d does not tile df_fc_emb into multiples of 4", c->enc_lin_groups);
    if (!div_ok(emb, 256, c->lin_groups) || !div_ok(256, emb, c->lin_groups) || !div_ok(emb, 256, 8) ||
        !div_ok(256, c->nb_df * 2 * c->df_order, c->lin_groups))
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "linear_groups=%d does not tile the grouped linears into multiples of 4", c->lin_groups);
    const int G = dfx_gcd(c->conv_ch, 2 * c->df_order);
    if ((c->conv_ch / G) % 4 || (2 * c->df_order / G) > 16) DFX_FAIL(DFX_ERR_UNSUPPORTED, "df_convp group shape unsupported");
    if (c->df_gru_skip == DFX_SKIP_IDENTITY && emb != 256) DFX_FAIL(DFX_ERR_INVALID_ARG, "df_gru_skip=identity needs emb_dim == 256");
    if (c->df_gru_skip < 0 || c->df_gru_skip > 2) DFX_FAIL(DFX_ERR_INVALID_ARG, "bad df_gru_skip");
    if (c->emb_gru_skip_enc < 0 || c->emb_gru_skip_enc > 2 || c->emb_gru_skip < 0 || c->emb_gru_skip > 2 || (c->enc_concat & ~1))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "bad emb_gru_skip_enc / emb_gru_skip / enc_concat");
    // deepfilternet3.py:138-146: with enc_concat the encoder GRU's input is twice as wide as its output; identity then fails the
    // reference's own assert and the grouped-linear skip (built for emb_out_dim inputs) cannot take it either
    if (c->enc_concat && c->emb_gru_skip_enc != DFX_SKIP_NONE) DFX_FAIL(DFX_ERR_INVALID_ARG, "enc_concat excludes emb_gru_skip_enc (dimensions do not match)");
    if (!div_ok(2 * emb, 256, c->lin_groups) && c->enc_concat) DFX_FAIL(DFX_ERR_UNSUPPORTED, "linear_groups does not tile the concatenated embedding");
    if ((c->emb_gru_skip_enc == DFX_SKIP_GROUPEDLINEAR || c->emb_gru_skip == DFX_SKIP_GROUPEDLINEAR) && !div_ok(emb, emb, c->lin_groups))
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "linear_groups does not tile the embedding skip into multiples of 4");
    return DFX_OK;
}

// ------------------------------------------------------------------------------------------------ manifest API
extern "C" int dfx_model_tensor_count(const dfx_model_cfg *cfg, int *count) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!count) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    *count = (int)dfx_build_manifest(*cfg).t.size();
    return DFX_OK;
}
extern "C" int dfx_model_tensor_info(const dfx_model_cfg *cfg, int index, char *name_out, int name_cap,
                                     int64_t shape_out[4], int *ndim_out, int64_t *offset_out) {
    if (int rc = check_cfg(cfg)) return rc;
    const DfxManifest m = dfx_build_manifest(*cfg);
    if (index < 0 || index >= (int)m.t.size()) DFX_FAIL(DFX_ERR_INVALID_ARG, "tensor index out of range");
    const DfxTensor &t = m.t[index];
    if (name_out && name_cap > 0) snprintf(name_out, (size_t)name_cap, "%s", t.name.c_str());
    if (shape_out)
        for (int i = 0; i < 4; ++i) shape_out[i] = i < t.ndim ? t.shape[i] : 1;
    if (ndim_out) *ndim_out = t.ndim;
    if (offset_out) *offset_out = t.offset;
    return DFX_OK;
}
extern "C" int dfx_model_blob_floats(const dfx_model_cfg *cfg, int64_t *n) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!n) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    *n = dfx_build_manifest(*cfg).total;
    return DFX_OK;
}

// ------------------------------------------------------------------------------------------------ prepared weights
struct PwW {   // separable conv block: depthwise + pointwise(+BN) [+ pathway skip scalars]
    size_t dw = 0, wt = 0, bias = 0, sk_a = 0, sk_b = 0;
    bool has_skip = false;
    size_t wt_h3 = 0;       // pointwise weights as pre-scaled f16 hi/lo MFMA fragments (dfx_chain_stage_h3) ...
    bool has_h3 = false;    // ... which pack_pw_h3 made for this block (the six ERB blocks where C % 32 == 0; df_conv1 has its own order: dfc1_h3)
    float unscale = 1.f;
};
struct GruW {
    size_t wih_t = 0, bias_i = 0, whh4 = 0, bhn = 0;
    size_t wih_h3 = 0;      // W_ih as pre-scaled f16 hi/lo MFMA fragments (dfx_k_proj256_h3)
    float wih_unscale = 1.f;
    size_t whh_h3 = 0;      // W_hh as pre-scaled f16 hi/lo MFMA fragments (dfx_k_gru_rec_h3)
    float whh_unscale = 1.f;
    size_t whh_pj = 0;      // W_hh in the projection kernel's fragment order (dfx_k_gru_step_h3: one time step of many streams), same scale
    size_t whh_x32 = 0;     // W_hh as fp32 fragments in dfx_k_gru_rec_h3's order (dfx_k_gru_rec_x32: the exact recurrence of the layer-pipelined phase)
    size_t wih_x32 = 0;     // W_ih in the same fp32 fragment order, exact models only (dfx_k_gru_step_x32: one time step of many streams; it reads W_hh from whh_x32)
    bool has_wih_x32 = false;
};
struct GlinW {
    size_t w = 0;
    int G = 0, Kg = 0, Ng = 0;
};

#define DFX_MAX_LANES 4
#define DFX_LANE_EVENTS 12
#define DFX_THROTTLE_MIN_FRAMES 16384   /* passes of at least this many frames are enqueued one at a time (dfx_model::ev_pass) */
#define DFX_MAX_GRU_LAYERS 8   /* all GRU layers of the three stacks */
static_assert(DFX_MAX_GRU_LAYERS == DFX_GS_MAX_LAYERS, "the host lays the XCD / progress tables out with the stride the kernels index them with");
#define DFX_MAX_TCHUNKS 16     /* time chunks of the layer-pipelined GRU phase */
#define DFX_SEQ_GMAX 64        /* most 16-clip groups per layer the persistent GRU phase is used for (all workgroups must be co-resident) */
struct DfxLane;
struct DfxLane {
    hipStream_t main = nullptr;
    hipStream_t aux[2] = {nullptr, nullptr};
    hipEvent_t ev[DFX_LANE_EVENTS] = {};
    hipStream_t gs[DFX_MAX_GRU_LAYERS] = {};                      // recurrence stream of GRU layer l
    hipStream_t ps[DFX_MAX_GRU_LAYERS] = {};                      // preparation stream of GRU layer l (linear_in, projection)
    hipStream_t ts[2] = {};                                       // tails of the ERB / DF decoder
    hipEvent_t gev[DFX_MAX_GRU_LAYERS][DFX_MAX_TCHUNKS] = {};     // layer l has produced time chunk k
    hipEvent_t pev[DFX_MAX_GRU_LAYERS][DFX_MAX_TCHUNKS] = {};     // gi of layer l, chunk k is ready
    hipEvent_t eev[DFX_MAX_TCHUNKS] = {};                         // emb chunk k is ready
};
// The internal streams and events of a process on one device (created on demand, kept for the life of the process) and what the handshake of
// the persistent GRU phase found about them (hwq_probe: -1 not run, 1 concurrent, 0 not).
struct DfxLaneSet {
    DfxLane lanes[DFX_MAX_LANES];
    int hwq_probe = -1;
};
// enhance() hands the synthesis to the model forward so that it runs behind the deep filter on the stream that carries the last coefficients
struct DfxFinish {
    const dfx_state *st;
    float *y;
    int64_t out_stride, out_skip, out_len;
    int64_t spec_stride;   // row stride (complex elements) of enhance()'s own spec / spec_e buffers: F rounded up to even, so that
                           // every row is 16-byte aligned (dfx_k_df_apply_rows); dfx_model_forward's caller-owned arrays are dense
    bool out_i16 = false;  // y points at int16_t PCM samples (dfx_enhance_pcm16)
    bool feat_ps_made = false;   // the pre-split copy of feat_spec is already in the model workspace (Ws::fps: the norm scan wrote it)
};
// Streaming (dfx_stream_process): a forward pass over a window.  Every feature / activation array holds T = H + n frames per clip
// (H history frames, then the n new ones); only the new frames are computed (kernels take t_begin, per-frame kernels a DfxRowMap),
// the GRUs continue from h_state, the spec array has spec_T = T + lookahead frames and the enhanced spectra are stored compactly.
struct DfxStreamCtx {
    int64_t H;         // history frames in front of the new ones
    int64_t t_zero;    // local frames < t_zero precede the start of the stream (df_convp sees zero padding there)
    const int *t_zero_rows = nullptr;   // non-null: t_zero per stream [B] (some streams started over later than the handle: dfx_stream_reset_streams)
    int64_t spec_T;    // frames per clip of the spec array
    int64_t spec_stride = 0;   // > 0: bins per row of spec and out (padded rows)
    int64_t feat_T = 0;    // > 0: frames per clip of feat_erb and feat_spec (windows inside the linear buffers; both share it)
    float *h_state;    // [GRU layers][B][256], in model order enc, erb_dec, df_dec
    float *h_next = nullptr;   // non-null (one new frame, ungated): the layers run as dfx_k_gru_step_h3 and leave their new states HERE
    void *c0ring = nullptr;    // non-null (one new frame, ungated): df_convp keeps the pending sums of its next kt - 1 outputs here (dfx_k_df_convp_step)
    int c0slot = 0;            //   slot of the new frame = its net position % (kt - 1)
    bool c0rebuild = false;    //   the sums are not current: recompute the older frames' taps from the feature window
    mutable bool c0ring_used = false;   //   out: dfx_k_df_convp_step ran in this pass (only then are the sums current afterwards)
    std::function<int(hipStream_t)> erb_pre;  // set: the ERB feature window's update, enqueued on the caller's stream BEHIND the event the DF branch
                                              //   starts on (that branch's chain to c1 is the longer one)
    std::function<int(hipStream_t)> df_pre;   // set: state updates that only the DF branch reads — enqueued on that branch's stream before its
                                              //   first kernel instead of in front of the encoder
    std::function<int(hipStream_t)> df_post;  // set: state updates that nothing before the final deep filter reads — enqueued behind df_convp on
                                              //   its stream (joined through EV_C0P before df_out), or with df_pre when that kernel does not run
    float pf_beta;     // < 0: the model's setting
    const float *lim_rows = nullptr, *beta_rows = nullptr;   // non-null: per-stream attenuation limit (linear) / post-filter beta [B] in place of the scalars
    float *out;        // [B, out_T, F][2]: local frame t of clip b is stored at frame t - out_toff
    int64_t out_T, out_toff;
    const struct DfxGate *gate = nullptr;  // per-stream stage gating (one new frame per pass); null: every frame runs every stage
    int channels = 1;                      // > 1: consecutive streams are the channels of one multi-channel stream ...
    int reduce_mask = 0;                   // ... whose ERB masks are reduced over the channels: 0 none, 1 max, 2 mean (tract.rs:96-118,868-902)
};

// ---- per-stream stage gating of the streaming runtime (DfTract::process / apply_stages, tract.rs:509-616,658-672) ----------------
// The reference decides per frame, from the encoder's local-SNR estimate, whether the ERB decoder (stage 1) and the DF decoder
// (stage 2) run at all; a decoder that does not run keeps its state (tract's pulsed models only advance when they are run), and a
// stream that has been silent for more than 5 hops is not processed at all.  Lockstep streams take those decisions independently:
// every kernel still runs for every stream (a skipped stream costs the same as a busy one on a GPU), and the decisions are applied
// as data: flags[b] selects whose state is kept (dfx_k_gate_commit) and what the deep-filter kernel is fed (dfx_k_gate_edit).
// DFX_GATE_PAUSED (pausable handles, dfx_stream_process_active): the stream sits this pass out.  It is always set together with
// DFX_GATE_FROZEN (dfx_k_stream_pause), so every kernel that gives a frozen stream its state back does the same for a paused one; the bit
// itself only tells dfx_k_gate_finish and the warm-up of a reset stream that no hop was consumed at all.
enum { DFX_GATE_FROZEN = 1, DFX_GATE_GAINS = 2, DFX_GATE_ZEROS = 4, DFX_GATE_DF = 8, DFX_GATE_PAUSED = 16 };
struct DfxGate {
    unsigned char *flags;  // [B]
    float thr[3];          // min_db_thresh, max_db_erb_thresh, max_db_df_thresh
    const float *thr_rows = nullptr;   // non-null: the same three per row [B][3] (per-stream thresholds: the rows of a stream hold the stream's entry)
    float *c0_win;         // [B, T, Fd, C]: slots T-kt .. T-2 = c0 of the last kt-1 frames the DF decoder ran on, T-1 = this frame
    void *pend2 = nullptr;           // fp16-split models: df_convp's pending sums instead, twice per stream (dfx_k_df_convp_step), with
    unsigned char *par = nullptr;    //   the half that is current and
    int *cnt = nullptr;              //   the frames each stream's DF decoder has consumed
    int channels;          // streams per multi-channel group: one skip counter and one stage decision (the first channel's lsnr) per group
};

// tract.rs:513-525: mean square of the hop (sequential f32 fold like the reference: the comparison with 1e-7 is then the same
// decision); below the threshold the counter goes up, else it is cleared; above 5 the stream is frozen for this hop.
// Multi-channel streams (ch consecutive rows): the fold runs over all channels of the hop, channel after channel, like the
// reference's `noisy.iter()` over its [ch, hop] array; every row of the group keeps an identical copy of the group's counter.
__global__ void dfx_k_gate_pre(const float *x, int64_t x_stride, int hop, int64_t B, int *skip_counter, unsigned char *flags, int ch) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t b0 = b - b % ch;
    float e = 0.f;
    for (int c = 0; c < ch; ++c) {
        const float *xp = x + (b0 + c) * x_stride;
        for (int i = 0; i < hop; ++i) e = __fadd_rn(e, __fmul_rn(xp[i], xp[i]));
    }
    const float ms = __fdiv_rn(e, (float)(hop * ch));
    int c = skip_counter[b];
    c = ms < 1e-7f ? c + 1 : 0;
    skip_counter[b] = c;
    flags[b] = c > 5 ? DFX_GATE_FROZEN : 0;
}

// The same for mono streams with the hop staged through LDS: 16 streams per 64-thread workgroup, rows loaded coalesced (a thread walking
// its own row touches 64 cache lines per load instruction: 50 us at 4096 streams, in front of everything else of a gated hop), then one
// lane per stream folds its row in the reference's order (rows padded by one float: the 16 lanes read different banks).
#define DFX_GATE_PRE_ROWS 16
__global__ void __launch_bounds__(64) dfx_k_gate_pre_lds(const float *x, int64_t x_stride, int hop, int64_t B, int *skip_counter, unsigned char *flags) {
    DFX_DYN_SMEM(float4, rows4);   // [16][hop / 4 + 1] float4: rows padded by one float4 (16 lanes x 16 bytes then read 64 different banks)
    const int64_t b0 = (int64_t)blockIdx.x * DFX_GATE_PRE_ROWS;
    const int q4 = hop >> 2, ld4 = q4 + 1;
    // all loads of eight rows are requested before the first LDS store (hop = 480: two float4 per thread and row)
    for (int r0 = 0; r0 < DFX_GATE_PRE_ROWS; r0 += 8) {
        for (int i0 = threadIdx.x; i0 < q4; i0 += 128) {
            float4 v[8][2];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int64_t b = b0 + r0 + r < B ? b0 + r0 + r : B - 1;
                const float4 *xr = reinterpret_cast<const float4 *>(x + b * x_stride);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int i = i0 + 64 * u;
                    v[r][u] = xr[i < q4 ? i : i0];
                }
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int i = i0 + 64 * u;
                    if (i < q4) rows4[(r0 + r) * ld4 + i] = v[r][u];
                }
        }
    }
    __syncthreads();
    const int64_t b = b0 + threadIdx.x;
    if (threadIdx.x >= DFX_GATE_PRE_ROWS || b >= B) return;
    const float4 *xp = rows4 + threadIdx.x * ld4;
    float e = 0.f;
    for (int i0 = 0; i0 < q4; i0 += 8) {   // eight LDS reads in flight, the fold itself in the reference's order
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = xp[i0 + u < q4 ? i0 + u : i0];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + u >= q4) break;
            e = __fadd_rn(e, __fmul_rn(v[u].x, v[u].x));
            e = __fadd_rn(e, __fmul_rn(v[u].y, v[u].y));
            e = __fadd_rn(e, __fmul_rn(v[u].z, v[u].z));
            e = __fadd_rn(e, __fmul_rn(v[u].w, v[u].w));
        }
    }
    const float ms = __fdiv_rn(e, (float)hop);
    int c = skip_counter[b];
    c = ms < 1e-7f ? c + 1 : 0;
    skip_counter[b] = c;
    flags[b] = c > 5 ? DFX_GATE_FROZEN : 0;
}
static int launch_gate_pre(const float *x, int64_t x_stride, int hop, int64_t B, int *skip_counter, unsigned char *flags, int ch, hipStream_t s) {
    const size_t smem = (size_t)DFX_GATE_PRE_ROWS * (hop / 4 + 1) * 16;
    if (ch == 1 && smem <= 64 * 1024 && hop % 4 == 0 && x_stride % 4 == 0 && !((uintptr_t)x & 15)) {
        dfx_launch(dfx_k_gate_pre_lds, dim3((unsigned)dfx_ceil_div(B, DFX_GATE_PRE_ROWS)), dim3(64), smem, s, x, x_stride, hop, B, skip_counter, flags);
    } else {
        dfx_launch(dfx_k_gate_pre, dim3((unsigned)dfx_ceil_div(B, 64)), dim3(64), 0, s, x, x_stride, hop, B, skip_counter, flags, ch);
    }
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}

// tract.rs:658-672 apply_stages on the newest frame's lsnr (lsnr[b*T + T-1])
// (multi-channel: the decision of a group is taken from its first channel's lsnr, tract.rs:468 `to_scalar`)
// thr_rows: per-stream thresholds [B][3] in place of the three scalars (a finite thr_df only: a mask-only model passes -inf and has no stage 2)
__global__ void dfx_k_gate_post(const float *lsnr, int64_t T, float thr_min, float thr_erb, float thr_df, unsigned char *flags,
                                int64_t B, int ch, const float *thr_rows) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    unsigned char f = flags[b];
    if (f & DFX_GATE_FROZEN) return;
    const float v = lsnr[(b - b % ch) * T + T - 1];
    if (thr_rows) {
        const float *tr = thr_rows + (b - b % ch) * 3;
        thr_min = tr[0], thr_erb = tr[1];
        if (thr_df != -INFINITY) thr_df = tr[2];
    }
    if (v < thr_min) f |= DFX_GATE_ZEROS;
    else if (v > thr_erb) f |= 0;
    else if (v > thr_df) f |= DFX_GATE_GAINS;
    else f |= DFX_GATE_GAINS | DFX_GATE_DF;
    flags[b] = f;
}

// The decisions as inputs of the (unchanged) deep-filter kernel, newest frame of every stream:
//   no stage 1: the band gains become 0 (zero mask, tract.rs:485-486) or 1 (gains absent: the spectrum passes, :565-567);
//   no stage 2: the low bins take the masked spectrum (:570-581) = a deep filter whose only non-zero tap is the current frame's,
//               with the band gain as a real coefficient (x*g - y*0 and 0-taps add exact zeros: the same bits as the mask path).
__global__ void dfx_k_gate_edit(const unsigned char *flags, float *mask, float *coefs, const unsigned char *bin2band, int64_t B,
                                int64_t T, int E, int Fd, int O, int tap0) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const unsigned char f = flags[b];
    float *mrow = mask + (b * T + T - 1) * E;
    if (!(f & DFX_GATE_GAINS)) {
        const float g = (f & DFX_GATE_ZEROS) ? 0.f : 1.f;
        for (int i = threadIdx.x; i < E; i += blockDim.x) mrow[i] = g;
    }
    __syncthreads();
    if (!(f & DFX_GATE_DF)) {
        for (int i = threadIdx.x; i < O * Fd; i += blockDim.x) {
            const int n = i / Fd, fq = i - n * Fd;
            float2 *cp = reinterpret_cast<float2 *>(coefs) + ((b * O + n) * T + T - 1) * Fd + fq;
            *cp = make_float2(n == tap0 ? mrow[bin2band[fq]] : 0.f, 0.f);
        }
    }
}

// Multi-channel streams: the ERB decoder's mask is reduced over the channels of a group and the reduced mask is applied to every
// channel (tract.rs:868-902: Reduce<Max> or Reduce<Sum> * (1/ch) wired behind the decoder; :547-556 the one mask for all channels).
// mask [B*T, E]; frames [t_begin, T) of every stream; mode 1 max, 2 mean.
__global__ void dfx_k_mask_reduce(float *mask, int64_t B, int64_t T, int64_t t_begin, int E, int ch, int mode) {
    const int64_t n = (B / ch) * (T - t_begin) * E;
    const float inv = 1.f / (float)ch;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const int64_t r = i / E, g = r / (T - t_begin), t = t_begin + r % (T - t_begin);
        float *p = mask + ((g * ch) * T + t) * E + e;
        float acc = p[0];
        for (int c = 1; c < ch; ++c) {
            const float v = p[(int64_t)c * T * E];
            acc = mode == 1 ? fmaxf(acc, v) : acc + v;
        }
        if (mode == 2) acc *= inv;
        for (int c = 0; c < ch; ++c) p[(int64_t)c * T * E] = acc;
    }
}

// The stage decisions as dfx_stream_process_raw reports them: DFX_GATE_GAINS and DFX_GATE_ZEROS both mean "gains exist".
__global__ void dfx_k_gate_stages(const unsigned char *flags, unsigned char *stages, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned char f = flags[b];
    stages[b] = (unsigned char)((f & DFX_GATE_DF) | ((f & (DFX_GATE_GAINS | DFX_GATE_ZEROS)) ? DFX_GATE_GAINS : 0));
}

// State selection after a gated pass: entry e copies row b of src to dst when (flags[b] & mask) == want.  Frozen streams get all
// their state back (STFT memories, running means, history rings, hidden states), a stream whose stage 1 / stage 2 was skipped its
// decoder's hidden states.
#define DFX_GATE_MAX_ENTRIES 24
struct DfxGateTable {
    float *dst[DFX_GATE_MAX_ENTRIES];
    const float *src[DFX_GATE_MAX_ENTRIES];
    int64_t row[DFX_GATE_MAX_ENTRIES];
    unsigned char mask[DFX_GATE_MAX_ENTRIES], want[DFX_GATE_MAX_ENTRIES];
    int n;
    void add(float *dst_, const float *src_, int64_t row_, unsigned char mask_, unsigned char want_) {   // host
        dst[n] = dst_, src[n] = src_, row[n] = row_, mask[n] = mask_, want[n] = want_;
        ++n;
    }
};
__global__ void dfx_k_gate_commit(DfxGateTable G, const unsigned char *flags, int64_t B) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const unsigned char f = flags[b];
    for (int e = 0; e < G.n; ++e) {
        if ((f & G.mask[e]) != G.want[e]) continue;
        const float *sp = G.src[e] + b * G.row[e];
        float *dp = G.dst[e] + b * G.row[e];
        for (int64_t i = threadIdx.x; i < G.row[e]; i += blockDim.x) dp[i] = sp[i];
    }
}

// Streams whose DF decoder ran push the newest c0 frame into their window (slot j <- slot j+1, j = T-kt .. T-2); the others keep
// theirs: the delay line in front of df_convp only moves when the DF decoder runs.
__global__ void dfx_k_gate_c0_shift(const unsigned char *flags, float *c0_win, int64_t B, int64_t T, int kt, int64_t frame) {
    const int64_t b = blockIdx.x;
    if (b >= B || !(flags[b] & DFX_GATE_DF)) return;
    float *w = c0_win + (b * T + T - kt) * frame;
    for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < frame; i += (int64_t)gridDim.y * blockDim.x)
        for (int j = 0; j + 1 < kt; ++j) w[j * frame + i] = w[(j + 1) * frame + i];
}

// Linear windows (dfx_stream_state::spec_lin, fe_lin, fs_lin) of gated handles: every stream's window slides by the hop, but a frozen stream's
// history must stay what it was.  After the hop's frame has been appended at frame pos + h, the frozen streams' h history frames
// [pos, pos + h) are moved up by one frame (the appended frame is overwritten): the next hop's history [pos + 1, pos + 1 + h) is then
// the old one.  One thread per element of a frame row, walking the frames from the newest down (an overlapping move within its column).
__global__ void dfx_k_gate_hold(const unsigned char *flags, float *win, int64_t cap, int64_t row, int64_t pos, int64_t h, int64_t B) {
    const int64_t b = blockIdx.x;
    if (b >= B || !(flags[b] & DFX_GATE_FROZEN)) return;
    float *w = win + (b * cap + pos) * row;
    for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < row; i += (int64_t)gridDim.y * blockDim.x)
        for (int64_t j = h - 1; j >= 0; --j) w[(j + 1) * row + i] = w[j * row + i];
}

// The same for the pending-sum form of df_convp (dfx_k_df_convp_step): where the DF decoder ran the sums written by this pass become
// current and the stream's frame count goes up.
__global__ void dfx_k_gate_pend_commit(const unsigned char *flags, unsigned char *par, int *cnt, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || !(flags[b] & DFX_GATE_DF)) return;
    par[b] ^= 1;
    cnt[b] += 1;
}

// End of a gated hop: frozen streams answer zeros and lsnr = -15 (tract.rs:522-525); the others update the skip counter from the
// stage decision (:562-567: gains present -> 0, absent -> += 1).  warm: the hop produced no net position yet (no decision taken).
// A paused stream (DFX_GATE_PAUSED, set with DFX_GATE_FROZEN) answers zeros too, but no estimate was made for it: its lsnr is NaN.
__global__ void dfx_k_gate_finish(const unsigned char *flags, int *skip_counter, float *y, int64_t y_stride, int hop, float *lsnr_out,
                                  int64_t lsnr_stride, int64_t B, int warm) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const unsigned char f = flags[b];
    if (f & DFX_GATE_FROZEN) {
        for (int i = threadIdx.x; i < hop; i += blockDim.x) y[b * y_stride + i] = 0.f;
        if (threadIdx.x == 0 && lsnr_out) lsnr_out[b * lsnr_stride] = (f & DFX_GATE_PAUSED) ? __int_as_float(0x7fc00000) : -15.f;
    } else if (threadIdx.x == 0 && !warm) {
        skip_counter[b] = (f & (DFX_GATE_GAINS | DFX_GATE_ZEROS)) ? 0 : skip_counter[b] + 1;
    }
}

enum { EV_START = 0, EV_C0, EV_C1, EV_C0P, EV_EMB, EV_COEFS, EV_FRONT, EV_DONE, EV_XA, EV_MASK, EV_FIN, EV_TICKET };

// What this model can run: decided once at the end of dfx_model_create (model_capabilities: the ONLY place these rules are written) from cfg,
// from what the optional packers packed and from the arithmetic mode.  A pass combines them with what depends on the pass (streaming window,
// B and T against the 32-bit limits, the sw test hooks, run_df, the lane, the ticket): DfxPass::plan() / DfxStreamPass::plan().
struct DfxCan {
    // df_conv0's output c0 is recomputed by its consumers instead of being stored when the pathway conv has the sliding-window kernel
    // (kt <= 5, df_order <= 8); otherwise c0 is materialised (dfx_k_conv_in_df -> dfx_k_pwconv / dfx_k_df_convp2 / dfx_k_df_convp).
    bool fuse_c0 = false;
    // Exact mode, batch passes: c0 is written once and read by its two consumers instead of being recomputed by both — on fp32 matrix ops a c0
    // tile is 20 ops of 32 cycles (3 of 16 on the fp16-split path), and the two recomputing kernels side by side are the exact front's 10 ms:
    // 28.65 vs 29.45 ms per step (the frame-by-frame runtime always uses the recomputing forms)
    bool c0_batch_unfused = false;
    bool c0_h3 = false;        // the fused c0 kernels on fp16-split fragments (dfx_k_df_conv01_h3, dfx_k_df_convp_h3, dfx_k_df_convp_step): fuse_c0, not exact, conv_ch % 32 == 0
    bool c0_presplit = false;  // batch passes of such a model read the pre-split copy of feat_spec (Ws::fps; DFX_C0_PRESPLIT=0: they do not)
    bool pw_h3 = false;        // the ERB blocks' pointwise contractions on fp16-split fragments (PwW::wt_h3 of the blocks that have them)
    // dfx_k_emb_fan (one pass over the encoder GRU's output for emb and its consumers) where the grouped linears nest the way pack_fan needs,
    // else the separate grouped GEMMs; fan_skp: df_skip is a grouped linear and one of the kernel's consumers (a pass: && run_df)
    bool fan = false, fan_skp = false;
    bool enc_fan = false;      // dfx_k_enc_fan: df_fc_emb + the encoder GRU's linear_in in one pass over c1 (pack_encfan's nesting, no enc_concat)
    bool dfenc = false;        // dfx_k_df_enc_h3: the DF branch of the encoder as one kernel, c1 never stored (else dfx_k_df_conv01_h3 + dfx_k_enc_fan)
    // frame-resident ERB encoder head (dfx_k_erb_enc: a frame's zero-bordered feature rows within the kernel's 192 staging lanes, two workgroups' rows
    // within the LDS; streaming has no other form of the head).  (The decoder end, dfx_k_erb_dec10: convt1 + conv0_out, fits every accepted shape: check_cfg.)
    bool fuse_enc = false;
    // The ERB decoder's convolutions as ONE launch (dfx_k_erb_tail: d3 / d2 / d1 stay in LDS, -12 KB per frame beside the GRU chain); otherwise
    // three launches (convt3, convt2, convt1 + conv0_out).  Measured at config 2 (profiles/r03_fusion_ab.log): the first version (8 waves per
    // CU) 2.19 ms alone against 1.5 ms for the three launches and +0.37 ms per step; the second (12 waves per CU, 8.5 KB of strips per wave,
    // fragments read from LDS per k-chunk) 1.32 ms alone and -0.25 ... -0.45 ms per step.
    // e0 = erb_conv0's output (8 KB per frame) is then not stored: the fused decoder tail recomputes it from the three feature rows it depends on
    // (rejected: written by dfx_k_erb_enc, read back by dfx_k_erb_tail)
    bool erb_tail = false;
    bool erb_enc4 = false;     // the four ERB encoder convolutions as one launch (dfx_k_erb_enc4; batch passes only)
    int df_out = DFX_PLAN_DF_OUT_GGEMM;   // df_out + tanh + c0p: DFX_PLAN_DF_OUT_RESIDENT / _STREAMING (dfx_k_df_out_h3r / _h3, a pass: while 32-bit offsets reach) or the grouped GEMM
};

// The flag block d_sync of the persistent GRU phase (dfx_k_gru_seq), word offsets.  All words are monotonic over the model's life or zeroed by
// their users; LG = one word per (layer, 16-clip group).
struct DfxSyncLayout {
    static constexpr size_t LG = (size_t)DFX_MAX_GRU_LAYERS * DFX_SEQ_GMAX;
    static constexpr size_t ready = 0;             // [8] per layer: gi chunks ready
    static constexpr size_t emb = 8;               // emb chunks ready
    static constexpr size_t probe = 13;            // the handshake's meeting counter (hwq_probe_run)
    static constexpr size_t poison = 14;           // "a kernel of this pass raised a fault", for the synthesis (dfx_k_fault_mirror)
    static constexpr size_t done = 16;             // [LG] chunks done per (layer, group)
    static constexpr size_t pcnt = done + LG;      // [16] producers' completion counters (DfxPublish), one per producing stream (layer), [8] = emb
    static constexpr size_t yprog = pcnt + 16;     // [LG] steps of y per (layer, group): the followers' hand-overs
    static constexpr size_t giprog = yprog + LG;   // [LG] steps of gi
    static constexpr size_t xtab = giprog + LG;    // [3 kinds][LG] XCD registrations (DfxXcd)
    static constexpr size_t xstat = xtab + 3 * LG; // [64]: [0] light hand-overs counted (dev aid), [8..48) the followers' claim counters
    static constexpr size_t total = xstat + 64;
};

struct dfx_model {
    dfx_model_cfg cfg{};
    float *d_w = nullptr;  // all prepared weights, one device allocation
    size_t n_w = 0;
    // offsets (floats) into d_w
    size_t erb0_w = 0, erb0_b = 0;
    PwW erb1, erb2, erb3, dfc0, dfc1, ct3, ct2, ct1;
    size_t co_w = 0, co_ska = 0, co_skb = 0;
    float co_bias = 0.f;
    size_t tail_w0h3 = 0, tail_woh3 = 0;    // dfx_k_erb_tail's fp16-split fragments of erb_conv0 (e0 recomputed, bias in a constant-1 slot) and of conv0_out
    float tail_w0_unscale = 1.f, tail_wo_unscale = 1.f;
    GlinW fc_emb, enc_in, enc_out, dec_in, dec_out, dfg_in, df_skip, df_out, enc_skip, dec_skip;
    std::vector<GruW> enc_gru, dec_gru, df_gru;
    size_t lsnr_w = 0;
    float lsnr_b = 0.f;
    // The fragment sets below are optional: a packer whose shape condition fails leaves its offsets alone, and whether a kernel that reads
    // them may run is `can`'s answer, never "is this offset non-zero".
    // dfx_k_emb_fan: fragments [chunks][8][64] float4, fan_chunks super-chunks of 32 hidden columns (can.fan)
    size_t fan_w = 0;
    int fan_chunks = 0;
    // dfx_k_enc_fan: fragments of df_fc_emb (efan_groups groups) and of the encoder GRU's linear_in (can.enc_fan)
    size_t efan_w1 = 0, efan_w2 = 0;
    int efan_groups = 0;
    // dfx_k_df_enc_h3 (df_conv0 -> df_conv1 -> df_fc_emb -> linear_in in one kernel): fc / linear_in fragments (can.dfenc)
    size_t dfenc_fc = 0, dfenc_in = 0;
    float dfenc_fc_unscale = 1.f, dfenc_in_unscale = 1.f;
    // dfx_k_df_out_h3 / _h3r (df_out + tanh + c0p as a row-streaming kernel of its own): fragments [G][ceil(Ng / 16)] (can.df_out)
    size_t dfo_h3 = 0;
    float dfo_unscale = 1.f;
    size_t cp_w1 = 0, cp_w2 = 0, cp_b = 0;   // df_convp, tiled form (kt > 5)
    size_t cp_weff = 0, cp_b16 = 0;          // df_convp, folded sliding-window form (kt <= 5)
    size_t cin_weff = 0, cin_b = 0;          // enc.df_conv0 folded into a dense 3x3 conv 2 -> C
    // fp16-split MFMA fragments of the fused DF-encoder kernels (can.c0_h3): df_conv0, df_conv1 pointwise, df_convp
    size_t c0_h3 = 0, dfc1_h3 = 0, cp_h3 = 0;
    float c0_unscale = 1.f, dfc1_unscale = 1.f, cp_unscale = 1.f;
    int cp_G = 0, cp_NO = 0;
    // concurrency (created once; one forward / enhance at a time per handle):
    //   a lane = the streams of one batch chunk: `main` (only used when dfx_enhance pipelines chunks; otherwise the caller's
    //   stream plays that role) + two auxiliary streams for the independent branches of the forward pass + fork/join events
    //   Round 6: the lanes belong to the PROCESS (one set per device, DfxLaneSet), not to the handle: every handle of a process enqueues on the
    //   same ~14 internal streams.  Handles used to bring 14 streams each, the second handle's streams shared hardware queues with the first
    //   one's (GPU_MAX_HW_QUEUES = 24) and its handshake put it on the event-synchronised form for good; passes of different handles take turns
    //   anyway (DfxTurn), so nothing is lost.
    DfxLane *lanes = nullptr;
    struct DfxLaneSet *laneset = nullptr;
    hipEvent_t ev_fork = nullptr;
    // One big pass in flight per handle: a call that would enqueue a multi-stream pass while the previous one is still running first
    // waits (on the host) for that one to drain.  Packets queued ahead on the pass's ~13 hardware queues slow the running pass — measured
    // at config 2: 19.45 ms per step with free enqueue-ahead, 18.8 ms when the host holds the next step back (DF-apply inside the loop
    // 0.60 -> 0.50 ms, the rate it has alone).  DFX_ENQUEUE_AHEAD=1 restores the unthrottled enqueue.
    hipEvent_t ev_pass = nullptr;
    hipEvent_t ev_gate = nullptr;       // recorded behind every multi-stream pass of this handle (DfxTurn)
    mutable bool pass_pending = false;
    bool enqueue_ahead = false;
    bool concurrent = false;
    int max_chunks = 1;       // batch chunks pipelined by dfx_enhance (dfx_model_set_pipeline; measured: no gain over time-chunk pipelining)
    int tchunks = 12;         // time chunks of the layer-pipelined GRU phase (DFX_TCHUNKS)
    int tchunk_min = 32;      // shortest chunk worth a launch (frames)
    bool run_df = true;       // DfNet(run_df=False): mask only (dfx_model_set_run_df)
    bool exact_fp32 = false;  // DFX_EXACT_FP32=1: keep the dense contractions on the exact fp32 MFMA path
    DfxCan can;               // which kernels this model's shape, fragments and arithmetic allow (model_capabilities)
    unsigned int *d_sync = nullptr;     // persistent GRU phase (dfx_k_gru_seq): its flag words (DfxSyncLayout)
    unsigned int *d_psync = nullptr;    // pair form of the persistent GRU phase: [DFX_MAX_GRU_LAYERS * DFX_SEQ_GMAX / 2][48] words
    mutable unsigned int seq_pbase = 0;       // step counter base of the follower hand-overs (yprog / giprog), monotonic like seq_base
    mutable int64_t passes_ps = 0;   // batch passes whose c0 kernels read the pre-split copy of feat_spec (DFX_Q_PASSES_C0_PRESPLIT)
    mutable int64_t passes_pair = 0; // passes whose persistent GRU phase ran on pairs of CUs (DFX_Q_PASSES_PAIR)
    mutable int64_t last_plan = 0;   // DFX_PLAN_* bits of the last pass (DFX_Q_LAST_PLAN): written by DfxPass::plan() / df_out_rows() / finish()
    mutable int64_t passes_seq = 0, passes_ev = 0;   // passes that ran the persistent phase / that gave it up because another process held the device's ticket (DFX_Q_TICKET_*)
    mutable unsigned int seq_base = 0;  // flag value of "nothing of the current forward pass yet"
    unsigned long long *d_trace = nullptr;   // dev aid (DFX_SEQ_TRACE=1): chunk timestamps of the last persistent GRU launch
    mutable int trace_dims[3] = {0, 0, 0};
    bool gru_seq = true;                // DFX_GRU_SEQ=0: one launch per (layer, time chunk) synchronised with events (round-1 form)
    // switches of the persistent GRU phase and its side work, read when the handle is created like the rest; -1 = "the default"
    struct {
        int chunks = 0;                 // DFX_SEQ_CHUNKS (0: 12)
        bool gru_pair_far = false;      // DFX_GRU_PAIR_FAR=1 (test hook): the pairs' hand-overs in their agent-scope form, as if the halves sat on different XCDs
        bool gru_pair = true;           // DFX_GRU_PAIR=0: every 16-clip group's recurrence on one CU (W_hh streamed from the L2) instead of 32 clips on a pair of CUs (dfx_gru_pair.h)
        int convp_late = -1;            // DFX_CONVP_LATE (percent)
        int p0_ahead = 3;               // DFX_SEQ_P0_AHEAD
        int tail_every = 1;             // DFX_SEQ_TAIL_EVERY
        int dftail_every = 0;           // DFX_SEQ_DFTAIL_EVERY (0: the rule in forward_impl)
        bool tail_split = true;         // the ERB decoder's linear_out on a stream of its own beside the decoder tail (round 6; DFX_TAIL_SPLIT=0 in -DDFX_DEV builds)
        int64_t convp_elems = (int64_t)1 << 29;   // DFX_CONVP_ELEMS (test hook)
        bool c0_presplit = true;        // DFX_C0_PRESPLIT=0 (test hook): batch passes run the unsplit instances of dfx_k_df_enc_h3 / dfx_k_df_convp_h3 on the fp32 feat_spec
        bool seq_trace = false;         // DFX_SEQ_TRACE=1 (dev aid): d_trace below
        char hwq_probe_mode = 0;        // DFX_HWQ_PROBE: '0' no handshake, 'f' ("fail") a failed one, 0 the handshake before the first pass that needs it
        bool erb_enc_split = false;     // DFX_ERB_ENC_SPLIT=1 (test hook): batch passes run the ERB encoder as three launches (dfx_k_erb_enc, dfx_k_pwconv_f x 2) instead of dfx_k_erb_enc4
        int ws_fill = -1;               // DFX_WS_FILL=0..255 (test hook): every pass starts by setting the bytes of its workspace layout to this value (dfx_ws_fill); -1: no fill
    } sw;
    // Error words, written by kernels, read by the host (page-locked host memory the device can store to: dfx_env_err_words_alloc):
    // [0] unused, [1] fp16-split range, [2] a flag wait of the persistent GRU phase timed out.
    // The host looks at them wherever it waits for the device anyway (pass_begin, dfx_model_check) and at the start of every call
    // (model_poll: plain loads, no synchronisation), so a fault is reported by the NEXT call on the handle at the latest;
    // DFX_CHECK_EVERY_PASS=1 makes every call wait for its own pass and report its own faults.
    unsigned int *d_err = nullptr;      // device address
    unsigned int *h_err = nullptr;      // host address of the same words
    bool check_every_pass = false;
    int spin_limit = DFX_SYNC_SPIN_LIMIT;   // DFX_SYNC_SPIN_LIMIT=n (tests: force the timeouts)
    bool hwq_probe_pending = false;     // the handshake of the persistent phase's streams has not run yet (hwq_probe_run)
    int hwq_probe = -1;                 // -1 not run, 1: the phase's streams run concurrently, 0: they do not (event-based GRU phase instead)
    const float *p(size_t off) const { return d_w + off; }
};

namespace {
struct Prep {
    const float *blob;
    const DfxManifest &man;
    std::vector<float> out;
    std::string err;
    bool exact_fp32 = false;   // the model is created under DFX_EXACT_FP32=1: weights that only the exact kernels read are packed
    struct Packed {            // which optional fragment sets the packers made (each states its shape condition at its head); model_capabilities reads it
        bool pw = false, tail = false, c0 = false, fan = false, fan_skp = false, encfan = false, dfenc = false;
        int dfo_tiles = 0;     // 16-column tiles per group of df_out's fragments (0: not packed)
    } packed;
    const float *get(const std::string &name, const DfxTensor **tt = nullptr) {
        const DfxTensor *t = man.find(name);
        if (!t) {
            err = "tensor not in manifest: " + name;
            return nullptr;
        }
        if (tt) *tt = t;
        return blob + t->offset;
    }
    size_t alloc(size_t n) {  // 16-byte aligned carve
        size_t off = (out.size() + 3) & ~(size_t)3;
        out.resize(off + n, 0.f);
        return off;
    }
    // BatchNorm2d eval: y = x*scale + shift
    bool bn(const std::string &p, int n, std::vector<float> &scale, std::vector<float> &shift) {
        const float *g = get(p + ".weight"), *b = get(p + ".bias"), *m = get(p + ".running_mean"), *v = get(p + ".running_var");
        if (!g || !b || !m || !v) return false;
        scale.resize(n);
        shift.resize(n);
        for (int i = 0; i < n; ++i) {
            const float s = g[i] / sqrtf(v[i] + 1e-5f);
            scale[i] = s;
            shift[i] = b[i] - m[i] * s;
        }
        return true;
    }
};

// depthwise [C,1,1,3] (+transposed [C,1,1,3]) + pointwise [C,C,1,1] + BN at Sequential indices .0/.1/.2
bool prep_sep(Prep &P, const std::string &name, int C, PwW &w) {
    const float *dw = P.get(name + ".0.weight"), *pw = P.get(name + ".1.weight");
    std::vector<float> sc, sh;
    if (!dw || !pw || !P.bn(name + ".2", C, sc, sh)) return false;
    w.dw = P.alloc(3 * C);
    w.wt = P.alloc((size_t)C * C);
    w.bias = P.alloc(C);
    for (int c = 0; c < C; ++c)
        for (int j = 0; j < 3; ++j) P.out[w.dw + j * C + c] = dw[c * 3 + j];
    for (int n = 0; n < C; ++n)
        for (int k = 0; k < C; ++k) P.out[w.wt + (size_t)k * C + n] = pw[(size_t)n * C + k] * sc[n];
    for (int n = 0; n < C; ++n) P.out[w.bias + n] = sh[n];
    return true;
}
// pathway conv{N}p: Conv2d(C,C,1,groups=C) [C,1,1,1] + BN at .0/.1  ->  y = relu(a*x + b)
bool prep_path(Prep &P, const std::string &name, int C, size_t &a_off, size_t &b_off) {
    const float *w = P.get(name + ".0.weight");
    std::vector<float> sc, sh;
    if (!w || !P.bn(name + ".1", C, sc, sh)) return false;
    a_off = P.alloc(C);
    b_off = P.alloc(C);
    for (int c = 0; c < C; ++c) {
        P.out[a_off + c] = w[c] * sc[c];
        P.out[b_off + c] = sh[c];
    }
    return true;
}
// fp16-split MFMA A fragments: nfrag fragments of [hi, lo][64 lanes][8 halves]; val(frag, lane, i) is the fp32 weight of that slot.
// All values are scaled by one power of two so that the largest is just below 2^14 (lo parts stay normal f16); *unscale undoes it.
// val may read P.out: the values are taken first, the fragments carved afterwards (alloc may move P.out).
template <typename F>
size_t pack_h3(Prep &P, int nfrag, F val, float *unscale) {
    std::vector<float> v((size_t)nfrag * 64 * 8);
    float mx = 0.f;
    for (int fr = 0; fr < nfrag; ++fr)
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 8; ++i) {
                const float w = val(fr, l, i);
                v[((size_t)fr * 64 + l) * 8 + i] = w;
                mx = fmaxf(mx, fabsf(w));
            }
    int e = 0;
    if (mx > 0.f) {
        int ex;
        frexpf(mx, &ex);          // mx = f * 2^ex, f in [0.5, 1)
        e = 14 - ex;              // scaled magnitude < 2^14
        if (e > 24) e = 24;
        if (e < -14) e = -14;
    }
    const float sc = ldexpf(1.f, e);
    *unscale = ldexpf(1.f, -e);
    const size_t off = P.alloc((size_t)nfrag * 2 * 64 * 8 / 2);
    uint16_t *dst = reinterpret_cast<uint16_t *>(&P.out[off]);
    for (int fr = 0; fr < nfrag; ++fr)
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 8; ++i) {
                const float w = v[((size_t)fr * 64 + l) * 8 + i] * sc;
                const uint16_t hb = dfx_f32_to_f16_bits(w);
                const uint16_t lb = dfx_f32_to_f16_bits(w - dfx_f16_bits_to_f32(hb));
                dst[(((size_t)fr * 2 + 0) * 64 + l) * 8 + i] = hb;
                dst[(((size_t)fr * 2 + 1) * 64 + l) * 8 + i] = lb;
            }
    return off;
}
// The fp32 twin for the GRU weights w [3 H][H] (H = 256), in dfx_k_gru_rec_h3's fragment order: [16-unit tile][k-chunk][gate][half][lane][4],
// half h = weights 32 kc + 8 q + 4 h + 0..3 of the lane's unit
size_t pack_x32(Prep &P, const float *w) {
    const int H = 256;
    const size_t off = P.alloc((size_t)3 * H * H);
    float *dst = &P.out[off];
    for (int ut = 0; ut < 16; ++ut)
        for (int kc = 0; kc < 8; ++kc)
            for (int gate = 0; gate < 3; ++gate)
                for (int half = 0; half < 2; ++half)
                    for (int l = 0; l < 64; ++l)
                        for (int i = 0; i < 4; ++i) {
                            const int unit = 16 * ut + (l & 15), k = 32 * kc + 8 * (l >> 4) + 4 * half + i;
                            const size_t frag = (((size_t)ut * 8 + kc) * 3 + gate) * 2 + half;
                            dst[(frag * 64 + l) * 4 + i] = w[(size_t)(gate * H + unit) * H + k];
                        }
    return off;
}
// pointwise weights of a separable block as dfx_chain_stage_h3's A fragments: fragment (nt, kc), lane l, element i = the weight of output
// channel 16 nt + (l & 15) for input channel (C/4) (l >> 4) + 8 kc + i (lane (pos, q) owns the C/4 consecutive channels from (C/4) q)
void pack_pw_h3(Prep &P, dfx_model *m) {   // the six ERB blocks (df_conv1 has its own order: dfc1_h3)
    const int C = m->cfg.conv_ch, KC = C / 32;
    if (C % 32 != 0) return;
    for (PwW *w : {&m->erb1, &m->erb2, &m->erb3, &m->ct3, &m->ct2, &m->ct1}) {
        w->wt_h3 = pack_h3(P, (C / 16) * KC, [&](int fr, int l, int i) {
            const int nt = fr / KC, kc = fr % KC;
            return P.out[w->wt + (size_t)((C / 4) * (l >> 4) + 8 * kc + i) * C + 16 * nt + (l & 15)];
        }, &w->unscale);
        w->has_h3 = true;
    }
    P.packed.pw = true;
}
bool prep_glin(Prep &P, const std::string &name, GlinW &g) {
    const DfxTensor *t = nullptr;
    const float *w = P.get(name, &t);
    if (!w) return false;
    g.G = (int)t->shape[0];
    g.Kg = (int)t->shape[1];
    g.Ng = (int)t->shape[2];
    g.w = P.alloc((size_t)t->numel());
    memcpy(&P.out[g.w], w, sizeof(float) * (size_t)t->numel());
    return true;
}
// Fragments of dfx_k_emb_fan.  Needs the nesting of DeepFilterNet3's released shape: linear_out of the encoder GRU in groups of
// 16 -> 32 (lin_groups = 16 over 256 -> 512), erb_dec's linear_in and df_skip in groups of 32 -> 16 ("narrow": lin_groups = 16 over
// 512 -> 256), df_gru's linear_in in groups of 64 -> 32 ("wide": SqueezedGRU_S's default of 8 groups, deepfilternet3.py:296-302), so that
// y[:, 32J:32J+32] -> emb[:, 64J:64J+64] -> out[:, 32J:32J+32] is closed for every super-chunk J.  Other shapes: fan_nj stays 0.
//   fragment (J, i), lane l = (m = l & 15, kq = l >> 4), component s:
//     i = 2 ch + t            stage 1, chunk ch of the super-chunk, output features 16 t + m of it: W_out[2J + ch][4 kq + s][16 t + m]
//     i = 4 + 8 c + 2 u + t   narrow consumer c, output column 16 u + m: W_c[2J + u][16 t + 4 kq + s][m]
//     i = 4 + 8 c + 4 u + tt  wide consumer c, output column 16 u + m:   W_c[J][16 tt + 4 kq + s][16 u + m]
void pack_fan(Prep &P, dfx_model *m) {
    int kind[DFX_FAN_NC];   // per consumer (dec_in, dfg_in, df_skip): 0 absent, 1 narrow (32 -> 16 groups), 2 wide (64 -> 32 groups)
    const GlinW &o = m->enc_out;
    const GlinW *cons[DFX_FAN_NC] = {&m->dec_in, &m->dfg_in, m->cfg.df_gru_skip == DFX_SKIP_GROUPEDLINEAR ? &m->df_skip : nullptr};
    if (o.Kg != 16 || o.Ng != 32 || o.G % 2 != 0) return;
    const int nj = o.G / 2;
    for (int c = 0; c < DFX_FAN_NC; ++c) {
        const GlinW *g = cons[c];
        kind[c] = 0;
        if (!g) continue;
        if (g->G == 2 * nj && g->Kg == 32 && g->Ng == 16) kind[c] = 1;
        else if (g->G == nj && g->Kg == 64 && g->Ng == 32) kind[c] = 2;
        else return;
    }
    // the instantiated combinations (launch_emb_fan)
    if (kind[0] != 1 || kind[1] != 2 || (kind[2] != 1 && kind[2] != 0)) return;
    const size_t off = P.alloc((size_t)nj * DFX_FAN_WPJ * 64 * 4);   // (may reallocate P.out: offsets only below)
    auto frag = [&](int J, int i, int l, int sidx) -> float & { return P.out[off + (((size_t)J * DFX_FAN_WPJ + i) * 64 + l) * 4 + sidx]; };
    for (int J = 0; J < nj; ++J)
        for (int l = 0; l < 64; ++l) {
            const int mm = l & 15, kq = l >> 4;
            for (int sidx = 0; sidx < 4; ++sidx) {
                for (int ch = 0; ch < 2; ++ch)
                    for (int t = 0; t < 2; ++t) frag(J, 2 * ch + t, l, sidx) = P.out[o.w + ((size_t)(2 * J + ch) * 16 + 4 * kq + sidx) * 32 + 16 * t + mm];
                for (int c = 0; c < DFX_FAN_NC; ++c) {
                    if (kind[c] == 1) {
                        for (int u = 0; u < 2; ++u)
                            for (int t = 0; t < 2; ++t)
                                frag(J, 4 + 8 * c + 2 * u + t, l, sidx) = P.out[cons[c]->w + ((size_t)(2 * J + u) * 32 + 16 * t + 4 * kq + sidx) * 16 + mm];
                    } else if (kind[c] == 2) {
                        for (int u = 0; u < 2; ++u)
                            for (int tt = 0; tt < 4; ++tt)
                                frag(J, 4 + 8 * c + 4 * u + tt, l, sidx) = P.out[cons[c]->w + ((size_t)J * 64 + 16 * tt + 4 * kq + sidx) * 32 + 16 * u + mm];
                    }
                }
            }
        }
    m->fan_w = off;
    m->fan_chunks = nj;
    P.packed.fan = true, P.packed.fan_skp = kind[2] == 1;
}
// Fragments of dfx_k_enc_fan: df_fc_emb in groups of 96 -> 16 (enc_lin_groups = 32 over 3072 -> 512) feeding linear_in of the encoder GRU in
// groups of 32 -> 16 (lin_groups = 16 over 512 -> 256), i.e. two groups of the first per group of the second.
//   w1 (g, i), lane (m, kq), component s: W_fc[g][16 i + 4 kq + s][m];   w2 (h, t), component r: W_in[h][16 t + 4 kq + r][m]
void pack_encfan(Prep &P, dfx_model *m) {
    const GlinW &a = m->fc_emb, &b = m->enc_in;
    if (a.Kg != 96 || a.Ng != 16 || a.G % 2 != 0 || b.G * 2 != a.G || b.Kg != 32 || b.Ng != 16) return;
    const size_t o1 = P.alloc((size_t)a.G * 6 * 64 * 4);
    const size_t o2 = P.alloc((size_t)b.G * 2 * 64 * 4);
    for (int l = 0; l < 64; ++l) {
        const int mm = l & 15, kq = l >> 4;
        for (int sidx = 0; sidx < 4; ++sidx) {
            for (int g = 0; g < a.G; ++g)
                for (int i = 0; i < 6; ++i) P.out[o1 + (((size_t)g * 6 + i) * 64 + l) * 4 + sidx] = P.out[a.w + ((size_t)g * 96 + 16 * i + 4 * kq + sidx) * 16 + mm];
            for (int h = 0; h < b.G; ++h)
                for (int t = 0; t < 2; ++t) P.out[o2 + (((size_t)h * 2 + t) * 64 + l) * 4 + sidx] = P.out[b.w + ((size_t)h * 32 + 16 * t + 4 * kq + sidx) * 16 + mm];
        }
    }
    m->efan_w1 = o1, m->efan_w2 = o2;
    m->efan_groups = a.G;
    P.packed.encfan = true;
}
bool prep_gru(Prep &P, const std::string &name, int layers, std::vector<GruW> &out) {
    const int H = 256;
    for (int l = 0; l < layers; ++l) {
        const std::string s = std::to_string(l);
        const float *wih = P.get(name + ".weight_ih_l" + s), *whh = P.get(name + ".weight_hh_l" + s);
        const float *bih = P.get(name + ".bias_ih_l" + s), *bhh = P.get(name + ".bias_hh_l" + s);
        if (!wih || !whh || !bih || !bhh) return false;
        GruW g;
        g.wih_t = P.alloc((size_t)H * 3 * H);
        g.bias_i = P.alloc(3 * H);
        g.whh4 = P.alloc((size_t)H * 3 * H);
        g.bhn = P.alloc(H);
        for (int n = 0; n < 3 * H; ++n)
            for (int k = 0; k < H; ++k) P.out[g.wih_t + (size_t)k * 3 * H + n] = wih[(size_t)n * H + k];
        // r and z gates: both biases can be summed up front; the n gate keeps b_hn inside r*(...)
        for (int n = 0; n < 3 * H; ++n) P.out[g.bias_i + n] = bih[n] + (n < 2 * H ? bhh[n] : 0.f);
        for (int k4 = 0; k4 < H / 4; ++k4)
            for (int gate = 0; gate < 3; ++gate)
                for (int j = 0; j < H; ++j)
                    for (int e = 0; e < 4; ++e)
                        P.out[g.whh4 + ((((size_t)k4 * 3 + gate) * H + j) * 4 + e)] = whh[(size_t)(gate * H + j) * H + 4 * k4 + e];
        for (int j = 0; j < H; ++j) P.out[g.bhn + j] = bhh[2 * H + j];
        // fp16-split fragments [n/64][kc][ct] of W[k][n] = w[n][k] (dfx_k_proj256_h3; W_hh in the same order: dfx_k_gru_step_h3) ...
        auto proj_order = [&](const float *w) {
            return [w](int fr, int l, int i) {
                const int ch = fr / 32, kc = fr / 4 % 8, ct = fr % 4;
                return w[(size_t)(ch * 64 + ct * 16 + (l & 15)) * H + 32 * kc + 8 * (l >> 4) + i];
            };
        };
        // ... and [16-unit tile][k-chunk][gate] of W_hh (dfx_k_gru_rec_h3); both forms of W_hh carry the one scale that max |W_hh| gives
        auto rec_order = [whh](int fr, int l, int i) {
            const int ut = fr / 24, kc = fr / 3 % 8, gate = fr % 3;
            return whh[(size_t)(gate * H + 16 * ut + (l & 15)) * H + 32 * kc + 8 * (l >> 4) + i];
        };
        g.wih_h3 = pack_h3(P, 3 * H / 64 * 8 * 4, proj_order(wih), &g.wih_unscale);
        g.whh_pj = pack_h3(P, 3 * H / 64 * 8 * 4, proj_order(whh), &g.whh_unscale);
        g.whh_h3 = pack_h3(P, 16 * 8 * 3, rec_order, &g.whh_unscale);
        g.whh_x32 = pack_x32(P, whh);
        if (P.exact_fp32) g.wih_x32 = pack_x32(P, wih), g.has_wih_x32 = true;   // (fp16-split models do not carry it)
        out.push_back(g);
    }
    return true;
}
}  // namespace

static std::mutex &dfx_laneset_mu() {
    static std::mutex mu;
    return mu;
}
static DfxLaneSet *dfx_laneset_of_device() {   // (never freed: streams of a process live as long as it does)
    static std::map<int, DfxLaneSet *> sets;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(dfx_laneset_mu());
    DfxLaneSet *&ls = sets[dev];
    if (!ls) ls = new DfxLaneSet();
    return ls;
}
// The persistent GRU phase across PROCESSES.  Its ~160 workgroups must all be resident (each owns a CU); two such passes of two processes on one
// GPU can each hold the CUs the other's missing workgroups wait for, and both end in flag-wait timeouts (a fault the host is told about, but two
// seconds late and with both passes lost).  Inside a process the passes take turns (DfxTurn); between processes there is a ticket per device: an
// advisory lock on /dev/shm/dfx_persistent_<PCI bus id>.lock, taken without waiting in front of a persistent phase and given back by a host callback
// behind the pass (on a side stream: the caller's stream does not wait for the callback).  A pass that does not get the ticket runs the
// event-synchronised form of the phase (no residency requirement; ~1.4 x slower), so nobody ever waits for another process.  DFX_DEVICE_TICKET=0:
// off (one process per GPU is guaranteed by the deployment); processes that do not share /dev/shm do not see each other.
struct DfxTicket {
    int fd = -2;                    // -2 not opened yet, -1 unavailable
    std::atomic<int> holds{0};      // passes of this process that hold it
};
static DfxTicket &dfx_ticket() {
    static DfxTicket t;
    return t;
}
static bool dfx_ticket_try() {   // (under the enqueue lock)
    DfxTicket &t = dfx_ticket();
    if (t.fd == -2) {
        const char *e = getenv("DFX_DEVICE_TICKET");
        t.fd = -1;
        if (!(e && e[0] == '0')) {
            int dev = 0;
            char bus[64] = "gpu";
            if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), dev);
            for (char *c = bus; *c; ++c)
                if (*c == ':' || *c == '.' || *c == '/') *c = '_';
            char path[160];
            snprintf(path, sizeof(path), "/dev/shm/dfx_persistent_%s.lock", bus);
            t.fd = open(path, O_RDWR | O_CREAT | O_CLOEXEC, 0666);
            if (t.fd >= 0) (void)fchmod(t.fd, 0666);
        }
    }
    if (t.fd < 0) return true;                      // no ticket office: as before
    if (t.holds.load() > 0) {                       // this process already holds it (an earlier pass still in flight)
        t.holds.fetch_add(1);
        return true;
    }
    if (flock(t.fd, LOCK_EX | LOCK_NB) != 0) return false;
    t.holds.fetch_add(1);
    return true;
}
static void dfx_ticket_release_cb(void *) {
    DfxTicket &t = dfx_ticket();
    if (t.fd >= 0 && t.holds.fetch_sub(1) == 1) (void)flock(t.fd, LOCK_UN);
}
// One enqueue at a time per process: every entry point that puts work on the process's internal streams holds this lock while it does
// (forward, enhance, the streaming calls); see DfxTurn.
static std::mutex &dfx_enqueue_mu() {
    static std::mutex mu;
    return mu;
}
static bool dfx_create_lane(dfx_model *m, int l) {
    if (!m->laneset) {
        m->laneset = dfx_laneset_of_device();
        if (!m->laneset) return false;
        m->lanes = m->laneset->lanes;
    }
    // idempotent: whatever of the lane does not exist yet is created (a second handle finds the first one's streams; a deeper model adds its layers')
    std::lock_guard<std::mutex> lk(dfx_laneset_mu());
    DfxLane &ln = m->lanes[l];
    bool good = true;
    auto stream = [&](hipStream_t &st) {
        if (!st) good = good && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    };
    auto event = [&](hipEvent_t &e) {
        if (!e) good = good && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    };
    stream(ln.main);
    for (int i = 0; i < 2; ++i) stream(ln.aux[i]);
    for (int i = 0; i < DFX_LANE_EVENTS; ++i) event(ln.ev[i]);
    if (l == 0) {  // the layer-pipelined GRU phase runs on lane 0 only
        const int nl_model = 1 + (m->cfg.emb_num_layers - 1) + m->cfg.df_num_layers;
        const int nl = nl_model > 5 ? nl_model : 5;   // (at least the five layers of the shipped shapes: the handshake then covers what later handles use)
        for (int i = 0; i < nl && i < DFX_MAX_GRU_LAYERS; ++i) {
            if (i > 0) stream(ln.gs[i]);  // layer 0 recurs on the caller's stream
            stream(ln.ps[i]);             // (highest priority for these was measured: the spinning wait kernels then starve every other queue, seconds per step)
            for (int k = 0; k < DFX_MAX_TCHUNKS; ++k) event(ln.gev[i][k]), event(ln.pev[i][k]);
        }
        for (int i = 0; i < 2; ++i) stream(ln.ts[i]);
        for (int k = 0; k < DFX_MAX_TCHUNKS; ++k) event(ln.eev[k]);
    }
    return good;
}

// The persistent GRU phase synchronises through device flags: the stream of the persistent launch, the preparation stream of
// every layer and the two decoder-tail streams must make progress independently.  Streams that share a hardware queue
// (GPU_MAX_HW_QUEUES left at ROCm's default of 4, or set after HIP had initialised) would put a spinning wait in front of the
// launch it waits for — a timeout and an invalid pass.  Checked once per handle with a handshake between exactly those streams, the
// first time it matters (hwq_probe_pending).
static void hwq_probe_fallback(dfx_model *m) {   // the event-synchronised form (DFX_GRU_SEQ=0) needs no concurrency to be correct
    m->gru_seq = false;
    if (!(getenv("DFX_QUIET") && getenv("DFX_QUIET")[0] == '1'))
        fprintf(stderr, "dfx: the streams of the persistent GRU phase do not run concurrently (GPU_MAX_HW_QUEUES >= 16 must be in the environment "
                        "before HIP initialises): this model uses the slower event-synchronised GRU phase (dfx_model_query DFX_Q_HWQ_PROBE = 0)\n");
}
// (the caller holds the enqueue lock, DfxTurn: the handshake synchronises the process's internal streams, so whatever another handle has in flight
// on them is over before it starts; its result belongs to the lane set — one handshake per process and device)
static void hwq_probe_run(dfx_model *m) {
    if (!m->hwq_probe_pending) return;
    m->hwq_probe_pending = false;
    DfxLaneSet *ls = m->laneset;
    if (ls && ls->hwq_probe >= 0) {
        m->hwq_probe = ls->hwq_probe;
        if (m->hwq_probe == 0) hwq_probe_fallback(m);
        return;
    }
    const DfxLane &ln = m->lanes[0];
    std::vector<hipStream_t> ss;
    if (ln.gs[1]) ss.push_back(ln.gs[1]);
    for (int i = 0; i < DFX_MAX_GRU_LAYERS; ++i)
        if (ln.ps[i]) ss.push_back(ln.ps[i]);
    for (int i = 0; i < 2; ++i)
        if (ln.ts[i]) ss.push_back(ln.ts[i]);
    unsigned int *cnt = m->d_sync + DfxSyncLayout::probe;
    // warm-up: the kernel's code object is loaded and every stream's queue exists before the bounded handshake starts (a slow first
    // launch must not look like a shared queue); a failed handshake is tried once more with a longer bound before it counts
    for (hipStream_t st : ss) dfx_launch(dfx_k_probe_meet, dim3(1), dim3(64), 0, st, cnt, 0u, 1, m->d_err + 9);
    bool okp = hipGetLastError() == hipSuccess;
    for (hipStream_t st : ss) okp = hipStreamSynchronize(st) == hipSuccess && okp;
    m->hwq_probe = 0;
    for (int attempt = 0; attempt < 2 && okp && m->hwq_probe == 0; ++attempt) {
        (void)hipMemset(cnt, 0, sizeof(unsigned int));
        m->h_err[8] = 0u;
        for (hipStream_t st : ss) dfx_launch(dfx_k_probe_meet, dim3(1), dim3(64), 0, st, cnt, (unsigned int)ss.size(), 1 << (16 + 3 * attempt), m->d_err + 8);
        okp = hipGetLastError() == hipSuccess;
        for (hipStream_t st : ss) okp = hipStreamSynchronize(st) == hipSuccess && okp;
        m->hwq_probe = okp && ((volatile unsigned int *)m->h_err)[8] == 0u ? 1 : 0;
    }
    m->h_err[8] = 0u, m->h_err[9] = 0u;
    (void)hipMemset(cnt, 0, sizeof(unsigned int));
    if (ls) ls->hwq_probe = m->hwq_probe;
    if (m->hwq_probe == 0) hwq_probe_fallback(m);
}

// ------------------------------------------------------------------------------------------------ model creation
// Weight preparation: BatchNorm folded into the layer in front of it, every array re-laid-out the way its kernel reads it, carved from P.out
// in the order of the steps below (prepare_weights).  A step returns false where a tensor is missing (P.err names it).
namespace {
// enc.erb_conv0: pad(.0) conv(.1) bn(.2)
bool prep_erb_conv0(Prep &P, dfx_model *m) {
    const int C = m->cfg.conv_ch;
    const float *w = P.get("enc.erb_conv0.1.weight");
    std::vector<float> sc, sh;
    if (!w || !P.bn("enc.erb_conv0.2", C, sc, sh)) return false;
    m->erb0_w = P.alloc(9 * C);
    m->erb0_b = P.alloc(C);
    for (int ch = 0; ch < C; ++ch) {
        for (int k = 0; k < 9; ++k) P.out[m->erb0_w + k * C + ch] = w[ch * 9 + k] * sc[ch];
        P.out[m->erb0_b + ch] = sh[ch];
    }
    return true;
}
// enc.df_conv0: pad(.0) conv groups=2 (.1) pointwise(.2) bn(.3), folded into one dense conv (K = 18 -> 20)
bool prep_df_conv0(Prep &P, dfx_model *m) {
    const int C = m->cfg.conv_ch;
    const float *w = P.get("enc.df_conv0.1.weight"), *pw = P.get("enc.df_conv0.2.weight");
    std::vector<float> sc, sh;
    if (!w || !pw || !P.bn("enc.df_conv0.3", C, sc, sh)) return false;
    m->cin_weff = P.alloc((size_t)20 * C);
    m->cin_b = P.alloc(C);
    for (int n = 0; n < C; ++n) {
        for (int tap = 0; tap < 9; ++tap)
            for (int ch = 0; ch < 2; ++ch) {
                double acc = 0.0;  // groups=2: output channel c of the 3x3 conv sees input ch = c / (C/2)
                for (int c = ch * (C / 2); c < (ch + 1) * (C / 2); ++c) acc += (double)pw[(size_t)n * C + c] * (double)w[c * 9 + tap];
                P.out[m->cin_weff + (size_t)(tap * 2 + ch) * C + n] = (float)(acc * (double)sc[n]);
            }
        P.out[m->cin_b + n] = sh[n];
    }
    return true;
}
bool prep_lsnr(Prep &P, dfx_model *m) {
    const float *w = P.get("enc.lsnr_fc.0.weight"), *b = P.get("enc.lsnr_fc.0.bias");
    if (!w || !b) return false;
    const int emb = m->cfg.conv_ch * m->cfg.nb_erb / 4;
    m->lsnr_w = P.alloc(emb);
    memcpy(&P.out[m->lsnr_w], w, sizeof(float) * emb);
    m->lsnr_b = b[0];
    return true;
}
// erb_dec.conv0_out: conv [1,C,1,3] (.0) bn(1) (.1)
bool prep_conv0_out(Prep &P, dfx_model *m) {
    const int C = m->cfg.conv_ch;
    const float *w = P.get("erb_dec.conv0_out.0.weight");
    std::vector<float> sc, sh;
    if (!w || !P.bn("erb_dec.conv0_out.1", 1, sc, sh)) return false;
    m->co_w = P.alloc(3 * C);
    for (int ch = 0; ch < C; ++ch)
        for (int j = 0; j < 3; ++j) P.out[m->co_w + j * C + ch] = w[ch * 3 + j] * sc[0];
    m->co_bias = sh[0];
    return true;
}
// matrix-op forms of the two small contractions inside dfx_k_erb_tail (round 5)
void pack_tail_h3(Prep &P, dfx_model *m) {
    const int C = m->cfg.conv_ch;
    if (C % 32 != 0) return;
    const int KC = C / 32;
    const size_t w0 = m->erb0_w, b0 = m->erb0_b, wo = m->co_w;
    // erb_conv0 as [C x 32] fragments per 16 channels: k-slot 8 (l >> 4) + i = tap 3 kt + kf for k < 9, the bias (against a constant 1) at k = 9
    m->tail_w0h3 = pack_h3(P, C / 16, [&](int nt, int l, int i) {
        const int k = 8 * (l >> 4) + i, ch = 16 * nt + (l & 15);
        return k < 9 ? P.out[w0 + (size_t)k * C + ch] : (k == 9 ? P.out[b0 + ch] : 0.f);
    }, &m->tail_w0_unscale);
    // conv0_out's three taps as the rows 0..2 of one 16-row tile; the contraction index is enumerated the way a D fragment leaves it (lane
    // (position, q): element 8 kc + i <-> channel 16 ((8 kc + i) >> 2) + 4 q + ((8 kc + i) & 3))
    m->tail_woh3 = pack_h3(P, KC, [&](int kc, int l, int i) {
        const int j = l & 15, e = 8 * kc + i, ch = 16 * (e >> 2) + 4 * (l >> 4) + (e & 3);
        return j < 3 ? P.out[wo + (size_t)j * C + ch] : 0.f;
    }, &m->tail_wo_unscale);
    P.packed.tail = true;
}
// df_dec.df_convp: the tiled form (dfx_k_df_convp on a materialised c0) and, where 2 * df_order <= 16, the folded sliding-window form
bool prep_df_convp(Prep &P, dfx_model *m) {
    const dfx_model_cfg &c = m->cfg;
    const int C = c.conv_ch, kt = c.df_pathway_kernel_size_t, NO = 2 * c.df_order, G = dfx_gcd(C, NO), CG = C / G, OG = NO / G;
    const int idx = kt > 1 ? 1 : 0;
    const bool has_pw = kt > 1;  // separable only if groups > 1 and max(kernel) > 1; groups > 1 always holds (2 | C, 2O)
    const float *w = P.get("df_dec.df_convp." + std::to_string(idx) + ".weight");
    const float *pw = has_pw ? P.get("df_dec.df_convp." + std::to_string(idx + 1) + ".weight") : nullptr;
    std::vector<float> sc, sh;
    if (!w || (has_pw && !pw) || !P.bn("df_dec.df_convp." + std::to_string(idx + (has_pw ? 2 : 1)), NO, sc, sh)) return false;
    m->cp_G = G;
    m->cp_NO = NO;
    m->cp_w1 = P.alloc((size_t)G * kt * CG * 16);
    m->cp_w2 = P.alloc((size_t)NO * NO);
    m->cp_b = P.alloc(NO);
    for (int g = 0; g < G; ++g)
        for (int k = 0; k < kt; ++k)
            for (int ci = 0; ci < CG; ++ci)
                for (int o = 0; o < OG; ++o) {
                    // weight [NO, CG, kt, 1]
                    float v = w[(((size_t)(g * OG + o) * CG + ci) * kt + k)];
                    if (!has_pw) v *= sc[g * OG + o];
                    P.out[m->cp_w1 + ((((size_t)g * kt + k) * CG + ci) * 16 + o)] = v;
                }
    for (int n = 0; n < NO; ++n) {
        for (int o = 0; o < NO; ++o) P.out[m->cp_w2 + (size_t)n * NO + o] = has_pw ? pw[(size_t)n * NO + o] * sc[n] : (n == o ? 1.f : 0.f);
        P.out[m->cp_b + n] = sh[n];
    }
    // folded form: W_eff[k][c][n] = scale[n] * sum_o PW[n][o] * W1[o][c - group(o)*CG][k]   (PW = identity if absent).
    // One 16-wide MFMA tile of outputs: 2 * df_order <= 16; longer filters (BASELINE.json configs[4]: df_order = 10) take the
    // tiled kernel dfx_k_df_convp on a materialised c0.
    const bool folded = NO <= 16;
    m->cp_weff = P.alloc(folded ? (size_t)kt * C * 16 : 0);
    m->cp_b16 = P.alloc(16);
    for (int k = 0; folded && k < kt; ++k)
        for (int ch = 0; ch < C; ++ch) {
            const int g = ch / CG, ci = ch - g * CG;
            for (int n = 0; n < NO; ++n) {
                double acc = 0.0;
                for (int o = g * OG; o < (g + 1) * OG; ++o) {
                    const double p2 = has_pw ? (double)pw[(size_t)n * NO + o] : (n == o ? 1.0 : 0.0);
                    acc += p2 * (double)w[((size_t)o * CG + ci) * kt + k];
                }
                P.out[m->cp_weff + ((size_t)k * C + ch) * 16 + n] = (float)(acc * (double)sc[n]);
            }
        }
    for (int n = 0; folded && n < NO; ++n) P.out[m->cp_b16 + n] = sh[n];
    return true;
}
// fragments of the fused fp16-split DF-encoder kernels (dfx_k_df_conv01_h3, dfx_k_df_convp_h3): df_conv0, df_conv1's pointwise, folded df_convp
void pack_c0_h3(Prep &P, dfx_model *m) {
    const dfx_model_cfg &c = m->cfg;
    const int C = c.conv_ch, kt = c.df_pathway_kernel_size_t;
    if (C % 32 != 0 || 2 * c.df_order > 16) return;   // (df_convp has its folded form)
    const int KC = C / 32;
    // channel a lane (q = l>>4) feeds as element i of k-chunk kc after dfx_c0_tile
    auto chan = [](int kc, int l, int i) { const int e = 8 * kc + i; return 16 * (e >> 2) + 4 * (l >> 4) + (e & 3); };
    const size_t cin = m->cin_weff, wt1 = m->dfc1.wt, cpw = m->cp_weff;
    m->c0_h3 = pack_h3(P, C / 16, [&](int nt, int l, int i) {
        const int k = 8 * (l >> 4) + i;
        return k < 18 ? P.out[cin + (size_t)k * C + 16 * nt + (l & 15)] : 0.f;
    }, &m->c0_unscale);
    m->dfc1_h3 = pack_h3(P, (C / 16) * KC, [&](int fr, int l, int i) {
        const int nt = fr / KC, kc = fr % KC;
        return P.out[wt1 + (size_t)chan(kc, l, i) * C + 16 * nt + (l & 15)];
    }, &m->dfc1_unscale);
    m->cp_h3 = pack_h3(P, kt * KC, [&](int fr, int l, int i) {
        const int k = fr / KC, kc = fr % KC;
        return P.out[cpw + ((size_t)k * C + chan(kc, l, i)) * 16 + (l & 15)];
    }, &m->cp_unscale);
    P.packed.c0 = true;
}
// fragments of dfx_k_df_out_h3: [G][ceil(Ng / 16)] tiles of 32 x 16
void pack_dfo_h3(Prep &P, dfx_model *m) {
    const GlinW a = m->df_out;
    const int NO = 2 * m->cfg.df_order, Fd = m->cfg.nb_df;
    if (!(a.Kg <= 32 && a.Kg % 8 == 0 && a.Ng % 2 == 0 && NO % 2 == 0 && Fd % 2 == 0 && (int64_t)a.G * a.Ng == (int64_t)NO * Fd &&
          DFX_DFO_SMEM(NO, Fd) <= (size_t)64 * 1024))
        return;
    const int NU = (a.Ng + 15) / 16;
    m->dfo_h3 = pack_h3(P, a.G * NU, [&](int fr, int l, int i) {
        const int g = fr / NU, u = fr % NU, o = 16 * u + (l & 15), k = 8 * (l >> 4) + i;
        return o < a.Ng && k < a.Kg ? P.out[a.w + ((size_t)g * a.Kg + k) * a.Ng + o] : 0.f;
    }, &m->dfo_unscale);
    P.packed.dfo_tiles = NU;
}
// fragments of the fused DF branch of the encoder (dfx_k_df_enc_h3): df_fc_emb in groups of 32 n -> 16 feeding linear_in in groups of 32 -> 16,
// behind the c0 fragments
void pack_dfenc_h3(Prep &P, dfx_model *m) {
    const GlinW a = m->fc_emb, b = m->enc_in;
    const int C = m->cfg.conv_ch, Fout = m->cfg.nb_df / 2, KC = C / 32;
    if (!P.packed.c0) return;
    if (!(a.Kg % 32 == 0 && a.Ng == 16 && b.Kg == 32 && b.Ng == 16 && b.G * 2 == a.G && (int64_t)a.G * a.Kg == (int64_t)Fout * C)) return;
    // chunk ci = fo * KC + kc; lane (o = l & 15, q = l >> 4), element i <-> channel 16 ((8 kc + i) >> 2) + 4 q + (i & 3) of bin fo (the order
    // in which dfx_k_df_conv01_h3's D fragments hold df_conv1's output)
    m->dfenc_fc = pack_h3(P, Fout * KC, [&](int ci, int l, int i) {
        const int fo = ci / KC, kc = ci % KC, ch = 16 * ((8 * kc + i) >> 2) + 4 * (l >> 4) + (i & 3);
        const int idx = fo * C + ch, g = idx / a.Kg, kin = idx % a.Kg;
        return P.out[a.w + ((size_t)g * a.Kg + kin) * 16 + (l & 15)];
    }, &m->dfenc_fc_unscale);
    // linear_in group j: element i <-> feature 16 (i >> 2) + 4 q + (i & 3) of its 32 inputs (two finished fc groups)
    m->dfenc_in = pack_h3(P, b.G, [&](int j, int l, int i) {
        return P.out[b.w + ((size_t)j * 32 + 16 * (i >> 2) + 4 * (l >> 4) + (i & 3)) * 16 + (l & 15)];
    }, &m->dfenc_in_unscale);
    P.packed.dfenc = true;
}

// All of it, in the order of the packed array.  The optional packers (pack_*: void) state their own shape conditions and note in P.packed
// what they made.
bool prepare_weights(Prep &P, dfx_model *m) {
    const dfx_model_cfg &c = m->cfg;
    const int C = c.conv_ch;
    const bool skip_enc = c.emb_gru_skip_enc == DFX_SKIP_GROUPEDLINEAR, skip_dec = c.emb_gru_skip == DFX_SKIP_GROUPEDLINEAR;
    // encoder convolutions
    if (!prep_erb_conv0(P, m)) return false;
    if (!prep_sep(P, "enc.erb_conv1", C, m->erb1) || !prep_sep(P, "enc.erb_conv2", C, m->erb2) || !prep_sep(P, "enc.erb_conv3", C, m->erb3) ||
        !prep_sep(P, "enc.df_conv1", C, m->dfc1))
        return false;
    if (!prep_df_conv0(P, m)) return false;
    // encoder GRU, lsnr, ERB decoder GRU stack
    if (!prep_glin(P, "enc.df_fc_emb.0.weight", m->fc_emb) || !prep_glin(P, "enc.emb_gru.linear_in.0.weight", m->enc_in) ||
        !prep_gru(P, "enc.emb_gru.gru", 1, m->enc_gru) || !prep_glin(P, "enc.emb_gru.linear_out.0.weight", m->enc_out))
        return false;
    if (skip_enc && !prep_glin(P, "enc.emb_gru.gru_skip.weight", m->enc_skip)) return false;
    if (skip_dec && !prep_glin(P, "erb_dec.emb_gru.gru_skip.weight", m->dec_skip)) return false;
    if (!prep_lsnr(P, m)) return false;
    if (!prep_glin(P, "erb_dec.emb_gru.linear_in.0.weight", m->dec_in) || !prep_gru(P, "erb_dec.emb_gru.gru", c.emb_num_layers - 1, m->dec_gru) ||
        !prep_glin(P, "erb_dec.emb_gru.linear_out.0.weight", m->dec_out))
        return false;
    // ERB decoder blocks with their pathway scalars, the pointwise fragments of the six ERB blocks, conv0_out, the tail's two small sets
    if (!prep_sep(P, "erb_dec.convt3", C, m->ct3) || !prep_path(P, "erb_dec.conv3p", C, m->ct3.sk_a, m->ct3.sk_b) ||
        !prep_sep(P, "erb_dec.convt2", C, m->ct2) || !prep_path(P, "erb_dec.conv2p", C, m->ct2.sk_a, m->ct2.sk_b) ||
        !prep_sep(P, "erb_dec.convt1", C, m->ct1) || !prep_path(P, "erb_dec.conv1p", C, m->ct1.sk_a, m->ct1.sk_b) ||
        !prep_path(P, "erb_dec.conv0p", C, m->co_ska, m->co_skb))
        return false;
    m->ct3.has_skip = m->ct2.has_skip = m->ct1.has_skip = true;
    pack_pw_h3(P, m);
    if (!prep_conv0_out(P, m)) return false;
    pack_tail_h3(P, m);
    // DF decoder: df_convp (tiled, folded, fragments), GRU stack, df_out
    if (!prep_df_convp(P, m)) return false;
    pack_c0_h3(P, m);
    if (!prep_glin(P, "df_dec.df_gru.linear_in.0.weight", m->dfg_in) || !prep_gru(P, "df_dec.df_gru.gru", c.df_num_layers, m->df_gru)) return false;
    if (c.df_gru_skip == DFX_SKIP_GROUPEDLINEAR && !prep_glin(P, "df_dec.df_skip.weight", m->df_skip)) return false;
    if (!prep_glin(P, "df_dec.df_out.0.weight", m->df_out)) return false;
    // fragment sets of the fan-out kernels
    pack_fan(P, m);
    pack_encfan(P, m);
    pack_dfo_h3(P, m);
    pack_dfenc_h3(P, m);
    return true;
}
}  // namespace

// Every variable dfx_model_create reads, each with its own parse rule: "off only when 0", "on only when 1", a number.
// First in creation: exact_fp32 steers the packing.
static void read_switches(dfx_model *m) {
    auto is = [](const char *name, char ch) {   // the variable's first character
        const char *v = getenv(name);
        return v && v[0] == ch;
    };
    auto at_least = [](const char *name, int least, int *out) {   // a number >= least, else *out stays
        const char *v = getenv(name);
        if (v && atoi(v) >= least) *out = atoi(v);
    };
    m->exact_fp32 = is("DFX_EXACT_FP32", '1');
    m->concurrent = !is("DFX_STREAMS", '0');   // independent branches of the forward pass run on two auxiliary streams (0: everything serial)
    m->gru_seq = !is("DFX_GRU_SEQ", '0') && !dfx_env_is_emulator();
    if (getenv("DFX_GRU_PAIR")) m->sw.gru_pair = !is("DFX_GRU_PAIR", '0');
    m->sw.gru_pair_far = is("DFX_GRU_PAIR_FAR", '1');
    m->check_every_pass = is("DFX_CHECK_EVERY_PASS", '1');
    at_least("DFX_SYNC_SPIN_LIMIT", 1, &m->spin_limit);
    if (const char *v = getenv("DFX_CONVP_ELEMS"))          // test hook: the 32-bit-offset split of df_convp at small sizes
        if (atoll(v) > 0) m->sw.convp_elems = atoll(v);
    m->sw.erb_enc_split = is("DFX_ERB_ENC_SPLIT", '1');   // test hook: the three-launch form of the ERB encoder in batch passes
    m->sw.c0_presplit = !is("DFX_C0_PRESPLIT", '0');      // test hook: the c0 kernels of batch passes split their feat_spec patches themselves
    if (const char *v = getenv("DFX_WS_FILL"))              // test hook: a pass may not depend on what its workspace held (tests/test_scratch_contents.py)
        if (v[0] >= '0' && v[0] <= '9' && atoi(v) <= 255) m->sw.ws_fill = atoi(v);
#ifdef DFX_DEV
    // dev A/Bs of the phase's side work (product builds have no such switches)
    if (getenv("DFX_TAIL_SPLIT")) m->sw.tail_split = !is("DFX_TAIL_SPLIT", '0');
    at_least("DFX_SEQ_P0_AHEAD", 1, &m->sw.p0_ahead);
    at_least("DFX_SEQ_DFTAIL_EVERY", 1, &m->sw.dftail_every);
    at_least("DFX_SEQ_TAIL_EVERY", 1, &m->sw.tail_every);
    at_least("DFX_SEQ_CHUNKS", 1, &m->sw.chunks);
    at_least("DFX_CONVP_LATE", 0, &m->sw.convp_late);
#endif
    m->sw.seq_trace = is("DFX_SEQ_TRACE", '1');
    int tc = 0;
    at_least("DFX_TCHUNKS", 1, &tc);
    if (tc) m->tchunks = tc < DFX_MAX_TCHUNKS ? tc : DFX_MAX_TCHUNKS;
    m->enqueue_ahead = is("DFX_ENQUEUE_AHEAD", '1');
    m->sw.hwq_probe_mode = is("DFX_HWQ_PROBE", '0') ? '0' : is("DFX_HWQ_PROBE", 'f') ? 'f' : 0;   // "0": no handshake (trust the environment); "fail": dev / test hook
}

// dfx_model::can, from cfg, from what the packers made and from the arithmetic mode (the forms that rounds 2-5 could select by environment were
// measured and lost; tools/dev/patches/ keeps the experiments).  The rules are written here and nowhere else.
static void model_capabilities(dfx_model *m, const Prep::Packed &k) {
    const dfx_model_cfg &c = m->cfg;
    const int C = c.conv_ch, E = c.nb_erb, Fd = c.nb_df, NO = 2 * c.df_order, emb = C * E / 4;
    const bool split = !m->exact_fp32;   // fp16-split matrix ops (default)
    DfxCan &can = m->can;
    can.fuse_c0 = c.df_pathway_kernel_size_t <= 5 && NO <= 16;
    can.c0_batch_unfused = m->exact_fp32 && can.fuse_c0;
    can.c0_h3 = can.fuse_c0 && split && k.c0;
    can.c0_presplit = m->sw.c0_presplit && can.c0_h3;
    can.pw_h3 = split && k.pw;
    can.fan = k.fan && !c.enc_concat && emb == 64 * m->fan_chunks;   // (exact fp32 matrix ops: also with DFX_EXACT_FP32=1)
    can.fan_skp = can.fan && c.df_gru_skip == DFX_SKIP_GROUPEDLINEAR && k.fan_skp;
    can.enc_fan = k.encfan && !c.enc_concat && emb == 16 * m->efan_groups;
    can.dfenc = can.c0_h3 && can.enc_fan && k.dfenc;
    can.fuse_enc = E % 2 == 0 && 3 * (E + 2) <= 192 && 2 * DFX_ENC_SMEM(C, E) <= (size_t)160 * 1024;
    can.erb_tail = can.pw_h3 && k.tail && dfx_tail_ok(C, E);
    // (dfx_k_erb_enc4's strips assume what DeepFilterNet3's encoder is: erb_conv1..3 of kernel 1 x 3 over frequency, strides 2 / 2 / 1 — the only
    // form prep_sep packs for these layers)
    can.erb_enc4 = can.fuse_enc && can.pw_h3 && dfx_enc4_ok(C, E);
    // df_out's fragments resident in registers when a wave's share fits: <= 16 groups of <= 4 tiles — every shipped shape
    const bool resident = k.dfo_tiles == 4 && m->df_out.G <= 16 && (int64_t)(NO / 2) * 16 * (Fd / 2) <= (int64_t)DFX_DFO_NPT * DFX_DFO_THREADS;
    can.df_out = !(split && k.dfo_tiles > 0) ? DFX_PLAN_DF_OUT_GGEMM : resident ? DFX_PLAN_DF_OUT_RESIDENT : DFX_PLAN_DF_OUT_STREAMING;
}

// Sync words, error words, events and the streams of lane 0.
static int create_device_objects(dfx_model *m) {
    if (m->sw.seq_trace) (void)hipMalloc(reinterpret_cast<void **>(&m->d_trace), (size_t)DFX_MAX_GRU_LAYERS * DFX_SEQ_GMAX * DFX_GS_MAX_CHUNKS * 3 * 8);
    const size_t sync_bytes = DfxSyncLayout::total * sizeof(unsigned int);
    const size_t psync_bytes = (size_t)DFX_MAX_GRU_LAYERS * (DFX_SEQ_GMAX / 2) * 48 * sizeof(unsigned int);
    if (hipMalloc(reinterpret_cast<void **>(&m->d_psync), psync_bytes) != hipSuccess || hipMemset(m->d_psync, 0, psync_bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&m->d_sync), sync_bytes) != hipSuccess || hipMemset(m->d_sync, 0, sync_bytes) != hipSuccess ||
        dfx_env_err_words_alloc(&m->h_err, &m->d_err, 256) != hipSuccess)
        DFX_FAIL(DFX_ERR_ALLOC, "dfx_model_create: device allocation failed");
    // Streams are created sparingly: ROCm multiplexes them onto GPU_MAX_HW_QUEUES hardware queues and two live streams
    // that share a queue serialise each other.  Lane 0 gets exactly the streams its model needs; lanes 1.. (batch-chunk
    // pipelining, off by default) are created on demand by dfx_model_set_pipeline.
    bool good = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&m->ev_pass, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&m->ev_gate, hipEventDisableTiming) == hipSuccess;
    good = good && dfx_create_lane(m, 0);
    for (int l = 1; l < m->max_chunks && good; ++l) good = dfx_create_lane(m, l);
    if (!good) DFX_FAIL(DFX_ERR_HIP, "dfx_model_create: could not create the auxiliary streams/events");
    return DFX_OK;
}

// create = check, switches, weights, upload, capabilities, device-side objects, handshake arming
extern "C" int dfx_model_create(const dfx_model_cfg *cfg, const float *blob, dfx_model **out) {
    if (int rc = check_cfg(cfg)) return rc;
    if (!blob || !out) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_create: null");
    if (int rc = dfx_require_device()) return rc;
    dfx_model *m = new dfx_model();
    m->cfg = *cfg;
    read_switches(m);
    const DfxManifest man = dfx_build_manifest(m->cfg);
    Prep P{blob, man};
    P.exact_fp32 = m->exact_fp32;
    if (!prepare_weights(P, m)) {
        delete m;
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_create: %s", P.err.empty() ? "weight preparation failed" : P.err.c_str());
    }
    m->n_w = P.out.size();
    if (hipMalloc(reinterpret_cast<void **>(&m->d_w), m->n_w * sizeof(float)) != hipSuccess) {
        delete m;
        DFX_FAIL(DFX_ERR_ALLOC, "dfx_model_create: device allocation of %zu bytes failed", m->n_w * sizeof(float));
    }
    if (hipMemcpy(m->d_w, P.out.data(), m->n_w * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        dfx_model_free(m);
        DFX_FAIL(DFX_ERR_HIP, "dfx_model_create: upload failed");
    }
    model_capabilities(m, P.packed);
    if (int rc = create_device_objects(m)) {
        dfx_model_free(m);
        return rc;
    }
    // The persistent GRU phase synchronises through device flags and needs its streams to run concurrently: checked with a handshake
    // (hwq_probe_run) — not here but before the first pass that would use the persistent form, or when DFX_Q_HWQ_PROBE /
    // DFX_Q_GRU_PERSISTENT is asked for: a process that creates many handles it only streams through (df_create: one state per
    // stream, never a persistent phase) pays nothing for it.  DFX_HWQ_PROBE=0: skip it (trust the environment); "fail": dev / test hook
    if (m->gru_seq && m->concurrent && !dfx_env_is_emulator()) {
        if (m->sw.hwq_probe_mode == 'f') {
            m->hwq_probe = 0;
            hwq_probe_fallback(m);
        } else if (m->sw.hwq_probe_mode != '0') {
            m->hwq_probe_pending = true;
        }
    }
    *out = m;
    return DFX_OK;
}

static void pass_gate_forget(const dfx_model *m);
extern "C" void dfx_model_free(dfx_model *m) {
    if (!m) return;
    pass_gate_forget(m);   // (first: nobody may wait on ev_gate once it is destroyed; the lanes are the process's and stay)
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_pass) (void)hipEventDestroy(m->ev_pass);
    if (m->ev_gate) (void)hipEventDestroy(m->ev_gate);
    dfx_env_err_words_free(m->h_err);
    if (m->d_sync && m->d_trace) {   // dev aid (DFX_SEQ_TRACE=1): how many block hand-overs of the followers took the same-XCD form
        unsigned int n = 0;
        if (hipMemcpy(&n, m->d_sync + DfxSyncLayout::xstat, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess) fprintf(stderr, "[dfx] same-XCD (light) block hand-overs over the model's life: %u\n", n);
    }
    if (m->d_sync) (void)hipFree(m->d_sync);
    if (m->d_psync) (void)hipFree(m->d_psync);
    if (m->d_trace) (void)hipFree(m->d_trace);
    if (m->d_w) (void)hipFree(m->d_w);
    delete m;
}
extern "C" int dfx_model_set_streams(dfx_model *m, int enable) {
    if (!m) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    m->concurrent = enable != 0;
    return DFX_OK;
}
extern "C" int dfx_model_set_run_df(dfx_model *m, int enable) {
    if (!m) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    m->run_df = enable != 0;
    return DFX_OK;
}
extern "C" int dfx_model_set_pipeline(dfx_model *m, int time_chunks, int min_chunk_frames, int batch_chunks) {
    if (!m || time_chunks < 1 || min_chunk_frames < 1 || batch_chunks < 1) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_set_pipeline: bad arguments");
    m->tchunks = time_chunks < DFX_MAX_TCHUNKS ? time_chunks : DFX_MAX_TCHUNKS;
    m->tchunk_min = min_chunk_frames;
    m->max_chunks = batch_chunks < DFX_MAX_LANES ? batch_chunks : DFX_MAX_LANES;
    for (int l = 1; l < m->max_chunks; ++l)
        if (!dfx_create_lane(m, l)) DFX_FAIL(DFX_ERR_HIP, "dfx_model_set_pipeline: could not create the streams of lane %d", l);
    return DFX_OK;
}
// Reads (and clears) the error words without waiting for anything: faults of work that has completed.  Each word is taken with one
// atomic exchange, so a word the device raises while the host is looking is either seen now or stays set for the next look — never
// lost.  (A fault of an unthrottled small pass can therefore still surface one call later than the pass that raised it: only
// dfx_model_check / DFX_CHECK_EVERY_PASS=1 wait for the device first.)
static int model_poll(const dfx_model *m) {
    unsigned int *h = m->h_err;
    if (!h) return DFX_OK;
    if (!(((volatile unsigned int *)h)[1] | ((volatile unsigned int *)h)[2])) return DFX_OK;
    const unsigned int e1 = __atomic_exchange_n(&h[1], 0u, __ATOMIC_ACQ_REL), e2 = __atomic_exchange_n(&h[2], 0u, __ATOMIC_ACQ_REL);
    if (!(e1 | e2)) return DFX_OK;
    if (e2)
        DFX_FAIL(DFX_ERR_HIP, "dfx: a flag wait of the persistent GRU phase timed out (bounded spin: the streams of the pass did not make progress "
                              "independently — hardware queues shared with other work, or the GPU shared with another process); the results of "
                              "the previous pass on this model are invalid.  DFX_GRU_SEQ=0 selects the event-synchronised form");
    DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx: an activation of magnitude >= 6e4 reached an fp16-split matrix kernel (GRU / DF-encoder / separable-conv "
                                  "path); the results of the previous pass on this model are invalid.  DFX_EXACT_FP32=1 selects the exact fp32 kernels");
}
extern "C" int dfx_model_poll(const dfx_model *m) {
    if (!m) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    return model_poll(m);
}
extern "C" int dfx_model_check(const dfx_model *m) {
    if (!m) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    DFX_HIP(hipDeviceSynchronize());   // every stream of the process: whatever this model has in flight is over
    return model_poll(m);
}
extern "C" int dfx_model_query(const dfx_model *m, int what, int64_t *value) {
    if (!m || !value) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_query: null");
    switch (what) {
        case DFX_Q_GRU_PERSISTENT:
        case DFX_Q_HWQ_PROBE: {
            std::lock_guard<std::mutex> lk(dfx_enqueue_mu());
            hwq_probe_run(const_cast<dfx_model *>(m));
            *value = what == DFX_Q_HWQ_PROBE ? m->hwq_probe : (m->gru_seq && m->concurrent ? 1 : 0);
            return DFX_OK;
        }
        case DFX_Q_EXACT_FP32: *value = m->exact_fp32 ? 1 : 0; return DFX_OK;
        case DFX_Q_PASSES_PERSISTENT: *value = m->passes_seq; return DFX_OK;
        case DFX_Q_PASSES_TICKET_BUSY: *value = m->passes_ev; return DFX_OK;
        case DFX_Q_SPIN_LIMIT: *value = m->spin_limit; return DFX_OK;
        case DFX_Q_PASSES_C0_PRESPLIT: *value = m->passes_ps; return DFX_OK;
        case DFX_Q_LAST_PLAN: *value = m->last_plan; return DFX_OK;
        case DFX_Q_PASSES_PAIR: *value = m->passes_pair; return DFX_OK;
    }
    DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_query: unknown item %d", what);
}
// dev aid: chunk timestamps (100 MHz ticks) of the last persistent GRU launch, [layers][groups][chunks][3]; dims -> {layers, groups, chunks}
extern "C" int dfx_model_seq_trace(const dfx_model *m, unsigned long long *out_host, int64_t cap, int *dims) {
    if (!m || !m->d_trace || !out_host || !dims) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_seq_trace: tracing is off (DFX_SEQ_TRACE=1 at model creation)");
    const int64_t n = (int64_t)m->trace_dims[0] * m->trace_dims[1] * m->trace_dims[2] * 3;
    if (n > cap) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_seq_trace: buffer too small");
    DFX_HIP(hipMemcpy(out_host, m->d_trace, (size_t)n * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) dims[i] = m->trace_dims[i];
    return DFX_OK;
}
extern "C" int dfx_model_cfg_get(const dfx_model *m, dfx_model_cfg *out) {
    if (!m || !out) DFX_FAIL(DFX_ERR_INVALID_ARG, "null");
    *out = m->cfg;
    return DFX_OK;
}

// The pass-dependent half of "the DF branch of the encoder runs as the one kernel dfx_k_df_enc_h3" (DfxPass::plan(): dfenc = fuse_h3 && this).
// feat_T: frames per clip of the feature arrays (0: T).  The limits are the kernel's 32-bit element offsets; beyond them the two kernels run.
static inline bool dfx_dfenc_ok(const dfx_model *m, int64_t B, int64_t T, int64_t feat_T) {
    const dfx_model_cfg &c = m->cfg;
    const int64_t emb = (int64_t)c.conv_ch * c.nb_erb / 4;
    return m->can.dfenc && B * T * emb < ((int64_t)1 << 31) && B * (feat_T > 0 ? feat_T : T) * c.nb_df < ((int64_t)1 << 29);
}
// Is the pre-split copy ALL a batch pass reads of feat_spec?  The front takes the fused DF encoder and df_convp its PS instance: enhance() then has
// the norm scan store the copy INSTEAD of the fp32 values (the scan is bound by its stores).  DfxPass::plan() decides with the same two.
static inline bool dfx_feat_spec_unread(const dfx_model *m, int64_t B, int64_t T) { return m->can.c0_presplit && dfx_dfenc_ok(m, B, T, 0); }
// where model_forward_lane places the model's arrays inside the workspace it is given
static inline float *dfx_ws_base(void *workspace) { return reinterpret_cast<float *>(((uintptr_t)workspace + 255) & ~(uintptr_t)255); }

// ------------------------------------------------------------------------------------------------ workspace plan
namespace {
struct Ws {
    // offsets in floats, each 64-float (256 B) aligned
    size_t e0, e1, e2, e3, c0, c1, emb_in, emb, xa, xb, gi, xa2, xb2, gi2, demb, d3, d2, mask, c0p, xdf, coefs, lsnr, skp_e, skp_d, fps, total;
    size_t pgi[DFX_MAX_GRU_LAYERS], py[DFX_MAX_GRU_LAYERS], ph[DFX_MAX_GRU_LAYERS];  // layer-pipelined GRU phase: gi, y, h state per layer
};
Ws plan_ws(const dfx_model *m, int64_t R, int64_t B) {
    const dfx_model_cfg &c = m->cfg;
    const bool c0_stored = !m->can.fuse_c0 || m->can.c0_batch_unfused, presplit = m->can.c0_presplit;
    Ws w{};
    size_t off = 0;
    auto take = [&](size_t n) {
        size_t o = off;
        off += (n + 63) & ~(size_t)63;
        return o;
    };
    const size_t C = c.conv_ch, E = c.nb_erb, Fd = c.nb_df, emb = C * E / 4, NO = 2 * c.df_order;
    w.e0 = take(R * E * C);
    w.e1 = take(R * (E / 2) * C);
    w.e2 = take(R * (E / 4) * C);
    w.e3 = take(R * (E / 4) * C);
    w.c0 = c0_stored ? take(R * Fd * C) : 0;  // only materialised by the unfused DF-encoder path
    w.c1 = take(R * (Fd / 2) * C);
    w.emb_in = take(R * emb * (c.enc_concat ? 2 : 1));
    w.emb = take(R * emb);
    w.xa = take(R * 256);
    w.xb = take(R * 256);
    w.gi = take(R * 768);
    w.xa2 = take(R * 256);  // the DF decoder's GRU stack runs concurrently with the ERB decoder's
    w.xb2 = take(R * 256);
    w.gi2 = take(R * 768);
    w.demb = take(R * emb);
    w.d3 = take(R * (E / 4) * C);
    w.d2 = take(R * (E / 2) * C);
    w.mask = take(R * E);
    w.c0p = take(R * Fd * NO);
    w.xdf = take(R * 256);
    w.coefs = take(R * Fd * NO);
    w.lsnr = take(R);
    w.skp_e = take(c.emb_gru_skip_enc == DFX_SKIP_GROUPEDLINEAR ? R * emb : 0);   // grouped-linear skips around the embedding GRUs
    w.skp_d = take(c.emb_gru_skip == DFX_SKIP_GROUPEDLINEAR ? R * emb : 0);
    w.fps = take(presplit ? R * Fd * 2 : 0);   // the pre-split copy of feat_spec: 8 bytes per complex value (dfx_pack_h3), read by the PS instances of the c0 kernels
    const int nlayers = 1 + (c.emb_num_layers - 1) + c.df_num_layers;
    for (int l = 0; l < DFX_MAX_GRU_LAYERS; ++l) {
        const bool used = l < nlayers;
        w.pgi[l] = take(used ? R * 768 : 0);
        w.py[l] = take(used ? R * 256 : 0);
        w.ph[l] = take(used ? (B > 0 ? B : R) * 256 : 0);
    }
    w.total = off;
    return w;
}
}  // namespace

extern "C" int dfx_model_workspace_bytes(const dfx_model *m, int64_t B, int64_t T, int64_t *bytes) {
    if (!m || !bytes || B < 0 || T < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_model_workspace_bytes: bad arguments");
    *bytes = (int64_t)(plan_ws(m, B * T, B).total * sizeof(float)) + 256;
    return DFX_OK;
}

// ---- the rest of this translation unit, by concern
#include "dfx_model_launch.h"
#include "dfx_model_forward.h"
#include "dfx_model_stream.h"
#include "dfx_stream_move.h"
#include "dfx_model_enhance.h"
