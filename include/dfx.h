/*
 * dfx.h — C ABI of libdfx.so, the MI355X (gfx950) engine for DeepFilterNet's enhance() hot path.
 *
 * Drop-in boundary.  Every entry point names the reference interface it replaces
 * (paths relative to the reference checkout):
 *   - pyDF/src/lib.rs (pyo3 module `libdf`)  : class DF + erb / erb_inv / erb_norm / unit_norm / unit_norm_init
 *   - libDF/src/lib.rs, libDF/src/transforms.rs : DFState and the batched transforms behind it
 *   - DeepFilterNet/df/multiframe.py:160-180, DeepFilterNet/df/modules.py:226-269 : MF.DF and Mask (device ops)
 *   - DeepFilterNet/df/deepfilternet3.py:334-456, DeepFilterNet/df/enhance.py:190-250 : DfNet.forward, enhance()
 *   - libDF/src/capi.rs:83-253 : naming / ownership conventions (opaque handles, caller-owned buffers)
 *
 * Conventions
 *   - plain C types only; complex numbers are interleaved float pairs (re, im) == Complex32 == numpy complex64
 *   - every data pointer is a DEVICE pointer on the current HIP device unless the name ends in `_host`
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on that stream
 *   - all arrays are dense row-major ("C-contiguous") unless a stride argument is given
 *   - return value: DFX_OK or an error code; dfx_last_error() gives a thread-local message.  Nothing panics/aborts.
 *   - no hidden host<->device copies in the batched entry points; nothing here falls back to a CPU implementation
 */
#ifndef DFX_H
#define DFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_OK 0
#define DFX_ERR_INVALID_ARG 1
#define DFX_ERR_UNSUPPORTED 2
#define DFX_ERR_HIP 3
#define DFX_ERR_NO_DEVICE 4
#define DFX_ERR_ALLOC 5

#define DFX_VERSION 200 /* 0.2.0 */

/* G.711 companding laws (dfx_g711_decode / _encode, dfx_stream_process_g711) and the sample formats of dfx_stream_resampler_process */
#define DFX_G711_ULAW 1
#define DFX_G711_ALAW 2
#define DFX_FMT_F32 0   /* float32 */
#define DFX_FMT_PCM16 1 /* int16: x / 32768 in, dfx_f32_to_pcm16's encoding out */
#define DFX_FMT_ULAW 2  /* uint8 G.711 mu-law codes */
#define DFX_FMT_ALAW 3  /* uint8 G.711 A-law codes */

int dfx_version(void);
const char *dfx_status_string(int status);
const char *dfx_last_error(void);
/* Number of usable HIP devices (0 => every compute entry point returns DFX_ERR_NO_DEVICE). */
int dfx_device_count(void);
/* 1 when this library is the CPU SIMT interpreter build used by unit tests (tests/hipemu), 0 for the product. */
int dfx_is_emulator(void);

/* ------------------------------------------------------------------------------------------------------------------
 * ERB band table.  Replaces the `erb_fb: &[usize]` argument of libDF (lib.rs:280-348) / pyDF (lib.rs:142-250).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dfx_bands dfx_bands;
int dfx_bands_create(const uint64_t *widths_host, int nb_bands, dfx_bands **out);
void dfx_bands_free(dfx_bands *b);
int dfx_bands_nb(const dfx_bands *b);
int dfx_bands_nfreqs(const dfx_bands *b);

/* ------------------------------------------------------------------------------------------------------------------
 * DF state.  Replaces DFState::new (libDF/src/lib.rs:104-154) and pyDF's class DF (pyDF/src/lib.rs:14-136).
 * The handle is immutable after creation (window, twiddles, band table live on the device); streaming memories are
 * explicit caller-owned buffers (mem_in / mem_out below), so one handle serves any number of concurrent batches.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dfx_state dfx_state;
/* Fails with DFX_ERR_INVALID_ARG if hop*2 > fft (lib.rs:111 assert) and DFX_ERR_UNSUPPORTED if fft is odd, if fft/2 has a
 * prime factor other than 2, 3, 5, if more than 8 frames overlap (fft / hop rounded up), or if the LDS-resident transforms
 * of this size do not fit a workgroup: the analysis launch needs 76 * fft + 256 bytes of LDS and about 12 bytes per ERB band
 * of tables (2.9 KB at 8 bands, 3.6 KB at 64), against 163 840 bytes.  fft = 2048 fits, fft = 2160 does not; the message
 * names the bytes asked for and the limit.  The same limit holds on the CPU interpreter build. */
int dfx_state_create(int sr, int fft_size, int hop_size, int nb_bands, int min_nb_erb_freqs, dfx_state **out);
void dfx_state_free(dfx_state *st);
int dfx_state_sr(const dfx_state *st);
int dfx_state_fft_size(const dfx_state *st);
int dfx_state_hop_size(const dfx_state *st);
int dfx_state_nb_erb(const dfx_state *st);
float dfx_state_wnorm(const dfx_state *st);
const dfx_bands *dfx_state_bands(const dfx_state *st);
int dfx_state_erb_widths(const dfx_state *st, uint64_t *out_host /*[nb_erb]*/);   /* DF.erb_widths() */
int dfx_state_fft_window(const dfx_state *st, float *out_host /*[fft_size]*/);    /* DF.fft_window() */
/* libDF/src/lib.rs:68-100 erb_fb() on the host (pure index arithmetic, bit-exact). */
int dfx_erb_fb(int sr, int fft_size, int nb_bands, int min_nb_freqs, uint64_t *out_host);

/* DF.analysis (pyDF/src/lib.rs:41-72 -> lib.rs:356-394), batched over B independent rows.
 *   x      [B, T] f32            (row stride x_stride elements, >= T)
 *   spec   [B, T/hop, F][2] f32  (trailing T%hop samples are dropped, like chunks_exact)
 *   mem_in [B, fft-hop] or NULL  analysis memory before the first frame (NULL == reset == zeros)
 *   mem_out[B, fft-hop] or NULL  analysis memory after the last frame */
int dfx_analysis(const dfx_state *st, const float *x, int64_t B, int64_t T, int64_t x_stride, const float *mem_in,
                 float *mem_out, float *spec, void *stream);

/* DF.synthesis (pyDF/src/lib.rs:74-107 -> lib.rs:396-427), batched.  Does NOT modify `spec` (the reference clobbers
 * it).  imag(DC) and imag(Nyquist) are ignored (lib.rs:398-405).
 *   spec [B, Tf, F][2];  out [B, Tf*hop] (row stride out_stride);  mem_* [B, fft-hop] synthesis overlap memory. */
int dfx_synthesis(const dfx_state *st, const float *spec, int64_t B, int64_t Tf, const float *mem_in, float *mem_out,
                  float *out, int64_t out_stride, void *stream);

/* erb() (pyDF/src/lib.rs:142-192 -> transforms.rs:236-253, lib.rs:280-295): spec [rows, F][2] -> out [rows, nb]. */
int dfx_erb(const dfx_bands *bands, const float *spec, int64_t rows, int db, float *out, void *stream);
/* erb_inv() (pyDF/src/lib.rs:194-250 -> lib.rs:339-348): gains [rows, nb] -> out [rows, F]. */
int dfx_erb_inv(const dfx_bands *bands, const float *gains, int64_t rows, float *out, void *stream);
/* erb_norm() (pyDF/src/lib.rs:252-274 -> transforms.rs:301-330, lib.rs:244-251).  x [C, T, E] normalised IN PLACE.
 * state [C, E] in/out or NULL (NULL: linspace(-60,-90,E) per row, final state discarded). */
int dfx_erb_norm(float *x, int64_t C, int64_t T, int E, float alpha, float *state, void *stream);
/* unit_norm() (pyDF/src/lib.rs:276-298 -> transforms.rs:332-361, lib.rs:253-259).
 * x [C, T, F][2] read with frame stride x_frame_stride complex elements (lets spec[..., :nb_df] be read without a copy);
 * out [C, T, F][2] dense.  state [C, F] in/out or NULL (NULL: linspace(1e-3,1e-4,F)). */
int dfx_unit_norm(const float *x, int64_t x_frame_stride, float *out, int64_t C, int64_t T, int F, float alpha,
                  float *state, void *stream);
/* unit_norm_init() (pyDF/src/lib.rs:300-309). */
int dfx_unit_norm_init(int n, float *out_host);

/* df_features() (DeepFilterNet/df/enhance.py:190-203) fused on the device: analysis + erb(dB) + erb_norm + unit_norm.
 *   x [B, T] -> spec [B, Tf, F][2], erb_feat [B, Tf, nb_erb], spec_feat [B, Tf, nb_df][2];  states reset per row. */
int dfx_features(const dfx_state *st, const float *x, int64_t B, int64_t T, int64_t x_stride, int nb_df, float alpha,
                 float *spec, float *erb_feat, float *spec_feat, void *stream);

/* Deep filtering + ERB gains + post filter + attenuation limit, one fused memory-bound kernel.
 * Replaces MF.DF.forward (multiframe.py:169-180), Mask.forward (modules.py:248-269; == lib.rs:314-326), the combine
 * step of DfNet.forward (deepfilternet3.py:442-443), its post filter (:448-454; == lib.rs:446-471) and enhance()'s
 * atten_lim mix (enhance.py:238-240).
 *   spec  [B, T, F][2]   noisy spectrum
 *   coefs complex, nb_df bins, `order` taps:  layout DFX_COEF_BOTF = [B, O, T, nb_df][2]  (MF.DF's input)
 *                                             layout DFX_COEF_BTFO = [B, T, nb_df, O][2]  (DfDecoder's raw output)
 *                                             layout DFX_COEF_BTOF = [B, T, O, nb_df][2]
 *   gains [B, T, nb_bands] or NULL.  NULL: bins >= nb_df are copied from spec (plain MF.DF semantics).
 *   out   [B, T, F][2]   must not alias spec
 *   out[b,t,f<nb_df]  = sum_n coefs[b,n,t,f] * spec[b, t+n-(order-1-lookahead), f]   (zero outside [0,T))
 *   out[b,t,f>=nb_df] = spec[b,t,f] * gains[b,t,band(f)]
 *   pf_beta > 0: post filter;  atten_lim in (0,1): out = spec*atten_lim + out*(1-atten_lim). */
#define DFX_COEF_BOTF 0
#define DFX_COEF_BTFO 1
#define DFX_COEF_BTOF 2 /* [B, T, O, nb_df][2] */
int dfx_df_apply(const float *spec, const float *coefs, int coef_layout, const float *gains, const dfx_bands *bands,
                 int64_t B, int64_t T, int F, int nb_df, int order, int lookahead, float pf_beta, float atten_lim,
                 float *out, void *stream);
/* The same operator on rows with a stride (complex elements, >= F): spec [B,T,spec_stride][2] -> out [B,T,out_stride][2].  Even
 * strides make every row 16-byte aligned (F = fft/2 + 1 is odd for every shipped model) and select the row-streaming kernel the
 * engine uses on its own padded buffers; pad bins of `out` are written as zeros.  No reference counterpart (layout extension). */
int dfx_df_apply_strided(const float *spec, int64_t spec_stride, const float *coefs, int coef_layout, const float *gains,
                         const dfx_bands *bands, int64_t B, int64_t T, int F, int nb_df, int order, int lookahead, float pf_beta,
                         float atten_lim, float *out, int64_t out_stride, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * DeepFilterNet3 model.  Replaces df.deepfilternet3.DfNet (deepfilternet3.py:334-456) for inference.
 * ---------------------------------------------------------------------------------------------------------------- */
#define DFX_SKIP_NONE 0
#define DFX_SKIP_IDENTITY 1
#define DFX_SKIP_GROUPEDLINEAR 2

typedef struct dfx_model_cfg {
    /* [df] section (config.py:12-39) */
    int32_t sr, fft_size, hop_size, nb_erb, nb_df, min_nb_freqs, df_order, df_lookahead;
    int32_t lsnr_min, lsnr_max;
    /* [deepfilternet] section (deepfilternet3.py:25-77) */
    int32_t conv_lookahead, conv_ch, emb_hidden_dim, emb_num_layers, df_hidden_dim, df_num_layers;
    int32_t df_gru_skip; /* DFX_SKIP_* */
    int32_t df_pathway_kernel_size_t, lin_groups, enc_lin_groups;
    int32_t mask_pf;
    float pf_beta;
    float norm_alpha; /* utils.py:111-127 get_norm_alpha() */
    /* skip connections around the embedding GRUs (SqueezedGRU_S gru_skip_op, modules.py:702-738: x = linear_out(gru(linear_in(in))) +
     * skip(in); deepfilternet3.py:138-146 encoder, :198-206 ERB decoder) and the encoder's combine op (:132-136): DFX_SKIP_* / 0|1 */
    int32_t emb_gru_skip_enc, emb_gru_skip, enc_concat;
} dfx_model_cfg;

/* Tensor manifest: the tensors of the reference state-dict the engine consumes, in state_dict() order, with their
 * reference names ("enc.erb_conv0.1.weight", ...).  The host packs them (raw, un-folded float32) into one blob. */
int dfx_model_tensor_count(const dfx_model_cfg *cfg, int *count);
int dfx_model_tensor_info(const dfx_model_cfg *cfg, int index, char *name_out, int name_cap, int64_t shape_out[4],
                          int *ndim_out, int64_t *offset_out /* in floats */);
int dfx_model_blob_floats(const dfx_model_cfg *cfg, int64_t *n);

typedef struct dfx_model dfx_model;
/* Folds BatchNorm (eval mode, eps 1e-5) into the preceding convolution, re-lays the weights out for the kernels and
 * uploads them.  blob_host: float32[dfx_model_blob_floats] packed per dfx_model_tensor_info. */
int dfx_model_create(const dfx_model_cfg *cfg, const float *blob_host, dfx_model **out);
void dfx_model_free(dfx_model *m);
/* .dfx model file = the configuration + the packed blob above ("DFXM", version, cfg, float32 data; written by
 * deepfilternet_amd.export_dfx from a reference model directory or state-dict).  It is what df_create() (include/df_capi.h, the
 * reference's C API) takes as its model path, in place of the reference's tar.gz of ONNX graphs (tract.rs:37-70). */
int dfx_model_save_file(const dfx_model_cfg *cfg, const float *blob_host, const char *path);
/* Takes either file kind (told apart by their magic bytes): a .dfx file, or the reference's own `<model>_onnx.tar.gz` (below). */
int dfx_model_load_file(const char *path, dfx_model **out);
/* The reference's shipped model artefact (libDF/src/tract.rs:29-70 DfParams::from_targz; written by
 * DeepFilterNet/df/scripts/export.py:331-337): a gzip'ed tar of enc.onnx, erb_dec.onnx, df_dec.onnx and config.ini.  The DSP
 * parameters come from the config.ini keys DfTract::new reads (tract.rs:264-315), the network structure and the weights from the
 * three ONNX graphs (BatchNorm as folded by the exporter, GRU gates re-ordered z,r,h -> r,z,n); the result is the
 * (configuration, packed state-dict blob) pair of dfx_model_create().  blob_out may be NULL to query *blob_floats. */
int dfx_onnx_targz_read(const char *path, dfx_model_cfg *cfg_out, float *blob_out, int64_t blob_cap, int64_t *blob_floats);
int dfx_model_cfg_get(const dfx_model *m, dfx_model_cfg *out);
/* The forward pass runs its independent branches (ERB encoder/decoder | DF encoder/decoder | df_convp) on internal
 * streams, forked from and joined to the caller's stream with events.  enable = 0 serialises everything on the caller's
 * stream (useful for per-kernel timing).  Default: enabled (environment DFX_STREAMS=0 disables at creation). */
int dfx_model_set_streams(dfx_model *m, int enable);
/* DfNet(run_df=False) (deepfilternet3.py:383,433-443; init_df(mask_only=True), enhance.py:109,172-175): the DF decoder does not run,
 * the enhanced spectrum is the masked spectrum on every bin, df_coefs is not produced (a caller's buffer is zero-filled).  Read by
 * every pass: set it before the first call of a stream handle made on the model, not while one is running. */
int dfx_model_set_run_df(dfx_model *m, int enable);
/* Pipelining knobs (defaults 12, 32, 1; time_chunks <= 16; environment DFX_TCHUNKS / DFX_CHUNKS at creation):
 *   time_chunks      the GRU phase is cut into this many time chunks and every GRU layer runs on its own stream, chunk k of
 *                    layer l starting when layer l-1 has produced chunk k (chain = T*(1 + 2/K) steps instead of 3T);
 *   min_chunk_frames shortest chunk worth a launch;
 *   batch_chunks     dfx_enhance additionally pipelines this many batch chunks (multiples of 16 clips) on separate stream sets.
 * The streams need their own hardware queues: export GPU_MAX_HW_QUEUES=24 before HIP initialises (ROCm maps streams onto 4 queues by
 * default; the Python package sets it on import if it is unset).  The persistent, flag-synchronised GRU phase REQUIRES that its ~8
 * streams make progress independently; the engine checks that with a handshake between them (DFX_Q_HWQ_PROBE) — once per handle, before the
 * first pass that would use the persistent form (handles that are only streamed through never pay for it) — and selects the
 * event-synchronised form when they do not.  Co-residency with another process's kernels is not under the engine's control: a
 * starved flag wait then ends as a reported DFX_ERR_HIP (see dfx_model_check), never as silent garbage or a hang. */
int dfx_model_set_pipeline(dfx_model *m, int time_chunks, int min_chunk_frames, int batch_chunks);
/* Faults a kernel can find while it runs — an activation that left the range of the fp16-split matrix kernels (|x| >= 6e4 at a
 * split: DFX_ERR_UNSUPPORTED; DFX_EXACT_FP32=1 selects the exact fp32 kernels), a flag wait of the persistent GRU phase that timed out
 * (bounded spins, the engine never hangs: DFX_ERR_HIP) — are raised in error words
 * of the model that the device writes and the host reads.  The results of the pass that raised one are INVALID, and no call hides
 * that: every entry point that starts work on the model (dfx_enhance, dfx_model_forward, dfx_stream_process[_raw]) first looks at
 * the words and returns the error of the PREVIOUS pass instead of starting (each word is cleared, atomically, by being reported; a big pass
 * waits for its predecessor anyway, see dfx_enhance).  So a fault of a BIG pass (>= 16384 frames) is reported by the next call at the
 * latest; small passes are not waited for, so a fault of small pass N may only have been raised when call N + 2 looks — a hard
 * guarantee for the last results of a sequence takes dfx_model_check (or DFX_CHECK_EVERY_PASS=1);
 *   dfx_model_poll   looks now, without waiting (faults of work that has completed);
 *   dfx_model_check  waits for the device, then looks: call it before trusting the LAST results of a sequence of calls;
 *   DFX_CHECK_EVERY_PASS=1 (environment, read at dfx_model_create): every call waits for its own pass and reports its own faults.
 * The Python surface (enhance(), DfNet.__call__, DfStream.process) and the reference C API (df_process_frame: aborts like the
 * reference's panics) do this themselves. */
int dfx_model_poll(const dfx_model *m);
int dfx_model_check(const dfx_model *m);
/* Read-only facts about a model handle (what = DFX_Q_*). */
#define DFX_Q_GRU_PERSISTENT 1 /* 1: big multi-stream passes run the GRU phase as ONE persistent, flag-synchronised launch (default on the GPU) */
#define DFX_Q_HWQ_PROBE 2      /* 1: the streams of that phase were seen to run concurrently (the handshake runs at the first use or at this query); 0: they were not (hardware
                                * queues shared: GPU_MAX_HW_QUEUES too small or HIP initialised before it was set) and the event-synchronised
                                * form is used instead; -1: not probed (no streams, exact fp32, CPU interpreter) */
#define DFX_Q_EXACT_FP32 3     /* 1: DFX_EXACT_FP32=1 was set at creation */
#define DFX_Q_SPIN_LIMIT 4     /* polls a flag wait makes before it gives up (DFX_SYNC_SPIN_LIMIT, default 2^22 ~ 2 s) */
#define DFX_Q_PASSES_PERSISTENT 5   /* big passes of this handle that ran the persistent GRU phase */
#define DFX_Q_PASSES_TICKET_BUSY 6  /* big passes that took the event-synchronised form because another PROCESS held the device's ticket for its own
                                       persistent phase (/dev/shm/dfx_persistent_<PCI bus id>.lock, DFX_DEVICE_TICKET=0: no ticket) */
#define DFX_Q_PASSES_C0_PRESPLIT 7  /* batch passes whose fused DF-encoder kernels read the pre-split copy of feat_spec (default; DFX_C0_PRESPLIT=0: none) */
#define DFX_Q_PASSES_PAIR 9          /* passes whose persistent GRU phase ran its recurrences on pairs of CUs (dfx_k_gru_seq_p2; DFX_GRU_PAIR=0, one 16-clip group, exact fp32: none) */
#define DFX_Q_LAST_PLAN 8           /* what the last pass of this handle (batch or streaming) decided: a mask of DFX_PLAN_* bits, 0 before the first pass */
/* DFX_Q_LAST_PLAN: which fused kernels the pass ran and which form its GRU phase took (decided by the model's shape, the arithmetic mode and the
 * size of the pass; the names are those of DfxPass::plan() in csrc/dfx_model_forward.h).  Diagnostic: the tests use it to see that their shapes
 * reach every form. */
#define DFX_PLAN_FAN (1 << 0)         /* emb and its consumers in one kernel behind the encoder GRU (dfx_k_emb_fan) */
#define DFX_PLAN_FAN_SKP (1 << 1)     /* ... which also writes df_skip(emb) */
#define DFX_PLAN_FUSE_H3 (1 << 2)     /* fp16-split fused DF-encoder kernels (c0 recomputed on the matrix core) */
#define DFX_PLAN_PRESPLIT (1 << 3)    /* ... reading the pre-split copy of feat_spec (counted by DFX_Q_PASSES_C0_PRESPLIT) */
#define DFX_PLAN_FUSE_TAIL (1 << 4)   /* ERB decoder convolutions as one launch (dfx_k_erb_tail) */
#define DFX_PLAN_FUSE_ENC (1 << 5)    /* frame-resident ERB encoder head (dfx_k_erb_enc) */
#define DFX_PLAN_FUSE_ENC4 (1 << 6)   /* the four ERB encoder convolutions as one launch (dfx_k_erb_enc4) */
#define DFX_PLAN_ENC_FAN (1 << 7)     /* df_fc_emb + linear_in as the fan-out kernel (dfx_k_enc_fan) */
#define DFX_PLAN_DFENC (1 << 8)       /* the DF branch of the encoder as one kernel (dfx_k_df_enc_h3) */
#define DFX_PLAN_C0_FUSED (1 << 9)    /* c0 = df_conv0(feat_spec) never stored */
#define DFX_PLAN_PIPE (1 << 10)       /* layer-pipelined GRU phase (time chunks) */
#define DFX_PLAN_USE_SEQ (1 << 11)    /* ... in its persistent form (counted by DFX_Q_PASSES_PERSISTENT) */
#define DFX_PLAN_DF_OUT_SHIFT 12      /* two bits: the form df_out took, DFX_PLAN_DF_OUT_* (0: df_out did not run) */
#define DFX_PLAN_DF_OUT_MASK (3 << DFX_PLAN_DF_OUT_SHIFT)
#define DFX_PLAN_DF_OUT_RESIDENT 1    /* dfx_k_df_out_h3r: weight fragments in registers */
#define DFX_PLAN_DF_OUT_STREAMING 2   /* dfx_k_df_out_h3 */
#define DFX_PLAN_DF_OUT_GGEMM 3       /* the grouped GEMM */
#define DFX_PLAN_ROWS_FINISH (1 << 14) /* deep filter + gains inside the inverse transform (dfx_k_synthesis_rows) */
#define DFX_PLAN_FUSE_DEC (1 << 15)   /* frame-resident last two ERB decoder layers (dfx_k_erb_dec10 / inside dfx_k_erb_tail): set on every pass, every accepted shape */
int dfx_model_query(const dfx_model *m, int what, int64_t *value);

/* Scratch memory the caller must provide (device bytes) for a [B, T-frames] batch.  What a workspace — this one, dfx_enhance's, dfx_enhance_varlen's —
 * holds when a pass starts is irrelevant (no pass reads what it has not written, nothing is carried from pass to pass in it), and what it holds
 * when the pass is through is unspecified. */
int dfx_model_workspace_bytes(const dfx_model *m, int64_t B, int64_t T, int64_t *bytes);

/* DfNet.forward (deepfilternet3.py:389-456).
 *   spec [B,T,F][2], feat_erb [B,T,E], feat_spec [B,T,nb_df][2]  ->
 *   spec_e [B,T,F][2], mask [B,T,E] (may be NULL), lsnr [B,T] (may be NULL), df_coefs [B,O,T,nb_df][2] (may be NULL;
 *   DFX_COEF_BOTF == the reference's DfOutputReshapeMF layout, deepfilternet3.py:268-275)
 *   atten_lim: enhance()'s mix factor (0 = off), applied after the optional post filter. */
int dfx_model_forward(const dfx_model *m, const dfx_bands *bands, const float *spec, const float *feat_erb,
                      const float *feat_spec, int64_t B, int64_t T, float atten_lim, float *spec_e, float *mask,
                      float *lsnr, float *df_coefs, void *workspace, int64_t workspace_bytes, void *stream);

/* enhance() (enhance.py:206-250) end to end on the device: x [B, T] -> y [B, T] (pad=1) or y [B, (T/hop)*hop] (pad=0,
 * delayed by fft-hop like the reference).  atten_lim_db: 0 = off.  workspace from dfx_enhance_workspace_bytes.
 * Asynchronous: the call returns before the pass has run (y is valid once `stream` has caught up).  For passes of >= 16384 frames the
 * engine paces its own enqueue (DFX_ENQUEUE_AHEAD=1: off): the call first waits, on the host, until the previous pass of this handle
 * (dfx_enhance or dfx_model_forward) has drained, and it returns only when the encoder front of its own pass has run and the rest is
 * enqueued — packets queued ahead on the pass's hardware queues slow the kernels that are running (docs/measurements.md §5e).  One pass at a time
 * per handle, as before; use one handle per concurrent caller. */
int dfx_enhance_workspace_bytes(const dfx_model *m, const dfx_state *st, int64_t B, int64_t T, int pad, int64_t *bytes);
int dfx_enhance(const dfx_model *m, const dfx_state *st, const float *x, int64_t B, int64_t T, int pad,
                float atten_lim_db, float *y, void *workspace, int64_t workspace_bytes, void *stream);
/* The same pass from and to 16-bit PCM, the sample format the reference's file loop moves (df/enhance.py:73-89 -> df/io.py:25-57 load_audio:
 * torchaudio's int16 normalisation x / 32768; df/io.py:60-84 save_audio: (audio * (1 << 15)).to(torch.int16), truncation toward zero).  Both
 * conversions run inside the STFT kernel's loads and the ISTFT kernel's stores: half the bytes at the boundary (and over PCIe), no conversion
 * launches, and bit-identical samples to dfx_pcm16_to_f32 -> dfx_enhance -> dfx_f32_to_pcm16.  Same workspace, same asynchrony. */
int dfx_enhance_pcm16(const dfx_model *m, const dfx_state *st, const int16_t *x, int64_t B, int64_t T, int pad,
                      float atten_lim_db, int16_t *y, void *workspace, int64_t workspace_bytes, void *stream);
/* enhance() of B clips of different lengths in one pass: row b of x holds lengths[b] samples (x_stride >= max lengths[b]; what lies behind
 * them is never read); row b of y receives exactly what dfx_enhance(x row b, T = lengths[b]) stores, bit for bit (DFX_EXACT_FP32=1: within
 * that mode's 1e-6 RMS, its kernels' bits depend on the pass's frame count) — out_len_b = lengths[b]
 * (pad) or (lengths[b]/hop)*hop (no pad) samples — then zeros up to max_b out_len_b (y_stride >= that; y is not written behind it).
 * lengths: host memory, read during the call (the caller may reuse it when the call returns).  Every row runs the frames of the longest
 * one — the padded frames of a shorter row still cost their GRU steps —, so pass clips of similar lengths together.  Same asynchrony, pacing,
 * fault reporting and workspace rules as dfx_enhance, with the workspace from dfx_enhance_varlen_workspace_bytes; a faulted pass stores its
 * poison (NaN, 16-bit PCM: zeros) in the out_len_b samples of every row, the zeros behind them stay zeros.  DFX_ERR_INVALID_ARG,
 * before any device work, for a negative length, x_stride < max length, y_stride < max out_len, a workspace too small, or a null buffer
 * (lengths included) when B > 0. */
int dfx_enhance_varlen_workspace_bytes(const dfx_model *m, const dfx_state *st, int64_t B, const int64_t *lengths, int pad, int64_t *bytes);
int dfx_enhance_varlen(const dfx_model *m, const dfx_state *st, const float *x, int64_t B, int64_t x_stride, const int64_t *lengths,
                       int pad, float atten_lim_db, float *y, int64_t y_stride, void *workspace, int64_t workspace_bytes, void *stream);
int dfx_enhance_varlen_pcm16(const dfx_model *m, const dfx_state *st, const int16_t *x, int64_t B, int64_t x_stride, const int64_t *lengths,
                             int pad, float atten_lim_db, int16_t *y, int64_t y_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Streaming: the frame loop of the reference's real-time runtime, libDF/src/tract.rs `DfTract::process` (:509-642), exported by
 * its C API as df_create / df_get_frame_length / df_set_atten_lim / df_set_post_filter_beta / df_process_frame / df_free
 * (libDF/src/capi.rs:83-253), for `streams` independent mono streams advanced in lockstep on one GPU.
 *   dfx_stream_process(x [streams, n*hop]) -> y [streams, n*hop]: n hops per stream and call (1 <= n <= max_frames; n = 1 is
 *   df_process_frame).  All state lives in the handle: STFT/ISTFT memories, the running ERB / unit-norm means, the convolution
 *   input histories, the hidden states of the five GRU layers and the rolling spectra the deep filter reads.
 *   Like the reference the output is delayed by `lookahead` hops (max(conv_lookahead, df_lookahead), dfx_stream_delay_frames)
 *   on top of the fft-hop samples of the STFT: output hop k is the enhanced input hop k - lookahead; the first `lookahead`
 *   output hops are zero (tract.rs: the rolling spectra start as zeros).  Concatenated over calls, the output equals
 *   dfx_enhance(pad=0) of the whole signal delayed by `lookahead` hops — however the signal is cut into calls.
 *   Stage gating (off by default; dfx_stream_set_gating): the reference decides per frame from the encoder's local SNR whether the
 *   ERB decoder (stage 1) and the DF decoder (stage 2) run — `apply_stages`, tract.rs:658-672, thresholds of RuntimeParams
 *   (:160-189, defaults -10 / 30 / 20 dB) — and answers a stream that has been silent (mean square < 1e-7) for more than 5 hops with
 *   zeros and lsnr = -15 without processing it (:513-525).  With gating on every stream takes these decisions on its own, hop by
 *   hop: lsnr < min: zero mask, no DF; lsnr > max_erb: the spectrum passes unchanged; lsnr > max_df: mask only; otherwise mask +
 *   DF.  A decoder that is skipped keeps its state (GRU hidden states, the delay line in front of df_convp), a frozen stream all of
 *   its state, exactly like tract's pulsed sub-models, which only advance when they are run.  A call of n hops is then n passes.
 *   Multi-channel streams (dfx_stream_set_channels; RuntimeParams::n_ch, tract.rs:119-176; df_create itself is mono, capi.rs:83-104):
 *   `channels` consecutive rows are the channels of one stream.  Every channel has its own STFT / feature / network state; the ERB
 *   masks of a stream's channels are reduced to one mask (ReduceMask: 0 none, 1 max, 2 mean = the reference default, :96-118,868-902)
 *   that is applied to all of them; with gating the silent-input test runs over all channels of the hop and the stage decision is
 *   taken from the first channel's local SNR (:468), one decision and one skip counter per stream.
 * lsnr (optional) receives the local SNR estimate [streams, n] in dB (df_process_frame's return value); not meaningful for the
 * warm-up hops.
 *   Slots (dfx_stream_reset_streams): the start-of-stream position is per stream.  A stream that is reset while the others run on
 *   behaves, from the next dfx_stream_process call, like a stream of a freshly created handle with the same settings: `lookahead`
 *   hops of silence, then dfx_enhance(pad=0) of its own signal since the reset, delayed; the other streams do not notice.  While a
 *   reset stream is inside its first `lookahead` hops, a call of several hops is cut by the library into one-hop passes for those
 *   hops and one pass for the rest (the results do not depend on the cut beyond rounding, as for any other cut).
 *   dfx_stream_process_raw has one start for all streams: it refuses (DFX_ERR_UNSUPPORTED) while such a stream is younger than the
 *   window of history + lookahead hops.  A refused call does not advance the handle, so on a handle that is driven through the raw
 *   entry point alone the refusal lasts until dfx_stream_process has carried the handle past that window or dfx_stream_reset has
 *   reset all of it: do not reset single streams of such a handle.
 *   Paused streams (dfx_stream_set_pausable, dfx_stream_process_active): a call on a pausable handle may carry a mask of the streams that
 *   take part; a stream that does not is paused for the n hops of the call.  Nothing of a paused stream moves — STFT memories, running
 *   means, feature and spectrum windows, GRU states, df_convp's delay line, the silent-input counter and stage flags of a gated handle, its
 *   age (dfx_stream_frames) — so its next active hop is processed as if the paused calls had not happened: every caller keeps its own
 *   clock, as with one df_process_frame handle each.  Its rows of x are still read and computed like any row and the results discarded:
 *   they must hold finite, ordinary samples (zeros are fine).  Its rows of y are exact zeros, its lsnr entries NaN (no estimate was made).
 *   With `channels` rows per stream the mask has one entry per stream.  A pause is not silence: a gated handle takes no stage decision for
 *   the stream and its silent-input counter neither rises nor clears.  dfx_stream_reset_streams followed by paused calls is a reserved
 *   slot: the stream starts, `lookahead` silent hops included, with its first active hop.  A paused row still costs its lane in every
 *   kernel.  A pausable handle keeps its state in the per-stream forms of a gated handle from its first hop and runs one hop per pass
 *   (without gating every stage runs on every hop); a handle that is not pausable enqueues exactly what it did before.  The mask is a host
 *   array and travels to the device as kernel arguments (4096 streams per launch): no upload, and the call never waits for the device.
 *   Engine configurations: every model the batch path serves with a fused DF encoder streams, in either arithmetic and with the DF stage on
 *   or off; refused (DFX_ERR_UNSUPPORTED) are conv_lookahead != df_lookahead and df_pathway_kernel_size_t > 5 or df_order > 8.  A handle
 *   on a DFX_EXACT_FP32=1 model runs every contraction in fp32, like that model's batch path, and equals it delayed: a one-hop call steps
 *   each GRU layer in one launch (dfx_k_gru_step_x32), a call of several hops takes the projection + recurrence kernels with the handle's
 *   state.  Exact handles keep the encoder's feature windows in ring form and a gated one the per-stream window of c0 frames in front of
 *   df_convp (the forms of every model without fp16-split fragments; the fp16-split default keeps linear windows and pending sums).
 *   A mask-only model (dfx_model_set_run_df(m, 0), to be set before the handle's first call) never runs stage 2: its DF decoder's state
 *   never moves, gating decides between zeros / pass / mask only, and dfx_stream_process_raw reports gains (stage bit 2) with zero-filled
 *   coefficients and never bit 8.
 *   Per-stream settings (dfx_stream_set_atten_lim_streams, ..._post_filter_beta_streams, ..._thresholds_streams): in the reference the
 *   attenuation limit, the post-filter beta and the thresholds belong to one DfTract, i.e. to one caller (capi.rs:136-156,
 *   tract.rs:160-170); here every stream of a handle can have its own.  With `channels` rows per stream a stream's value holds for all its
 *   rows.  A setter is enqueued on `stream` like dfx_stream_reset_streams and never waits for the device; it takes effect with the next
 *   dfx_stream_process call enqueued behind it, for the frames that call outputs — the moment at which a handle-wide setter called at the
 *   same point takes effect.  Resets (of the handle or of single streams) leave settings alone: a new caller sets its own after the reset;
 *   a paused stream's settings can be changed while it sits out.  The handle-wide setters keep their behaviour: each sets every stream's
 *   value of its setting and makes the handle uniform in it again, and a handle that is uniform in a setting enqueues exactly what a handle
 *   without per-stream settings enqueues.  The undelayed pass-through (|dB| < 0.01) is a handle-wide mode and is reached through
 *   dfx_stream_set_atten_lim only: it returns the input undelayed and leaves the network idle for every stream.  A per-stream |dB| < 0.01
 *   mixes with lim = 0.99999994 instead, as dfx_enhance does: the stream's noisy signal comes back delayed like everybody's output and its
 *   state keeps advancing (a handle in pass-through mode leaves it with the first per-stream limit; its other streams then mix the same
 *   way).  Thresholds set on a handle without gating are stored and take effect once gating is on; a pausable handle that is not gated keeps
 *   running every stage on every hop, and a mask-only model keeps having no DF threshold.  A per-row handle enqueues the same kernels per
 *   hop as a uniform one: the finishing kernel and the stage decision read each row's values from small device arrays.
 *   Clip ends (dfx_stream_process_ends, below): a stream has no end, so "equals dfx_enhance(pad=0) delayed" stops `lookahead` frames short of a
 *   clip's last frame — they only come out when more hops are fed, and the features of fed silence are not the batch path's zero padding.  A
 *   call may say per row how many of its hops are still frames of the row's clip; behind them the row sees that padding, and its output is
 *   dfx_enhance(pad=0) of exactly its own frames, delayed, the last ones included.  With dfx_stream_reset_streams and
 *   dfx_stream_memory_bytes this is what a time-chunked enhance() of clips of any length in bounded memory is built from (enhance_long in the
 *   Python package).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dfx_stream_state dfx_stream_state;
int dfx_stream_create(const dfx_model *m, const dfx_state *st, int64_t streams, int max_frames, dfx_stream_state **out);
void dfx_stream_free(dfx_stream_state *s);
int dfx_stream_reset(dfx_stream_state *s, void *stream);                 /* back to the state after create */
/* Streams ids[0..count) start over as after dfx_stream_create; every other stream is untouched.  ids: HOST array of stream
 * indices in [0, rows / channels) (a multi-channel stream is reset as a whole), duplicates allowed.  Settings (attenuation limit,
 * post-filter beta, thresholds — handle-wide or the stream's own — gating, channels) stay: a new caller sets its own.  Enqueued on `stream`, ordered with dfx_stream_process
 * calls on the same stream; does not wait for the device. */
int dfx_stream_reset_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, void *stream);
/* hops of network time each stream has consumed since its own last reset (host array, [rows / channels]); host bookkeeping, no device access */
int dfx_stream_frames(const dfx_stream_state *s, int64_t *frames_out);
int dfx_stream_frame_length(const dfx_stream_state *s);                  /* hop size in samples (df_get_frame_length), at the caller's rate */
int dfx_stream_delay_frames(const dfx_stream_state *s);                  /* lookahead in hops */
int dfx_stream_set_atten_lim(dfx_stream_state *s, float lim_db);         /* df_set_atten_lim: |dB| >= 100 off, < 0.01 bypass */
/* The handle-wide limit by enhance()'s rule (df/enhance.py:238-240, as dfx_enhance applies it) instead of the runtime's: 0 = no limit, any
 * other value mixes with 10^(-|dB|/20) kept below 1 — no undelayed pass-through below 0.01 dB and no "off" from 100 dB on.  For drivers whose
 * streams are the clips of an enhance() call.  Makes the handle uniform in the setting, like dfx_stream_set_atten_lim.  dfx_stream_get_settings
 * then reports |atten_lim_db| as given (above 100 too: a real limit here) and 100 for 0 = no limit.  The rule belongs to the handle, not to its
 * streams: a stream exported from it carries the |dB| value, and the importing handle applies its own runtime's rule to it (|dB| >= 100: off;
 * < 0.01: lim = 0.99999994). */
int dfx_stream_set_atten_lim_enhance(dfx_stream_state *s, float atten_lim_db);
int dfx_stream_set_post_filter_beta(dfx_stream_state *s, float beta);    /* df_set_post_filter_beta: 0 disables the post filter */
int dfx_stream_set_channels(dfx_stream_state *s, int channels, int reduce_mask); /* rows per stream; 0 none / 1 max / 2 mean */
int dfx_stream_set_gating(dfx_stream_state *s, int enable);              /* DfTract::process's per-frame stage decisions, per stream */
int dfx_stream_set_thresholds(dfx_stream_state *s, float min_db_thresh, float max_db_erb_thresh,
                              float max_db_df_thresh);                   /* RuntimeParams::with_thresholds (tract.rs:160-170) */
/* The same three settings for the streams ids[0..count) alone.  ids: HOST array of stream indices in [0, rows / channels); the values are
 * HOST arrays with one entry (the thresholds: three — min_db, max_db_erb, max_db_df) per id; duplicate ids: the last occurrence wins.
 * count == 0 is a no-op.  A null handle or array, an index out of range, a negative beta or a NaN fail with DFX_ERR_INVALID_ARG and change
 * nothing.  Enqueued on `stream` (ids and values travel as kernel arguments, 192 streams per launch); no wait for the device. */
int dfx_stream_set_atten_lim_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const float *lim_db /*[count]*/,
                                     void *stream);                      /* df_set_atten_lim (capi.rs:136-144, tract.rs:387-398): |dB| >= 100 off, < 0.01 lim = 0.99999994 (delayed, not the bypass) */
int dfx_stream_set_post_filter_beta_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const float *beta /*[count]*/,
                                            void *stream);               /* df_set_post_filter_beta (capi.rs:146-156): 0 disables it for the stream */
int dfx_stream_set_thresholds_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const float *thr /*[count][3]*/,
                                      void *stream);                     /* RuntimeParams::with_thresholds (tract.rs:160-170) */
/* What was set, from the host's copy (no device access): out_host [rows / channels][5] = lim_db (|dB|; 100: off), beta (the model's value
 * where none was set), min_db, max_db_erb, max_db_df  (the reference keeps them in DfTract / RuntimeParams: tract.rs:150-189,387-398) */
int dfx_stream_get_settings(const dfx_stream_state *s, float *out_host);
int dfx_stream_process(dfx_stream_state *s, const float *x, int64_t n_frames, float *y, float *lsnr, void *stream);
/* Accepted only at a reset point (no hop consumed since create / dfx_stream_reset); else DFX_ERR_INVALID_ARG. */
int dfx_stream_set_pausable(dfx_stream_state *s, int enable);
/* dfx_stream_process with a mask: active = HOST array [streams / channels], nonzero = the stream takes part; NULL = all.
 * A mask (non-NULL) on a handle that is not pausable: DFX_ERR_INVALID_ARG. */
int dfx_stream_process_active(dfx_stream_state *s, const float *x, int64_t n_frames, float *y, float *lsnr,
                              const unsigned char *active, void *stream);
/* DfTract::process_raw (tract.rs:441-507) == df_process_frame_raw (capi.rs:172-210) for every stream: one spectral frame
 * spec [streams, F][2] in, the pass's raw ERB gains [streams, nb_erb] and deep-filter coefficients [streams, df_order, nb_df][2] out,
 * stages [streams] saying which of them exist (bit value 2: gains — the network's mask, or zeros below min_db_thresh; 8: coefficients;
 * the reference signals "absent" with NULL pointers).  Gating must be on; no STFT / deep filtering / synthesis happens here. */
int dfx_stream_process_raw(dfx_stream_state *s, const float *spec, float *gains, float *coefs, unsigned char *stages, float *lsnr,
                           void *stream);
/* Streaming at the caller's sample rate.  dfx_stream_set_sample_rate(sr, ...) gives the handle an up-sampler sr -> model rate and a
 * down-sampler model rate -> sr over all rows (dfx_stream_resampler_*, below; the filter parameters are dfx_resampler_create's) and the
 * model-rate staging rows for max_frames hops.  dfx_stream_process / _process_active / _process_pcm16 then take and return hops of
 * h = hop * sr / model_rate samples (dfx_stream_frame_length): x, y [rows, n_frames * h].  h must be a whole number of samples and of
 * up-sampler blocks, i.e. model_rate / gcd(sr, model_rate) must divide the hop: 8, 12, 16, 24, 32, 44.1, 88.2, 96 kHz at 48 kHz / hop
 * 480; 22.05 and 11.025 kHz fail with DFX_ERR_UNSUPPORTED.  Accepted only at a reset point (no hop consumed since create / dfx_stream_reset),
 * else DFX_ERR_INVALID_ARG; sr == the model's rate clears it.  The output equals
 *   up  = resample(cat(zeros(P_u), x), sr, model_rate)[:, : n_total * hop]
 *   ref = resample(cat(zeros(P_d), z), model_rate, sr)[:, : n_total * h],   z = what the model-rate handle makes of `up` under the same calls,
 * so the converters add P_u + P_d * sr / model_rate samples of delay at the caller's rate (dfx_stream_resample_delay; 34 at 16 kHz, 294 at
 * 44.1 kHz with sinc_fast) on top of the STFT's and the lookahead's.  Resets zero the converters' histories (single streams: their rows), a
 * paused stream's rows are inactive in both converters, and in the handle-wide pass-through the caller gets its own samples back unchanged
 * while both converters keep their histories moving.  dfx_stream_process_raw is spectral and knows no rate. */
int dfx_stream_set_sample_rate(dfx_stream_state *s, int sr, int lowpass_filter_width, double rolloff, int method, double beta);
int dfx_stream_sample_rate(const dfx_stream_state *s);                   /* the caller's rate (the model's when none was set) */
int64_t dfx_stream_resample_delay(const dfx_stream_state *s);            /* samples at the caller's rate; 0 without a rate */
/* dfx_stream_process_active on 16-bit PCM: x, y int16 [rows, n_frames * frame_length] (x / 32768 in, dfx_f32_to_pcm16's encoding out).  At a
 * converted rate the conversions happen inside the two converter kernels; at the model's rate through dfx_pcm16_to_f32 / dfx_f32_to_pcm16. */
int dfx_stream_process_pcm16(dfx_stream_state *s, const int16_t *x, int64_t n_frames, int16_t *y, float *lsnr, const unsigned char *active,
                             void *stream);
/* dfx_stream_process_pcm16 for G.711 codes, the bytes of an 8 kHz RTP payload: x, y uint8 [rows, n_frames * frame_length], law =
 * DFX_G711_ULAW or DFX_G711_ALAW (anything else: DFX_ERR_INVALID_ARG); the codec is dfx_g711_decode / dfx_g711_encode's, below.  At a
 * converted rate both conversions happen inside the two converter kernels (one byte per sample over the bus in either direction); at the
 * model's rate through dfx_g711_decode / dfx_g711_encode and the staging rows.  In the handle-wide undelayed pass-through the caller gets
 * its own BYTES back, not a re-encoding (0x7F stays 0x7F); a paused stream's rows come back as the law's silence code (0xFF / 0xD5).  The
 * sample format belongs to the call, not to the stream: it enters neither the snapshot record nor the fingerprint, one handle may be called
 * with float, 16-bit PCM and either law from call to call, and a stream may move between handles fed different formats at the same rate. */
int dfx_stream_process_g711(dfx_stream_state *s, const uint8_t *x, int law, int64_t n_frames, uint8_t *y, float *lsnr,
                            const unsigned char *active, void *stream);
/* Clips that end inside a call.  A stream has no end: the last `lookahead` frames of a clip only come out when more hops are fed, and the
 * features of fed silence are not the zero padding the batch path puts behind a clip (MF.DF's, df/multiframe.py:72-76, and pad_feat's,
 * df/deepfilternet3.py:359,409-410).  dfx_stream_process_ends is dfx_stream_process (x_format DFX_FMT_F32: float x, y) or
 * dfx_stream_process_pcm16 (DFX_FMT_PCM16: int16 x, y; anything else DFX_ERR_INVALID_ARG) with valid_hops: a HOST array [streams], NULL =
 * all n_frames.  valid_hops[b] = v, 0 <= v <= n_frames, says that the first v hops of this call are the last frames of row b's clip; every
 * later hop of the row — the rest of this call and all hops of later calls, whichever entry point makes them — lies behind the clip's end
 * until the row is reset (dfx_stream_reset_streams, dfx_stream_reset, or a stream imported into the slot).  Behind the end the row's spectrum
 * and its normalised ERB and DF features are zero wherever the network and the deep filter read them (rule (2) of dfx_enhance_varlen); the hops
 * are still processed, and they push the clip's last frames out.  The row then yields dfx_enhance(pad=0) of exactly its own frames, delayed
 * by `lookahead` hops, its last frames included; past that its output, lsnr and state are unspecified until the reset.  Feed zeros behind a
 * clip's samples.  A later call must pass 0 for a row that has ended (else DFX_ERR_INVALID_ARG, like a count outside [0, n_frames]; nothing is
 * enqueued).  A call in which no row ends and none has ended enqueues exactly what dfx_stream_process / _pcm16 enqueue and gives the same bits.
 * The counts travel to the device as kernel arguments (512 rows per launch): no upload, no wait.  Exact-fp32 and mask-only models are served;
 * DFX_ERR_UNSUPPORTED, the handle not advanced, on gated or pausable handles, with channels > 1 and at a caller's sample rate.  In the
 * handle-wide undelayed pass-through valid_hops is ignored.  Ends work inside the one-hop passes of a reset row's warm-up too. */
int dfx_stream_process_ends(dfx_stream_state *s, const void *x, int x_format, int64_t n_frames, void *y, float *lsnr,
                            const int64_t *valid_hops, void *stream);
/* Device bytes of a handle of that size without a sample rate: what dfx_stream_create allocates plus the two staging rows
 * [streams, max_frames * hop] the first 16-bit PCM or G.711 call adds.  No device access; refuses what dfx_stream_create refuses. */
int dfx_stream_memory_bytes(const dfx_model *m, const dfx_state *st, int64_t streams, int max_frames, int64_t *bytes);
/* Moving live streams between handles.  In the reference a caller's DfTract is a value the host owns; here a stream's state is its rows of
 * the handle's device arrays, in forms that change with the handle and the moment.  A snapshot of a stream is
 *   payload: one packed record of dfx_stream_snapshot_bytes() bytes in DEVICE memory — every state row of the stream's `channels` rows in a
 *            canonical layout that does not depend on the handle: STFT memories, running means, the three windows oldest frame first, the GRU
 *            rows, df_convp's pending sums in the stream's own order, the per-stream forms of gated / pausable handles, the sample-rate
 *            converters' histories.  Position-independent bytes: copy them to the host, a file, another GPU or process.
 *   meta:    this HOST struct, written by the export without asking the device.
 * The fingerprint covers what decides the record's layout and meaning: the dfx_model_cfg, the dfx_state parameters, channels and mask
 * reduction, gated / pausable / exact fp32 / run_df, the caller's rate with the resampler parameters, and the record size.  WEIGHTS ARE NOT
 * FINGERPRINTED: importing into a handle of a model with the same configuration and other weights is accepted, and continues the stream
 * with that model.  Source and destination may differ in the number of streams, max_frames, hop count and the form their windows are in.
 * Export is a copy (the source stream runs on).  Import overwrites the named streams completely, as dfx_stream_reset_streams does, and
 * leaves every other stream alone; the stream keeps its age (dfx_stream_frames), so its birth in the destination may lie before the
 * handle's own start.  with_settings != 0: the stream's limit, beta and thresholds arrive too (as by dfx_stream_set_*_streams); 0: the
 * destination slot keeps its own.  For H + L hops after an import a non-pausable destination runs the forms of a handle with a reset
 * stream; past them the steady call enqueues what it did before.  An import ends the reset point of the handle (dfx_stream_set_pausable,
 * dfx_stream_set_sample_rate).  Both calls are enqueued on `stream`: ids and ages travel as kernel arguments, 192 streams per launch,
 * nothing is uploaded and nothing waits; the payload must stay valid until the work on `stream` has passed it.
 * Refused with no state changed (DFX_ERR_INVALID_ARG / DFX_ERR_UNSUPPORTED; dfx_last_error names the first mismatch): null pointers, ids out
 * of range, duplicate destination ids, a magic, version or fingerprint mismatch, and — the one excluded mode — a handle in the handle-wide
 * undelayed pass-through (dfx_stream_set_atten_lim |dB| < 0.01), for both calls. */
#define DFX_STREAM_META_MAGIC 0x53584644u /* "DFXS" */
#define DFX_STREAM_META_VERSION 1u
typedef struct dfx_stream_meta {
    uint32_t magic, version;
    uint64_t fingerprint;
    int64_t age;             /* hops of network time the stream has consumed (dfx_stream_frames) */
    float settings[5];       /* as dfx_stream_get_settings reports them: |lim dB|, beta, min_db, max_db_erb, max_db_df */
    int32_t pending_current; /* the ungated pending sums in the record are current (0: the destination rebuilds them) */
} dfx_stream_meta;
int dfx_stream_snapshot_bytes(const dfx_stream_state *s, int64_t *bytes_per_stream);
int dfx_stream_export_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, void *payload_dev /*[count][bytes_per_stream]*/,
                              dfx_stream_meta *meta_host /*[count]*/, void *stream);
int dfx_stream_import_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const void *payload_dev,
                              const dfx_stream_meta *meta_host, int with_settings, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-frame Wiener / MVDR filters: df.multiframe.MfWf.forward (multiframe.py:282-321) and MfMvdr.forward (:373-413), the filter
 * stage of the reference's DeepFilterNetMF model (deepfilternetmf.py:335-352).  op 0 = MfWf, 1 = MfMvdr; frame_size N <= 8.
 *   spec [B,T,F][2], ifc [B,T,nb,N][2] (speech inter-frame correlation), mat [B,T,nb,N,N][2] (row-major; an inverse correlation
 *   matrix, a correlation matrix, or a Cholesky factor of either: cholesky_decomp / inverse exactly as the module's constructor
 *   flags, enforce_constraints / eps / dload likewise, defaults 1 / 1e-8 / 1e-7)  ->  out [B,T,F][2] (out != spec; bins >= nb are
 *   copied).  Y[t,f] = sum_n w[n] X[t + n - (N-1-lookahead), f], zero outside the clip (MultiFrameModule.pad :72-76).
 * ---------------------------------------------------------------------------------------------------------------- */
int dfx_mf_filter(const float *spec, const float *ifc, const float *mat, int op, int frame_size, int lookahead, int cholesky_decomp,
                  int inverse, int enforce_constraints, float eps, float dload, int64_t B, int64_t T, int F, int nb, float *out,
                  void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Either side of enhance() in the reference's file loop (df/enhance.py:73-89: load_audio -> enhance -> resample back -> save_audio):
 *   dfx_pcm16_to_f32   torchaudio.load's normalisation of 16-bit PCM, x / 32768 (df/io.py:48)
 *   dfx_f32_to_pcm16   save_audio's encoding, (audio * (1 << 15)).to(int16) (df/io.py:79-80): truncation toward zero, wrap-around
 *   dfx_resample       df.io.resample (io.py:114-116) == torchaudio.functional.resample(audio, orig_sr, new_sr, **params): polyphase
 *                      windowed-sinc bank, method 0 = "sinc_interp_hann", 1 = "sinc_interp_kaiser" (beta); io.py:92-111 parameter sets:
 *                      sinc_fast (0, width 16, rolloff 0.99) | sinc_best (0, 64, 0.99) | kaiser_fast (1, 16, 0.85, beta 8.555504641634386)
 *                      | kaiser_best (1, 16, 0.9475937167399596, 14.769656459379492).  x [B, T] (row stride x_stride) ->
 *                      y [B, dfx_resampler_out_len(T)] (row stride y_stride), device pointers.
 *   dfx_resampler_kernel   the filter bank itself (host arithmetic, no device): W [phases][taps] float32.
 *   dfx_g711_decode / dfx_g711_encode   G.711 codes (uint8, law = DFX_G711_ULAW | DFX_G711_ALAW) <-> float32 or int16, what
 *                      torchaudio.load(normalize=True) / libsndfile make of a mu-law / A-law WAVE file.  Closed forms, no table:
 *     decode to a 16-bit linear value s (float: s / 32768)
 *       mu-law: u = ~c & 0xFF;  t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);  s = (u & 0x80) ? 132 - t : t - 132          range +-32124
 *       A-law:  a = c ^ 0x55, e = (a >> 4) & 7, m = a & 15;  t = e == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (e - 1);
 *               s = (a & 0x80) ? t : -t                                                                                     range +-32256
 *     encode a 16-bit linear value s: sign-magnitude, as G.711 defines it (the codes of s and -s differ in the sign bit only, s = 1 .. 32767;
 *     |-32768| = 32768 is taken care of by the min)
 *       mu-law: m = min(|s|, 32635) + 132;  e = msb(m) - 7;  c = ~((s < 0 ? 0x80 : 0) | e << 4 | ((m >> (e + 3)) & 15)) & 0xFF
 *       A-law:  m = min(|s|, 32767) >> 3;  e = m < 32 ? 0 : msb(m) - 4;  mant = e == 0 ? (m >> 1) & 15 : (m >> e) & 15;
 *               c = ((s < 0 ? 0 : 0x80) | e << 4 | mant) ^ 0x55
 *     float -> code: s = trunc(clamp(x * 32768, -32768, 32767)), NaN -> 0, then encode.  This rule SATURATES; dfx_f32_to_pcm16 wraps like
 *     save_audio's cast and is unchanged.  Silence is 0xFF (mu-law) / 0xD5 (A-law); encode(decode(c)) == c for every code but mu-law's
 *     0x7F (negative zero), which gives 0xFF.
 *     codes / out (encode) may start at any byte address and n may be anything up to 2^40: 16 codes per lane as one 16-byte access between a
 *     single-code head and tail.  out (decode) / x (encode): float32, or int16 when the _is_pcm16 argument is non-zero.  n == 0: DFX_OK;
 *     another law, or a null buffer with n > 0: DFX_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------------------------------- */
int dfx_pcm16_to_f32(const int16_t *pcm, int64_t n, float *out, void *stream);
int dfx_f32_to_pcm16(const float *x, int64_t n, int16_t *out, void *stream);
int dfx_g711_decode(const uint8_t *codes, int law, int64_t n, void *out, int out_is_pcm16, void *stream);
int dfx_g711_encode(const void *x, int x_is_pcm16, int law, int64_t n, uint8_t *out, void *stream);
/* Native FLAC -> planar PCM, the bytes of .flac files decoded on the device (the reference loads them through torchaudio.load, df/io.py:25-57).
 * Read: native FLAC streams of 1 to 8 channels and 8 to 24 bits per sample, fixed or variable blocking, every subframe kind, behind an optional
 * ID3v2 tag.  Refused: Ogg-FLAC, 32-bit streams; nothing here writes FLAC.
 *   probe    HOST arithmetic, no device: the first bytes of a stream (through its last metadata block) -> STREAMINFO and the byte offset of the
 *            first frame.  DFX_ERR_INVALID_ARG: no 'fLaC' marker (Ogg-FLAC's 'OggS' is named), no STREAMINFO, more than 8 channels, bit depths
 *            outside 8 .. 24, metadata that does not end inside the n bytes given.
 *   decode   blob: DEVICE buffer (16-byte aligned) holding the bytes of n_streams streams; stream i lies at offsets[i] (a multiple of 16) with
 *            lengths[i] bytes (2^28 at most), and the buffer extends to the end of the 16-byte chunk of every stream's last byte.  offsets,
 *            lengths, infos (dfx_flac_probe's results) and out_offsets are HOST arrays, not read after the return.  Stream i's samples go to
 *            out + out_offsets[i] (BYTES, a multiple of 4) as a planar [channels, total_samples] block: int16 where the stream has at most
 *            16 bits (sample << (16 - bits): exactly what a 16-bit WAVE of the same audio holds), float32 = sample / 2^(bits - 1) otherwise (the
 *            scaling of a 24-bit WAVE).  The whole of out (out_bytes) is cleared first.  status: DEVICE int64 [n_streams][4]: frames decoded,
 *            frames lost, samples written per channel, flags (bit 0: more sync-code look-alikes than the candidate list holds).
 *            A frame counts only if it starts where the previous frame ended and its CRC-16 holds: the sync code appearing inside a frame's
 *            payload, even followed by a header with a valid CRC-8, does not split it.  A frame whose CRC-16 fails, that runs out of bytes or
 *            uses a reserved code leaves zeros for its block and counts as lost; decoding goes on at the next frame whose CRC-16 holds, at
 *            the sample position its header states.  Corrupt input never faults: every read is bounded by the stream's length.
 *            Asynchronous on `stream`; workspace (device, 16-byte aligned): dfx_flac_workspace_bytes. */
typedef struct dfx_flac_info {
    int32_t sample_rate, channels, bits_per_sample, min_block, max_block;
    int32_t first_frame;   /* byte offset of the first frame */
    int64_t total_samples; /* per channel; 0 = not stated */
    uint8_t md5[16];       /* of the interleaved little-endian samples; all zero = not computed */
} dfx_flac_info;
int dfx_flac_probe(const uint8_t *head, int64_t n, dfx_flac_info *out);
int dfx_flac_workspace_bytes(int64_t n_streams, const int64_t *lengths, const dfx_flac_info *infos, int64_t *bytes);
int dfx_flac_decode(const uint8_t *blob, int64_t blob_bytes, int64_t n_streams, const int64_t *offsets, const int64_t *lengths,
                    const dfx_flac_info *infos, const int64_t *out_offsets, void *out, int64_t out_bytes, int64_t *status, void *workspace,
                    int64_t workspace_bytes, void *stream);
typedef struct dfx_resampler dfx_resampler;
int dfx_resampler_create(int orig_sr, int new_sr, int lowpass_filter_width, double rolloff, int method, double beta,
                         dfx_resampler **out);
void dfx_resampler_free(dfx_resampler *r);
int64_t dfx_resampler_out_len(const dfx_resampler *r, int64_t in_len);   /* ceil(new_sr * in_len / orig_sr) */
int dfx_resampler_kernel(int orig_sr, int new_sr, int lowpass_filter_width, double rolloff, int method, double beta, int *phases,
                         int *taps, int *width, float *w_host /* may be NULL */, int64_t cap_floats);
int dfx_resample(const dfx_resampler *r, const float *x, int64_t B, int64_t T, int64_t x_stride, float *y, int64_t y_stride,
                 void *stream);
/* The resampler in step form: per-row state carried across calls.  A call takes in_len = m * block samples per row (block = orig_sr /
 * gcd, the input samples of one frame; in_len a multiple of it and <= max_in_samples, else DFX_ERR_INVALID_ARG) and writes m * new_sr / gcd.
 * Whatever the cut into calls, a row's concatenated output equals dfx_resample applied to P zeros followed by the row's signal, cut to
 * whole frames: P = ceil(width / block) * block input samples of delay = D = P * new_sr / orig_sr output samples (dfx_stream_resampler_delay);
 * bit-identical between cuts.  x / y, each in its own format (DFX_FMT_*, anything else: DFX_ERR_INVALID_ARG): float32, int16 PCM
 * (x / 32768 in, dfx_f32_to_pcm16's encoding out) or G.711 codes (dfx_g711_decode's value / 32768 in, dfx_g711_encode's saturating
 * float -> code rule out), converted inside the kernel's loads and stores; row strides in samples.
 * active_host: HOST array [rows], zero = the row sits the call out (zeros out — as codes: the law's silence —, its state does not move); NULL = all rows.  reset: rows = HOST
 * array of row indices, NULL = every row.  The handle refers to `r`, which must outlive it.  All calls are enqueued on `stream`. */
typedef struct dfx_stream_resampler dfx_stream_resampler;
int dfx_stream_resampler_create(const dfx_resampler *r, int64_t rows, int64_t max_in_samples, dfx_stream_resampler **out);
void dfx_stream_resampler_free(dfx_stream_resampler *h);
int dfx_stream_resampler_reset(dfx_stream_resampler *h, const int64_t *rows /* NULL = all */, int64_t count, void *stream);
int dfx_stream_resampler_delay(const dfx_stream_resampler *h, int64_t *in_samples, int64_t *out_samples);
int dfx_stream_resampler_process(dfx_stream_resampler *h, const void *x, int x_format, int64_t in_len, int64_t x_stride, void *y,
                                 int y_format, int64_t y_stride, const unsigned char *active_host /* NULL = all */, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Scoring on the device: what the reference computes per clip on a CPU process pool (df/evaluation_utils.py SiSDRMetric / StoiMetric,
 * evaluation_loop_dir_only) and pins its released models with (df/scripts/test_df.py:18-21,44-78).
 *   dfx_si_sdr   si_sdr_speechmetrics (evaluation_utils.py:599-619) of every row, in two passes like the reference: rss = ref . ref and ref . est,
 *                a = (eps + ref . est) / (rss + eps), then sum (a ref)^2 and sum (est - a ref)^2; out[b] = 10 log10((eps + sss) / (eps + snn)) dB,
 *                eps = float32's.  Float32 products and differences as numpy forms them on float32 input, float64 sums.
 *   dfx_stoi     df.stoi.stoi (stoi.py:163-231) of every row: both signals to 10 kHz (r: a dfx_resampler fs_source -> 10000, the reference's
 *                df.io.resample default set is sinc_fast; NULL: the rows are at 10 kHz already), remove_silent_frames (stoi.py:35-110), the
 *                512-point STFT (:146-160), thirdoct(10000, 512, 15, 150) (:113-143), the 30-frame normalised, clipped correlations (:206-230).
 * ref / est / clean / degraded: DEVICE float32 [B, stride]; lengths_host: HOST int64 [B], row b has lengths_host[b] <= stride samples (not read
 * after the return: the counts travel as kernel arguments); out: DEVICE float32 [B].  A row's result is that of the row alone —
 * stoi(clean[b : b + 1, : lengths[b]], ...) —: the same bits whatever the batch around it, the padding behind it and the workspace's contents
 * (the reference pads a batch to one length, which moves its pad_front; that is not copied).  Rows the reference skips (fewer than 512 samples
 * left after silent-frame removal, stoi.py:195-197, where it leaves out[i] uninitialised) give NaN.  info: NULL, or DEVICE int32 [B][4]: windows
 * examined, windows kept, STFT frames L, segments J (L = J = 0 for a skipped row).  The workspace (DEVICE, 16-byte aligned, the *_workspace_bytes
 * of the same arguments; host arithmetic) is the caller's; the calls only enqueue on `stream`: no copy to the host, no wait, no float atomics.
 * DFX_ERR_INVALID_ARG: a length outside [0, stride], a workspace that is too small, a resampler to another rate than 10 kHz.
 * ---------------------------------------------------------------------------------------------------------------- */
int dfx_si_sdr_workspace_bytes(int64_t B, const int64_t *lengths_host, int64_t *bytes);
int dfx_si_sdr(const float *ref, const float *est, int64_t B, int64_t stride, const int64_t *lengths_host, float *out, void *workspace,
               int64_t workspace_bytes, void *stream);
int dfx_stoi_workspace_bytes(int fs_source, int64_t B, const int64_t *lengths_host, int64_t *bytes);
int dfx_stoi(const dfx_resampler *r, const float *clean, const float *degraded, int64_t B, int64_t stride, const int64_t *lengths_host,
             float *out, int32_t *info, void *workspace, int64_t workspace_bytes, void *stream);

/* The composite measures' parts (df/sepm.py; evaluation_utils.py's third default metric, "composite", without PESQ, which the reference takes
 * from the third-party pesq package):
 *   dfx_sepm     of every row, at 16 kHz (r: a dfx_resampler fs_source -> 16000, the reference's sinc_fast, evaluation_utils.py:32,583-584, every
 *                row with its own length; NULL: the rows are at 16 kHz already), in float64 as sepm.py computes them:
 *                  out[b][0]  SNRseg    (sepm.py:28-51)    mean over the frames of 10 log10(sum c^2 / (sum (c - p)^2 + eps) + eps) in [-10, 35]
 *                  out[b][1]  llr       (sepm.py:200-277)  lags 0..16, Levinson with max(E, eps), a and R rounded to float32, the two quadratic
 *                                                          forms IN FLOAT64 (the reference: float32, in its BLAS's order; 2e-8 .. 3e-7 apart
 *                                                          for noise-like clips, up to 4e-3 for strongly tonal ones, where the float32 value is
 *                                                          the inexact one), frac <= 0 -> 1000, log; mean of the K smallest
 *                  out[b][2]  wss       (sepm.py:280-487)  25 critical bands of the 1024-point spectrum, -100 dB clip, findLocPeaks; mean of the
 *                                                          K smallest
 *                  out[b][3]  fwSNRseg  (sepm.py:54-182)   mean over the frames, each in [-10, 35]
 *                480-sample frames at hop 120: a row of n samples at 16 kHz has F = (n - 480) / 120 of them, K = round_half_even(0.95 F) (host,
 *                double).  F < 1 (n < 600), where the reference raises or averages nothing: all four NaN.  info: NULL, or DEVICE int32 [B][2]: F, K.
 * clean / processed, lengths_host, the workspace, the stream and the row-alone guarantee: as dfx_stoi; out: DEVICE float64 [B][4].
 * DFX_ERR_INVALID_ARG: null pointers, a length outside [0, stride], a workspace that is too small, a resampler to another rate than 16 kHz. */
int dfx_sepm_workspace_bytes(int fs_source, int64_t B, const int64_t *lengths_host, int64_t *bytes);
int dfx_sepm(const dfx_resampler *r, const float *clean, const float *processed, int64_t B, int64_t stride, const int64_t *lengths_host,
             double *out /* [B, 4]: ssnr, llr, wss, fwsnr */, int32_t *info /* [B, 2] or NULL: F, K */, void *workspace, int64_t workspace_bytes,
             void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-kernel timing (measurement aid, no reference counterpart; the reference only logs wall-clock RTF,
 * DeepFilterNet/df/enhance.py:77-87).  When a kernel's bit is set in `kernel_mask`, every launch of it is bracketed by
 * two hipEvents recorded on the stream the kernel is launched on.  dfx_prof_read() synchronises the pending events and
 * returns the accumulated device time and launch count since the last reset.  Mask 0 (default) = no events at all.
 * ---------------------------------------------------------------------------------------------------------------- */
int dfx_prof_kernel_count(void);
const char *dfx_prof_kernel_name(int kernel_id);
int dfx_prof_enable(uint32_t kernel_mask);
int dfx_prof_reset(void);
int dfx_prof_read(int kernel_id, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* DFX_H */
