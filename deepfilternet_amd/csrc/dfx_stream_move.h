// dfx: streams that move between handles (dfx_stream_export_streams / dfx_stream_import_streams).
// A part of dfx_model.hip (included behind dfx_model_stream.h).
//
// A stream's state is its rows of about 20 device arrays whose form depends on the handle and on the moment: ring or linear windows, two
// parities, pending sums whose slot follows the handle's hop count.  The record is the same state in one canonical, handle-independent
// layout, one record per row (a stream of `channels` rows: that many records, consecutive):
//   STFT memories (analysis, synthesis) | running means (erb, unit) | the three windows, oldest frame first (H, H, H + L frames) | the GRU
//   rows of all layers | df_convp's pending sums, kt - 1 slots in the stream's own order (slot j: the output of the j-th hop from now) |
//   per-stream forms of gated / pausable handles (flags, silent-input counter and its shadow, shadow means and GRU rows, the pending sums
//   twice with parity and count, or the window of c0 frames) | the histories of both sample-rate converters
// Every entry starts at a multiple of 16 bytes.  Which entries a record has follows from the model, the DF state and the kind of the handle
// alone (stream_layout_fingerprint), never from the number of streams, max_frames or the hop count.
#pragma once

// DfxRowClear with the place of every entry inside a row's record: entry e, repetition r <-> record bytes [off[e] + r * bytes[e], + bytes[e]).
// An entry without an array (p == null: pending sums on a handle too large to keep them) is exported as zeros and not imported.  Entries are in
// rising offset order and do not overlap.
struct DfxRowTable : DfxRowClear {
    int64_t off[DFX_ROWS_MAX_ENTRIES];
    bool add_at(int64_t off_, void *ptr, int64_t stride_, int64_t bytes_, int reps_ = 1, int64_t rep_stride_ = 0) {
        if (bytes_ <= 0) return true;
        if (n >= DFX_ROWS_MAX_ENTRIES) return false;
        off[n] = off_;
        p[n] = static_cast<unsigned char *>(ptr), stride[n] = stride_, bytes[n] = bytes_, reps[n] = reps_, rep_stride[n] = rep_stride_;
        ++n;
        return true;
    }
};
// Ids and the births the imported rows take travel as kernel arguments, like DfxRowIds (no upload, no wait).  With the table (32 entries of
// 44 bytes) the argument block is 1416 + 8 + 192 * 12 + 32 = 3760 bytes, inside the 4 KB a launch can carry.
#define DFX_MOVE_IDS 192
#define DFX_MOVE_PARTS 8   /* workgroups that share one row (grid.y) */
struct DfxMoveIds {
    int n;
    int id[DFX_MOVE_IDS];
    int64_t birth[DFX_MOVE_IDS];
};

// One 16-byte unit of a row's record, at record offset o: the entry that covers it is found by a scan over the table (uniform loads, selects:
// no per-lane index into the kernel arguments), then the unit's place in the state arrays.  A unit inside one repetition of an entry whose
// array side is 16-byte aligned moves as one float4 (spectra, feature windows, GRU rows, pending sums, STFT memories); every other unit —
// counters, flags, parities, the padding behind an entry — goes byte by byte.
struct DfxMoveUnit {
    unsigned char *p;      // the unit's first byte in the state array (null: the entry has no array, or the unit is all padding)
    int64_t bytes, rep_stride, rel, total;   // of the entry: bytes per repetition, array bytes between repetitions; the unit's offset inside the entry's record bytes, those bytes
    unsigned char *base;   // the entry's repetition 0 of this row
    bool fast;
};
static __device__ __forceinline__ DfxMoveUnit dfx_move_locate(const DfxRowTable &R, int64_t row, int64_t o) {
    // (every field is selected in the scan: reading them from the argument block at the lane's own index afterwards measured 45 % slower)
    unsigned char *p0 = nullptr;
    int64_t stride = 0, nb = 1, rs = 0, off = 0;
    int reps = 0;
    for (int e = 0; e < R.n; ++e)
        if (o >= R.off[e]) p0 = R.p[e], stride = R.stride[e], nb = R.bytes[e], rs = R.rep_stride[e], reps = R.reps[e], off = R.off[e];
    DfxMoveUnit u;
    u.bytes = nb, u.rep_stride = rs, u.rel = o - off, u.total = nb * reps;
    u.base = p0 ? p0 + row * stride : nullptr;
    const unsigned r = (unsigned)u.rel / (unsigned)nb, w = (unsigned)u.rel - r * (unsigned)nb;   // (a record is far below 2^32 bytes: 32-bit division)
    u.p = u.base && u.rel < u.total ? u.base + (int64_t)r * rs + w : nullptr;
    u.fast = u.p && (int64_t)w + 16 <= nb && (((uintptr_t)u.p) & 15) == 0;
    return u;
}

// Workgroups (k * ch + c, part): channel c of stream I.id[k] <-> record k * ch + c of `payload` (row_bytes each, a multiple of 16).  The
// record's 16-byte units are dealt out to the threads of the row's workgroups, four units in flight per thread: every thread's loads are
// issued before its first store, and no thread waits for an entry it has no share of.  IMPORT: the state arrays are written from the record
// and birth[row] = I.birth[k]; else the record is written from the state arrays (padding and entries without an array: zeros).  The host has
// refused duplicate destination ids, so no two workgroup columns write one row; an export may name a stream twice (two records).
template <bool IMPORT>
__global__ void __launch_bounds__(256) dfx_k_stream_move_rows(DfxRowTable R, DfxMoveIds I, int ch, unsigned char *payload, int64_t row_bytes, int64_t *birth) {
    const int k = (int)blockIdx.x / ch;
    if (k >= I.n) return;
    const int64_t row = (int64_t)I.id[k] * ch + (int)blockIdx.x % ch;
    unsigned char *rec = payload + (int64_t)blockIdx.x * row_bytes;
    const bool rec16 = (((uintptr_t)rec) & 15) == 0;
    const int64_t units = row_bytes >> 4, i0 = (int64_t)blockIdx.y * blockDim.x + threadIdx.x, step = (int64_t)gridDim.y * blockDim.x;
    for (int64_t i = i0; i < units; i += 4 * step) {
        float4 v[4];
        float4 *dst[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dst[j] = nullptr;
            const int64_t o = (i + j * step) << 4;
            if (o >= row_bytes) continue;
            const DfxMoveUnit u = dfx_move_locate(R, row, o);
            unsigned char *q = rec + o;
            if (u.fast && rec16) {
                v[j] = *reinterpret_cast<const float4 *>(IMPORT ? q : u.p);
                dst[j] = reinterpret_cast<float4 *>(IMPORT ? u.p : q);
                continue;
            }
            for (int t = 0; t < 16; ++t) {   // the unit's bytes one by one (they may lie in two repetitions; behind the entry's last byte: padding)
                const int64_t rel = u.rel + t;
                unsigned char *a = nullptr;
                if (u.base && rel < u.total) a = u.base + (int64_t)((unsigned)rel / (unsigned)u.bytes) * u.rep_stride + (unsigned)rel % (unsigned)u.bytes;
                if (IMPORT) {
                    if (a) *a = q[t];
                } else {
                    q[t] = a ? *a : (unsigned char)0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (dst[j]) *dst[j] = v[j];
    }
    if (IMPORT && blockIdx.y == 0 && threadIdx.x == 0) birth[row] = I.birth[k];
}

// every row's birth moves with the handle's hop count (stream_import_rebase)
__global__ void dfx_k_stream_birth_shift(int64_t *birth, int64_t B, int64_t d) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) birth[b] += d;
}

// ---- the canonical record -----------------------------------------------------------------------------------------------------------------
static inline int64_t stream_move_pad16(int64_t v) { return (v + 15) & ~(int64_t)15; }
// does the record carry per-stream forms / pending sums (a property of the kind of handle, not of its size)
static inline bool stream_move_has_gate(const dfx_stream_state *S) { return (S->gated || S->pausable) && S->gate_buf; }
static inline bool stream_move_has_pend(const dfx_stream_state *S) {
    const dfx_model_cfg &c = S->m->cfg;
    return c.df_pathway_kernel_size_t >= 2 && c.conv_ch % 32 == 0 && !S->m->exact_fp32;
}

// The table of a handle's state arrays against the record: every array in whichever form holds the state now, entries in rising record
// offset (dfx_move_locate scans them in order).  The GRU rows and the converters' histories move to and from the buffer that is current: the
// other one is written in full by the next pass before anything reads it.  Returns the bytes of one row's record in *row_bytes (R may be
// null: the size alone).
static int stream_move_rows(const dfx_stream_state *S, DfxRowTable *R, int64_t *row_bytes) {
    const dfx_model_cfg &c = S->m->cfg;
    const int64_t B = S->B, H = S->H, Hs = S->H + S->L, E = c.nb_erb, Fd = c.nb_df, ML = S->st->N - S->st->hop, Fp = S->Fp;
    int64_t off = 0;
    bool ok = true;
    if (R) R->n = 0;
    auto add = [&](unsigned char *p, int64_t stride, int64_t bytes, int reps = 1, int64_t rep_stride = 0) {
        if (bytes <= 0) return;
        if (R) ok = R->add_at(off, p, stride, bytes, reps, rep_stride) && ok;
        off += stream_move_pad16(bytes * reps);
    };
    const int f = S->flip;
    add(S->buf + S->ana_mem[f], ML * 4, ML * 4);
    add(S->buf + S->syn_mem[f], ML * 4, ML * 4);
    add(S->buf + S->erb_state, E * 4, E * 4);
    add(S->buf + S->unit_state, Fd * 4, Fd * 4);
    if (S->feat_owns) {
        add(S->buf + S->fe_lin + S->lin_pos * E * 4, S->feat_cap * E * 4, H * E * 4);
        add(S->buf + S->fs_lin + S->lin_pos * Fd * 8, S->feat_cap * Fd * 8, H * Fd * 8);
    } else {
        add(S->buf + S->hist_fe[f], H * E * 4, H * E * 4);
        add(S->buf + S->hist_fs[f], H * Fd * 8, H * Fd * 8);
    }
    if (S->lin_owns) add(S->buf + S->spec_lin + S->lin_pos * Fp * 8, S->lin_cap * Fp * 8, Hs * Fp * 8);
    else add(S->buf + S->hist_spec[f], Hs * Fp * 8, Hs * Fp * 8);
    add(reinterpret_cast<unsigned char *>(stream_h(S)), 1024, 1024, S->layers, B * 1024);
    if (stream_move_has_pend(S)) {   // slot j of the record = the sum of the j-th output from now: the handle's slot (frames - L + j) mod (kt - 1)
        const int ns = c.df_pathway_kernel_size_t - 1;
        const int64_t rb = (int64_t)stream_c0ring_row_bytes(c), sb = rb / ns;
        const int slot0 = (int)((((S->frames - S->L) % ns) + ns) % ns);
        for (int j = 0; j < ns; ++j) add(S->c0ring_bytes ? S->buf + S->c0ring + (size_t)((slot0 + j) % ns) * sb : nullptr, rb, sb);
    }
    if (stream_move_has_gate(S)) {
        unsigned char *g = S->gate_buf;
        add(g + S->g_flags, 1, 1);
        add(g + S->g_counter, 4, 4);
        add(g + S->g_sh_counter, 4, 4);
        add(g + S->g_sh_erb, E * 4, E * 4);
        add(g + S->g_sh_unit, Fd * 4, Fd * 4);
        add(g + S->g_sh_h, 1024, 1024, S->layers, B * 1024);
        if (S->g_pend2_ok) {
            add(g + S->g_pend2, (int64_t)stream_pend2_row_bytes(c), (int64_t)stream_pend2_row_bytes(c));
            add(g + S->g_par, 1, 1);
            add(g + S->g_cnt, 4, 4);
        } else if (c.df_pathway_kernel_size_t > 1) {
            const int64_t wb = (int64_t)(S->H + 1) * c.nb_df * c.conv_ch * 4;
            add(g + S->g_c0_win, wb, wb);
        }
    }
    if (S->sr) {
        dfx_stream_resampler *rs[2] = {S->up, S->dn};
        for (int i = 0; i < 2; ++i) {
            float *cur = nullptr, *other = nullptr;
            int hist = 0;
            dfx_stream_resampler_rows(rs[i], &cur, &other, &hist);
            add(reinterpret_cast<unsigned char *>(cur), (int64_t)hist * 4, (int64_t)hist * 4);
        }
    }
    if (!ok) DFX_FAIL(DFX_ERR_UNSUPPORTED, "stream export / import: more state arrays than DFX_ROWS_MAX_ENTRIES");
    *row_bytes = off;
    return DFX_OK;
}

// 64-bit FNV-1a over everything that decides the record's layout and meaning: the model configuration, the DF state's parameters, channels
// and mask reduction, the kind of handle (gated, pausable, exact fp32, DF stage on), the caller's rate with the converters' parameters, and
// the record size.  Weights are not part of it.
static uint64_t stream_layout_fingerprint(const dfx_stream_state *S, int64_t bytes_per_stream) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    auto mix_i = [&](int64_t v) { mix(&v, sizeof v); };
    auto mix_d = [&](double v) { mix(&v, sizeof v); };
    mix(&S->m->cfg, sizeof(dfx_model_cfg));   // (int32 / float fields only: no padding)
    const dfx_state *st = S->st;
    mix_i(st->sr), mix_i(st->N), mix_i(st->hop), mix_i(st->nb), mix_i(st->min_nb);
    mix_i(S->channels), mix_i(S->reduce_mask);
    mix_i(S->gated), mix_i(S->pausable), mix_i(S->m->exact_fp32), mix_i(S->m->run_df);
    mix_i(S->sr);
    if (S->sr) mix_i(S->rs_width), mix_d(S->rs_rolloff), mix_i(S->rs_method), mix_d(S->rs_beta);
    mix_i(bytes_per_stream);
    return h;
}

extern "C" int dfx_stream_snapshot_bytes(const dfx_stream_state *s, int64_t *bytes_per_stream) {
    if (!s || !bytes_per_stream) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_stream_snapshot_bytes: null argument");
    int64_t rb = 0;
    if (int rc = stream_move_rows(s, nullptr, &rb)) return rc;
    *bytes_per_stream = rb * s->channels;
    return DFX_OK;
}

// what both directions check before anything is enqueued
static int stream_move_check(const dfx_stream_state *s, const char *who, const int64_t *ids, int64_t count, const void *payload, const void *meta, bool unique) {
    if (!s || count < 0 || (count > 0 && (!ids || !payload || !meta))) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: null handle, id list, payload or meta", who);
    if (s->lim == 1.f)
        DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: the handle is in the undelayed pass-through (dfx_stream_set_atten_lim with |dB| < 0.01), the one mode in which streams do not move", who);
    const int64_t ns = s->B / s->channels;
    for (int64_t i = 0; i < count; ++i)
        if (ids[i] < 0 || ids[i] >= ns) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: stream index %lld is not in [0, %lld)", who, (long long)ids[i], (long long)ns);
    if (unique) {
        std::vector<unsigned char> seen((size_t)ns, 0);
        for (int64_t i = 0; i < count; ++i) {
            if (seen[(size_t)ids[i]]) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: stream index %lld is named twice", who, (long long)ids[i]);
            seen[(size_t)ids[i]] = 1;
        }
    }
    return DFX_OK;
}

template <bool IMPORT>
static int stream_move_launch(dfx_stream_state *s, const DfxRowTable &R, int64_t row_bytes, const int64_t *ids, const int64_t *births, int64_t count,
                              unsigned char *payload, hipStream_t hs) {
    const int ch = s->channels;
    for (int64_t i0 = 0; i0 < count; i0 += DFX_MOVE_IDS) {
        DfxMoveIds I;
        I.n = (int)(count - i0 < DFX_MOVE_IDS ? count - i0 : DFX_MOVE_IDS);
        for (int i = 0; i < I.n; ++i) I.id[i] = (int)ids[i0 + i], I.birth[i] = births ? births[i0 + i] : 0;
        dfx_launch(dfx_k_stream_move_rows<IMPORT>, dim3((unsigned)(I.n * ch), DFX_MOVE_PARTS), dim3(256), 0, hs, R, I, ch, payload + i0 * ch * row_bytes, row_bytes,
                   reinterpret_cast<int64_t *>(s->buf + s->birth_dev));
        DFX_LAUNCH_CHECK();
    }
    return DFX_OK;
}

extern "C" int dfx_stream_export_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, void *payload_dev, dfx_stream_meta *meta_host, void *stream) {
    if (int rc = stream_move_check(s, "dfx_stream_export_streams", ids, count, payload_dev, meta_host, false)) return rc;
    if (count == 0) return DFX_OK;
    if (int rc = dfx_require_device()) return rc;
    DfxRowTable R;
    int64_t rb = 0;
    if (int rc = stream_move_rows(s, &R, &rb)) return rc;
    const int ch = s->channels;
    const uint64_t fp = stream_layout_fingerprint(s, rb * ch);
    if (int rc = stream_move_launch<false>(s, R, rb, ids, nullptr, count, static_cast<unsigned char *>(payload_dev), dfx_stream(stream))) return rc;
    const bool pend_current = stream_move_has_pend(s) && s->c0ring_bytes && s->c0ring_ok;
    for (int64_t i = 0; i < count; ++i) {
        dfx_stream_meta &M = meta_host[i];
        memset(&M, 0, sizeof M);
        const size_t r = (size_t)(ids[i] * ch);
        M.magic = DFX_STREAM_META_MAGIC, M.version = DFX_STREAM_META_VERSION;
        M.fingerprint = fp;
        M.age = s->frames - s->birth[r];
        M.settings[0] = s->row_lim_db[r], M.settings[1] = s->row_beta[r];
        for (int j = 0; j < 3; ++j) M.settings[2 + j] = s->row_thr[r * 3 + j];
        M.pending_current = pend_current;
    }
    return DFX_OK;
}

// A handle whose own start is still inside the window (hop count < H + L) treats every row alike: zero features for the first L hops, one
// t_zero for all.  A stream that arrives with an age of its own does not fit that, so the handle's hop count moves on by a multiple of
// kt - 1 (the pending sums keep their phase) that is at least the window, and every row's birth moves with it: all ages stay, and the rows
// that are young are now young per stream, the way a stream reset on a running handle is.
static int stream_import_rebase(dfx_stream_state *s, hipStream_t hs) {
    const int64_t Hs = s->H + s->L;
    if (s->frames >= Hs) return DFX_OK;
    const int64_t ns = s->m->cfg.df_pathway_kernel_size_t > 1 ? s->m->cfg.df_pathway_kernel_size_t - 1 : 1;
    const int64_t d = dfx_ceil_div(Hs, ns) * ns;
    dfx_launch(dfx_k_stream_birth_shift, dim3((unsigned)dfx_ceil_div(s->B, 256)), dim3(256), 0, hs, reinterpret_cast<int64_t *>(s->buf + s->birth_dev), s->B, d);
    DFX_LAUNCH_CHECK();
    for (auto &b : s->birth) b += d;
    const int64_t old = s->frames;
    s->frames += d;
    s->mixed_until = s->frames + Hs;
    if (old < s->L) s->warm_until = s->frames + s->L;
    else if (s->warm_until > old) s->warm_until += d;
    return DFX_OK;
}

extern "C" int dfx_stream_import_streams(dfx_stream_state *s, const int64_t *ids, int64_t count, const void *payload_dev, const dfx_stream_meta *meta_host,
                                         int with_settings, void *stream) {
    const char *who = "dfx_stream_import_streams";
    if (int rc = stream_move_check(s, who, ids, count, payload_dev, meta_host, true)) return rc;
    if (count == 0) return DFX_OK;
    int64_t rb = 0;
    if (int rc = stream_move_rows(s, nullptr, &rb)) return rc;
    const int ch = s->channels;
    const uint64_t fp = stream_layout_fingerprint(s, rb * ch);
    bool pend_current = true;
    for (int64_t i = 0; i < count; ++i) {
        const dfx_stream_meta &M = meta_host[i];
        if (M.magic != DFX_STREAM_META_MAGIC) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: entry %lld is not a stream snapshot (magic %08x)", who, (long long)i, (unsigned)M.magic);
        if (M.version != DFX_STREAM_META_VERSION)
            DFX_FAIL(DFX_ERR_UNSUPPORTED, "%s: entry %lld has snapshot format version %u, this library reads version %u", who, (long long)i, (unsigned)M.version,
                     (unsigned)DFX_STREAM_META_VERSION);
        if (M.fingerprint != fp)
            DFX_FAIL(DFX_ERR_INVALID_ARG,
                     "%s: entry %lld comes from another kind of handle (layout fingerprint %016llx, this handle's %016llx: model configuration, DF state, channels, "
                     "gating, pausable, arithmetic, DF stage, sample rate and record size must agree)",
                     who, (long long)i, (unsigned long long)M.fingerprint, (unsigned long long)fp);
        if (M.age < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: entry %lld has a negative age", who, (long long)i);
        if (with_settings) {
            for (int j = 0; j < 5; ++j)
                if (std::isnan(M.settings[j])) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: setting %d of entry %lld is NaN", who, j, (long long)i);
            if (M.settings[1] < 0.f) DFX_FAIL(DFX_ERR_INVALID_ARG, "%s: beta of entry %lld is negative", who, (long long)i);
        }
        pend_current = pend_current && M.pending_current;
    }
    if (int rc = dfx_require_device()) return rc;
    hipStream_t hs = dfx_stream(stream);
    if (int rc = stream_import_rebase(s, hs)) return rc;
    DfxRowTable R;   // (behind the rebase: the pending sums' phase is the new hop count's)
    if (int rc = stream_move_rows(s, &R, &rb)) return rc;
    std::vector<int64_t> births((size_t)count);
    bool young = false;
    for (int64_t i = 0; i < count; ++i) {
        births[(size_t)i] = s->frames - meta_host[i].age;   // (negative where the stream is older than the handle)
        young = young || meta_host[i].age < s->L;
    }
    if (int rc = stream_move_launch<true>(s, R, rb, ids, births.data(), count, const_cast<unsigned char *>(static_cast<const unsigned char *>(payload_dev)), hs)) return rc;
    for (int64_t i = 0; i < count; ++i)
        for (int k = 0; k < ch; ++k) {
            const size_t r = (size_t)(ids[i] * ch + k);
            s->birth[r] = births[(size_t)i];
            s->n_ended -= s->ended[r], s->ended[r] = 0;   // (a slot that is overwritten holds a live stream again)
        }
    // the rows no longer share one start: the per-row t_zero for the next window of hops, one hop per pass while a stream is in warm-up
    if (s->mixed_until < s->frames + s->H + s->L) s->mixed_until = s->frames + s->H + s->L;
    if (young && s->warm_until < s->frames + s->L) s->warm_until = s->frames + s->L;
    if (!pend_current) s->c0ring_ok = false;   // stale at the source: the next one-hop pass rebuilds the sums from the feature windows
    s->fresh = false;
    if (with_settings) {
        std::vector<float> v((size_t)count * 3);
        for (int64_t i = 0; i < count; ++i) v[(size_t)i] = meta_host[i].settings[0];
        if (int rc = stream_set_rows<1>(s, who, 0, ids, count, v.data(), stream)) return rc;
        for (int64_t i = 0; i < count; ++i) v[(size_t)i] = meta_host[i].settings[1];
        if (int rc = stream_set_rows<1>(s, who, 1, ids, count, v.data(), stream)) return rc;
        for (int64_t i = 0; i < count; ++i)
            for (int j = 0; j < 3; ++j) v[(size_t)i * 3 + j] = meta_host[i].settings[2 + j];
        if (int rc = stream_set_rows<3>(s, who, 2, ids, count, v.data(), stream)) return rc;
    }
    return DFX_OK;
}
