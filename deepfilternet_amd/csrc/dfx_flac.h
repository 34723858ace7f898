// dfx: native FLAC (the bytes of .flac files, as they are) -> planar PCM on the device.  A part of dfx_io.hip; include/dfx.h states the contract.
//
// FLAC frames are independent and self-delimiting, the entropy code inside a subframe is sequential and subframes are not byte-aligned: the
// parallelism is across frames and channels.  Four kernels per dfx_flac_decode call, every stream of the batch in each of them (grid.y = stream):
//   dfx_k_flac_scan     one wave per stream walks its bytes 1024 at a time (one 16-byte load per lane), tests every byte position for the sync
//                       code 0xFF 0xF8/0xF9, validates the header there (reserved codes, agreement with STREAMINFO, CRC-8) and appends the
//                       survivors to the stream's candidate list IN POSITION ORDER (ballot + prefix count: no atomics, a deterministic list)
//   dfx_k_flac_measure  one lane per candidate parses the frame without reconstructing samples: where every subframe starts (bit offsets), where the
//                       frame ends, whether its CRC-16 holds.  A chance sync pair with a chance CRC-8 becomes a candidate and dies here.
//   dfx_k_flac_walk     one lane per stream links the chain: a frame counts only if it starts where the previous one ended and its CRC-16
//                       holds.  It assigns sample positions (cumulative; after a lost frame re-anchored by the next good header's coded number)
//                       and writes the status row.  Candidates inside an accepted frame (the adversarial case) are stepped over.
//   dfx_k_flac_decode   one lane per (accepted frame, channel): Rice / LPC reconstruction in lock step over the sample index, 32 samples per
//                       lane into an LDS tile, then the wave decorrelates the stereo pairs and stores the tile as 64-byte runs.
// Lane per subframe, not wave per frame: a wave per frame leaves 63 lanes idle through the entropy decode.  The decode kernel stages each lane's
// bit stream through an LDS ring filled at the tile boundary (dfx_bits_topup: one batch of loads, one wait); the measure kernel still reloads its
// 16-byte buffer from memory where it runs dry (docs/measurements.md, "Loading FLAC": what that costs).
// The bit reader holds a 64-bit MSB-first window refilled from a 16-byte register buffer or from the ring (aligned 16-byte loads; the unary run is one
// count-leading-zeros on the window); LPC history and coefficients live in LDS ([32][64], lane-contiguous: conflict-free), so nothing is indexed
// dynamically in registers and no kernel uses scratch.
// Every read is bounded: the blob is 16-byte aligned, every stream starts at a multiple of 16 and the blob extends to the 16-byte chunk its last
// byte lies in (checked on the host); a reader past its stream's length returns zeros and raises `over`, which invalidates the candidate.
#pragma once

#define DFX_FLAC_MAX_LEN (1 << 28)   // bytes per stream: bit positions fit 32 bits
#define DFX_FLAC_DESC_CHUNK 32       // stream descriptors per upload launch (kernel arguments, like dfx_launch_varlen_rows)
#define DFX_FLAC_TILE 32             // samples per lane between two flushes

struct alignas(16) DfxFlacQ {
    unsigned a, b, c, d;
};

struct DfxFlacStream {   // 64 bytes
    int64_t off;         // byte offset in the blob (multiple of 16)
    int64_t total;       // samples per channel (STREAMINFO)
    int64_t out_off;     // byte offset of the stream's [C, T] block in the output
    int32_t len, first, channels, bps, min_block, max_block;
    int32_t cand_base, cand_cap;
    int32_t pad_[2];
};

#define DFX_FLAC_F_PARSED 1u   // the frame's structure was read to its end inside the stream, no reserved code
#define DFX_FLAC_F_CRC 2u      // ... and its CRC-16 holds
struct DfxFlacCand {     // 80 bytes
    uint32_t pos, end;   // byte offsets in the stream: first byte of the sync code, first byte behind the CRC-16
    int32_t bs, hdr_len, assign, flags;
    int64_t number;      // the coded number: frame index (fixed blocking) or first sample (variable): bit 62 set = variable
    int64_t samp;        // the walk's verdict: first sample of the frame in the stream, -1 = not part of the chain
    uint32_t sub[8];     // bit offset of every subframe, from the frame's first byte
};

struct DfxFlacDescArgs {
    DfxFlacStream *dst;
    int n;
    DfxFlacStream s[DFX_FLAC_DESC_CHUNK];
};
__global__ void dfx_k_flac_desc(DfxFlacDescArgs A) {
    if ((int)threadIdx.x < A.n) A.dst[threadIdx.x] = A.s[threadIdx.x];
}

// ---- bit reader -----------------------------------------------------------------------------------------------------------------------------------
struct DfxBits {
    const DfxFlacQ *q;     // the stream's first 16-byte chunk
    int nchunk;            // chunks that hold bytes of the stream
    int chunk;             // next chunk to load
    DfxFlacQ buf;
    int wi;                // next word of buf
    unsigned *ring;        // decode kernel: the lane's column of the LDS ring ([64 word slots][64 lanes]) that dfx_bits_topup fills; else null
    int next_w, filled_w;  // ring form: next word of the stream to hand out; the ring holds the words in front of filled_w (a multiple of 4)
    uint64_t win;          // MSB first; the top `have` bits are valid, the rest zero
    int have;
    uint32_t pos, limit;   // bit position in the stream, its length in bits
    bool over;
};
static __device__ __forceinline__ void dfx_bits_load(DfxBits &r) {
    if (r.chunk < r.nchunk)
        r.buf = r.q[r.chunk];
    else
        r.buf.a = r.buf.b = r.buf.c = r.buf.d = 0u;
    ++r.chunk;
}
static __device__ __forceinline__ uint32_t dfx_bits_word(DfxBits &r) {
    if (r.ring) {
        unsigned w = 0u;
        if (r.next_w < r.filled_w)
            w = r.ring[(r.next_w & 63) * 64];
        else if ((r.next_w >> 2) < r.nchunk)   // ran ahead of the ring (more than ~57 bits per sample over a tile): a load of its own
            w = reinterpret_cast<const unsigned *>(r.q)[r.next_w];
        ++r.next_w;
        return __builtin_bswap32(w);
    }
    const unsigned w = r.wi == 0 ? r.buf.a : (r.wi == 1 ? r.buf.b : (r.wi == 2 ? r.buf.c : r.buf.d));
    if (++r.wi == 4) {
        r.wi = 0;
        dfx_bits_load(r);
    }
    return __builtin_bswap32(w);
}
static __device__ __forceinline__ void dfx_bits_refill(DfxBits &r) {
    if (r.have <= 32) {
        r.win |= (uint64_t)dfx_bits_word(r) << (32 - r.have);
        r.have += 32;
    }
}
static __device__ __forceinline__ uint32_t dfx_bits_get(DfxBits &r, int n) {   // 0 <= n <= 32
    dfx_bits_refill(r);
    const uint32_t v = n ? (uint32_t)(r.win >> (64 - n)) : 0u;
    r.win = n == 32 ? r.win << 32 : r.win << (n & 31);
    r.have -= n;
    r.pos += (uint32_t)n;
    r.over |= r.pos > r.limit;
    return v;
}
static __device__ __forceinline__ int32_t dfx_bits_sget(DfxBits &r, int n) {   // two's complement, 1 <= n <= 32
    const uint32_t v = dfx_bits_get(r, n);
    return n >= 32 ? (int32_t)v : (int32_t)(v ^ (1u << (n - 1))) - (int32_t)(1u << (n - 1));
}
static __device__ __forceinline__ uint32_t dfx_bits_unary(DfxBits &r) {   // zeros before the next one bit, which is consumed too
    uint32_t q = 0;
    for (;;) {
        dfx_bits_refill(r);
        if (r.win) {
            const int z = __builtin_clzll(r.win);
            r.win = (r.win << z) << 1;
            r.have -= z + 1;
            r.pos += (uint32_t)z + 1u;
            q += (uint32_t)z;
            r.over |= r.pos > r.limit;
            return q;
        }
        q += (uint32_t)r.have;
        r.pos += (uint32_t)r.have;
        r.have = 0;
        if (r.pos >= r.limit) {
            r.over = true;
            return q;
        }
    }
}
// Ring form, called where every lane of the wave is in step (the kernel's start, every tile boundary): the lane's next 15 chunks at most, up to 60
// words past its position, go into its ring column as one batch of loads with one wait — the refills between two calls then read LDS.
static __device__ __forceinline__ void dfx_bits_topup(DfxBits &r) {
    const int base = r.next_w & ~3, to = base + 60;   // slots of words >= base are never overwritten: to - base <= 64
    const int from = r.filled_w > base ? r.filled_w : base;
    DfxFlacQ v[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        const int w = from + 4 * i;
        if (w < to && (w >> 2) < r.nchunk)
            v[i] = r.q[w >> 2];
        else
            v[i].a = v[i].b = v[i].c = v[i].d = 0u;
    }
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        const int w = from + 4 * i;
        if (w < to) {
            r.ring[((w + 0) & 63) * 64] = v[i].a;
            r.ring[((w + 1) & 63) * 64] = v[i].b;
            r.ring[((w + 2) & 63) * 64] = v[i].c;
            r.ring[((w + 3) & 63) * 64] = v[i].d;
        }
    }
    if (to > r.filled_w) r.filled_w = to;
}
static __device__ __forceinline__ void dfx_bits_open(DfxBits &r, const uint8_t *blob, const DfxFlacStream &S, uint32_t bit, unsigned *ring = nullptr) {
    r.q = reinterpret_cast<const DfxFlacQ *>(blob + S.off);
    r.nchunk = (S.len + 15) >> 4;
    r.limit = (uint32_t)S.len * 8u;
    const uint32_t byte = bit >> 3;
    r.ring = ring;
    r.next_w = (int)(byte >> 2), r.filled_w = 0;
    r.chunk = (int)(byte >> 4);
    if (ring) {
        r.buf.a = r.buf.b = r.buf.c = r.buf.d = 0u;
        dfx_bits_topup(r);
    } else {
        dfx_bits_load(r);
    }
    r.wi = (int)((byte >> 2) & 3u);
    r.win = 0, r.have = 0, r.over = false;
    r.pos = (byte & ~3u) * 8u;
    (void)dfx_bits_get(r, (int)(bit - r.pos));   // < 32
}

// ---- frame header at byte p of a stream (byte loads, each bounded by the stream's length): false = no frame can start here ------------------------
static __device__ bool dfx_flac_header(const uint8_t *s, const DfxFlacStream &S, uint32_t p, DfxFlacCand &c) {
    const uint32_t len = (uint32_t)S.len;
    if (p + 6u > len) return false;   // sync, two code bytes, one number byte, CRC-8 at least
    if (s[p] != 0xFFu || (s[p + 1] & 0xFEu) != 0xF8u) return false;
    const unsigned b2 = s[p + 2], b3 = s[p + 3];
    const unsigned bsc = b2 >> 4, src = b2 & 15u, asg = b3 >> 4, ssc = (b3 >> 1) & 7u;
    if (bsc == 0u || src == 15u || asg > 10u || ssc == 3u || ssc == 7u || (b3 & 1u)) return false;
    if (asg < 8u ? (int)asg + 1 != S.channels : S.channels != 2) return false;
    const int bps = ssc == 0u ? S.bps : (ssc == 1u ? 8 : (ssc == 2u ? 12 : (ssc == 4u ? 16 : (ssc == 5u ? 20 : 24))));
    if (bps != S.bps) return false;
    uint32_t at = p + 4u;
    const unsigned b0 = s[at++];
    int extra = 0;
    uint64_t num = b0;
    if (b0 & 0x80u) {
        int ones = 0;
        while (ones < 8 && (b0 & (0x80u >> ones))) ++ones;
        if (ones < 2 || ones > 7) return false;
        extra = ones - 1;
        num = b0 & (0x7Fu >> ones);
    }
    if (at + (uint32_t)extra >= len) return false;
    for (int i = 0; i < extra; ++i) {
        const unsigned cb = s[at++];
        if ((cb & 0xC0u) != 0x80u) return false;
        num = (num << 6) | (cb & 0x3Fu);
    }
    const int nbs = bsc == 6u ? 1 : (bsc == 7u ? 2 : 0), nsr = src == 12u ? 1 : (src >= 13u ? 2 : 0);
    if (at + (uint32_t)(nbs + nsr) >= len) return false;   // (the CRC-8 byte behind them lies inside the stream)
    int bs;
    if (bsc == 1u)
        bs = 192;
    else if (bsc <= 5u)
        bs = 576 << (bsc - 2u);
    else if (bsc == 6u)
        bs = (int)s[at] + 1;
    else if (bsc == 7u)
        bs = (((int)s[at] << 8) | (int)s[at + 1]) + 1;
    else
        bs = 256 << (bsc - 8u);
    at += (uint32_t)(nbs + nsr);
    if (bs > S.max_block) return false;
    unsigned crc = 0;
    for (uint32_t i = p; i < at; ++i) {
        crc ^= s[i];
        for (int k = 0; k < 8; ++k) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xFFu : (crc << 1) & 0xFFu;
    }
    if (crc != s[at]) return false;
    c.pos = p, c.end = 0;
    c.bs = bs, c.hdr_len = (int)(at + 1u - p), c.assign = (int)asg, c.flags = 0;
    c.number = (int64_t)num | ((s[p + 1] & 1u) ? (int64_t)1 << 62 : 0);
    c.samp = -1;
    return true;
}

// One wave per stream.  Lane l of an iteration owns the 16 byte positions [base + 16 l, base + 16 l + 16) and needs the byte behind them: the next
// lane's first byte (a shuffle), for lane 63 a byte load.
__global__ void __launch_bounds__(64) dfx_k_flac_scan(const uint8_t *__restrict__ blob, const DfxFlacStream *__restrict__ streams,
                                                      DfxFlacCand *__restrict__ cands, int *__restrict__ cand_n, int *__restrict__ cand_lost) {
    const DfxFlacStream S = streams[blockIdx.y];
    const uint8_t *s = blob + S.off;
    const DfxFlacQ *q = reinterpret_cast<const DfxFlacQ *>(s);
    const int lane = (int)threadIdx.x, nchunk = (S.len + 15) >> 4;
    DfxFlacCand *list = cands + S.cand_base;
    int count = 0, lost = 0;   // wave-uniform
    for (int c0 = S.first >> 4; c0 < nchunk; c0 += 64) {
        const int ch = c0 + lane;
        DfxFlacQ v;
        if (ch < nchunk)
            v = q[ch];
        else
            v.a = v.b = v.c = v.d = 0u;
        unsigned nxt = __shfl(v.a, lane + 1) & 0xFFu;
        if (lane == 63) nxt = (ch + 1 < nchunk) ? (unsigned)s[(int64_t)(ch + 1) * 16] : 0u;
        // bytes j and j + 1 of the 17: a position is a suspect when they read FF, F8/F9
        unsigned suspects = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned w = j < 4 ? v.a : (j < 8 ? v.b : (j < 12 ? v.c : v.d));
            const unsigned b = (w >> (8 * (j & 3))) & 0xFFu;
            const unsigned wn = j + 1 < 4 ? v.a : (j + 1 < 8 ? v.b : (j + 1 < 12 ? v.c : v.d));
            const unsigned bn = j == 15 ? nxt : (wn >> (8 * ((j + 1) & 3))) & 0xFFu;
            if (b == 0xFFu && (bn & 0xFEu) == 0xF8u) suspects |= 1u << j;
        }
        if (__ballot(suspects != 0u) == 0ull) continue;
        // the survivors of this lane, then their place in the list: lanes in order, positions in order inside a lane
        unsigned keep = 0;
        for (int j = 0; j < 16; ++j) {
            if (!(suspects & (1u << j))) continue;
            const uint32_t p = (uint32_t)ch * 16u + (uint32_t)j;
            DfxFlacCand c;
            if (p >= (uint32_t)S.first && dfx_flac_header(s, S, p, c)) keep |= 1u << j;
        }
        const int mine = __builtin_popcount(keep);
        int before = 0, all = 0;
        for (int l = 0; l < 64; ++l) {
            const int m = __shfl(mine, l);
            before += l < lane ? m : 0;
            all += m;
        }
        int slot = count + before;
        for (int j = 0; j < 16; ++j) {
            if (!(keep & (1u << j))) continue;
            DfxFlacCand c;
            (void)dfx_flac_header(s, S, (uint32_t)ch * 16u + (uint32_t)j, c);
            for (int k = 0; k < 8; ++k) c.sub[k] = 0u;
            if (slot < S.cand_cap) list[slot] = c;
            ++slot;
        }
        count += all;
        if (count > S.cand_cap) lost = 1, count = S.cand_cap;
    }
    if (lane == 0) cand_n[blockIdx.y] = count, cand_lost[blockIdx.y] = lost;
}

// ---- subframe header: type, wasted bits, order; for LPC the precision and shift are left in the stream -----------------------------------------------
#define DFX_FLAC_CONST 0
#define DFX_FLAC_VERBATIM 1
#define DFX_FLAC_FIXED 2
#define DFX_FLAC_LPC 3
struct DfxFlacSub {
    int kind, order, wasted, ebps;   // ebps: bits per sample as coded (the side channel's extra bit added, the wasted bits taken off)
};
static __device__ __forceinline__ bool dfx_flac_sub_head(DfxBits &r, int bps, int assign, int ch, DfxFlacSub &u) {
    const uint32_t h = dfx_bits_get(r, 8);
    if (h & 0x80u) return false;
    const unsigned type = (h >> 1) & 63u;
    u.wasted = 0;
    if (h & 1u) u.wasted = (int)dfx_bits_unary(r) + 1;
    const bool side = (assign == 8 && ch == 1) || (assign == 9 && ch == 0) || (assign == 10 && ch == 1);
    u.ebps = bps + (side ? 1 : 0) - u.wasted;
    if (u.ebps < 1 || u.ebps > 32) return false;
    if (type == 0u)
        u.kind = DFX_FLAC_CONST, u.order = 0;
    else if (type == 1u)
        u.kind = DFX_FLAC_VERBATIM, u.order = 0;
    else if (type >= 8u && type <= 12u)
        u.kind = DFX_FLAC_FIXED, u.order = (int)type - 8;
    else if (type >= 32u)
        u.kind = DFX_FLAC_LPC, u.order = (int)type - 31;
    else
        return false;
    return true;
}

__global__ void __launch_bounds__(64) dfx_k_flac_measure(const uint8_t *__restrict__ blob, const DfxFlacStream *__restrict__ streams,
                                                         DfxFlacCand *__restrict__ cands, const int *__restrict__ cand_n) {
    __shared__ unsigned short tab[256];   // CRC-16, polynomial 0x8005, MSB first
    for (int i = (int)threadIdx.x; i < 256; i += 64) {
        unsigned c = (unsigned)i << 8;
        for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
        tab[i] = (unsigned short)c;
    }
    __syncthreads();
    const DfxFlacStream S = streams[blockIdx.y];
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= cand_n[blockIdx.y]) return;
    DfxFlacCand *cp = cands + S.cand_base + i;
    const uint32_t pos = cp->pos;
    const int bs = cp->bs, assign = cp->assign;
    DfxBits r;
    dfx_bits_open(r, blob, S, (pos + (uint32_t)cp->hdr_len) * 8u);
    bool ok = true;
    for (int ch = 0; ch < S.channels && ok && !r.over; ++ch) {
        cp->sub[ch] = r.pos - pos * 8u;
        DfxFlacSub u;
        ok = dfx_flac_sub_head(r, S.bps, assign, ch, u);
        if (!ok) break;
        if (u.kind == DFX_FLAC_CONST) {
            (void)dfx_bits_get(r, u.ebps);
            continue;
        }
        if (u.kind == DFX_FLAC_VERBATIM) {
            for (int n = 0; n < bs && !r.over; ++n) (void)dfx_bits_get(r, u.ebps);
            continue;
        }
        if (u.order > bs) {
            ok = false;
            break;
        }
        for (int n = 0; n < u.order; ++n) (void)dfx_bits_get(r, u.ebps);
        if (u.kind == DFX_FLAC_LPC) {
            const int prec = (int)dfx_bits_get(r, 4) + 1;
            const int shift = dfx_bits_sget(r, 5);
            if (prec == 16 || shift < 0) {
                ok = false;
                break;
            }
            for (int n = 0; n < u.order; ++n) (void)dfx_bits_get(r, prec);
        }
        const unsigned method = dfx_bits_get(r, 2);
        if (method > 1u) {
            ok = false;
            break;
        }
        const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
        const int po = (int)dfx_bits_get(r, 4);
        const int psize = bs >> po;
        if ((psize << po) != bs || psize < u.order) {
            ok = false;
            break;
        }
        for (int part = 0; part < (1 << po) && !r.over; ++part) {
            const int cnt = psize - (part == 0 ? u.order : 0);
            const int k = (int)dfx_bits_get(r, pbits);
            if (k == esc) {
                const int w = (int)dfx_bits_get(r, 5);
                for (int n = 0; n < cnt && !r.over; ++n) (void)dfx_bits_get(r, w);
            } else {
                for (int n = 0; n < cnt && !r.over; ++n) {
                    (void)dfx_bits_unary(r);
                    (void)dfx_bits_get(r, k);
                }
            }
        }
    }
    unsigned flags = 0;
    uint32_t end = 0;
    if (ok && !r.over) {
        (void)dfx_bits_get(r, (int)((8u - (r.pos & 7u)) & 7u));
        const uint32_t body_end = r.pos >> 3;
        const uint32_t want = dfx_bits_get(r, 16);
        if (!r.over) {
            end = body_end + 2u;
            flags = DFX_FLAC_F_PARSED;
            DfxBits c;
            dfx_bits_open(c, blob, S, pos * 8u);
            unsigned crc = 0;
            uint32_t left = body_end - pos;
            for (; left >= 4u; left -= 4u) {
                const uint32_t w = dfx_bits_get(c, 32);
                crc = ((crc << 8) & 0xFFFFu) ^ tab[((crc >> 8) ^ (w >> 24)) & 0xFFu];
                crc = ((crc << 8) & 0xFFFFu) ^ tab[((crc >> 8) ^ (w >> 16)) & 0xFFu];
                crc = ((crc << 8) & 0xFFFFu) ^ tab[((crc >> 8) ^ (w >> 8)) & 0xFFu];
                crc = ((crc << 8) & 0xFFFFu) ^ tab[((crc >> 8) ^ w) & 0xFFu];
            }
            for (; left > 0u; --left) crc = ((crc << 8) & 0xFFFFu) ^ tab[((crc >> 8) ^ dfx_bits_get(c, 8)) & 0xFFu];
            if (crc == want) flags |= DFX_FLAC_F_CRC;
        }
    }
    cp->end = end;
    cp->flags = (int)flags;
}

// status row of a stream: frames decoded, frames lost (CRC-16 failed, cut short, or no frame where one had to start), samples written per channel,
// flags (bit 0: the candidate list overflowed — more sync-code look-alikes with a valid CRC-8 than chance explains; the stream counts as damaged)
__global__ void dfx_k_flac_walk(const DfxFlacStream *__restrict__ streams, DfxFlacCand *__restrict__ cands, const int *__restrict__ cand_n,
                                const int *__restrict__ cand_lost, int n_streams, int64_t *__restrict__ status) {
    const int sid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (sid >= n_streams) return;
    const DfxFlacStream S = streams[sid];
    DfxFlacCand *list = cands + S.cand_base;
    const int n = cand_n[sid];
    uint32_t cur = (uint32_t)S.first;
    int64_t samp = 0, good = 0, bad = 0, written = 0;
    int i = 0;
    while (i < n) {
        const uint32_t p = list[i].pos;
        if (p < cur) {   // inside a frame that counted: a look-alike
            ++i;
            continue;
        }
        const int fl = list[i].flags;
        if (p == cur && (fl & (int)DFX_FLAC_F_CRC)) {
            const int64_t room = S.total - samp;
            const int64_t take = room < list[i].bs ? (room > 0 ? room : 0) : list[i].bs;
            list[i].samp = take > 0 ? samp : -1;
            written += take;
            samp += list[i].bs;
            cur = list[i].end;
            ++good, ++i;
            continue;
        }
        // the frame that had to start at cur is lost: its block (where its header survived) stays zeros; go on at the next frame whose CRC-16
        // holds and take the sample position its header states, if that lies ahead
        ++bad;
        if (p == cur) samp += list[i].bs, ++i;
        while (i < n && !(list[i].flags & (int)DFX_FLAC_F_CRC)) ++i;
        if (i >= n) break;
        const int64_t num = list[i].number & (((int64_t)1 << 62) - 1);
        const int64_t at = (list[i].number >> 62) ? num : num * S.max_block;
        if (at > samp) samp = at;
        cur = list[i].pos;
    }
    if (i >= n && bad == 0 && written < S.total) ++bad;   // the chain ended before the stream's samples did
    status[4 * sid + 0] = good;
    status[4 * sid + 1] = bad;
    status[4 * sid + 2] = written;
    status[4 * sid + 3] = cand_lost[sid] ? 1 : 0;
}

// One lane per (candidate, channel) of a stream, t = candidate * channels + channel: the two subframes of a stereo frame sit in neighbouring
// lanes of one wave (64 is even), which is all the decorrelation needs.  Every lane of the block runs the same sample loop (bound: the stream's
// largest block, rounded up to the tile); a lane without an accepted frame, or behind its frame's last sample, idles through it.
__global__ void __launch_bounds__(64) dfx_k_flac_decode(const uint8_t *__restrict__ blob, const DfxFlacStream *__restrict__ streams,
                                                        const DfxFlacCand *__restrict__ cands, const int *__restrict__ cand_n,
                                                        uint8_t *__restrict__ out) {
    __shared__ int hist[32][64];
    __shared__ int coef[32][64];
    __shared__ int tile[64][DFX_FLAC_TILE + 1];
    __shared__ int64_t rbase[64];   // element index of the row's sample 0 in the stream's [C, T] block
    __shared__ int rvn[64];         // samples of the row that lie inside the stream
    __shared__ int rmode[64];
    __shared__ unsigned ring[64][64];   // [word slot][lane]: every lane's next words of its frame (dfx_bits_topup)
    const DfxFlacStream S = streams[blockIdx.y];
    const int C = S.channels, ncand = cand_n[blockIdx.y];
    if ((int64_t)blockIdx.x * 64 >= (int64_t)ncand * C) return;   // (the whole block)
    const int lane = (int)threadIdx.x;
    const int t = (int)(blockIdx.x * 64u) + lane;
    const int ci = t / C, ch = t - ci * C;
    const DfxFlacCand *cp = cands + S.cand_base + (ci < ncand ? ci : 0);
    bool active = ci < ncand && cp->samp >= 0;
    const int bs = active ? cp->bs : 0, assign = active ? cp->assign : 0;
    DfxBits r;
    DfxFlacSub u;
    u.kind = DFX_FLAC_CONST, u.order = 0, u.wasted = 0, u.ebps = 1;
    int cval = 0, shift = 0, pbits = 4, esc = 15, psize = 0, prem = 0, k = 0, parts_left = 0;
    bool wide = false, first = true, raw = false;
    dfx_bits_open(r, blob, S, active ? cp->pos * 8u + cp->sub[ch] : 0u, &ring[0][lane]);   // (every lane: the ring is filled in step)
    if (active) active = dfx_flac_sub_head(r, S.bps, assign, ch, u);   // (held in the measure pass: a frame that counts has no reserved code)
    rbase[lane] = active ? (int64_t)ch * S.total + cp->samp : 0;
    {
        const int64_t room = active ? S.total - cp->samp : 0;
        rvn[lane] = (int)(room < bs ? room : bs);
    }
    rmode[lane] = active && assign >= 8 ? assign : 0;
    const bool i16 = S.bps <= 16;
    const int up = i16 ? 16 - S.bps : 0;                       // a stream below 16 bits fills the int16 from the top, like a 16-bit WAVE of it
    const float scale = 1.0f / (float)(1u << (S.bps - 1));
    const int nloop = (S.max_block + DFX_FLAC_TILE - 1) / DFX_FLAC_TILE * DFX_FLAC_TILE;
    for (int n0 = 0; n0 < nloop; n0 += DFX_FLAC_TILE) {
        if (n0) dfx_bits_topup(r);
#pragma unroll 1
        for (int n = n0; n < n0 + DFX_FLAC_TILE; ++n) {
            if (!active || n >= bs) continue;
            int v;
            if (n == 0 && u.kind == DFX_FLAC_CONST) cval = dfx_bits_sget(r, u.ebps);
            if (u.kind == DFX_FLAC_CONST) {
                v = cval;
            } else if (u.kind == DFX_FLAC_VERBATIM || n < u.order) {
                v = dfx_bits_sget(r, u.ebps);
            } else {
                if (n == u.order) {   // behind the warm-up: the predictor, then the residual's header
                    int prec = 4;
                    if (u.kind == DFX_FLAC_LPC) {
                        prec = (int)dfx_bits_get(r, 4) + 1;
                        shift = dfx_bits_sget(r, 5);
                        if (shift < 0) shift = 0;
                        for (int j = 0; j < u.order; ++j) coef[j][lane] = dfx_bits_sget(r, prec);
                    } else {
                        const int o = u.order;
                        coef[0][lane] = o == 1 ? 1 : (o == 2 ? 2 : (o == 3 ? 3 : 4));
                        coef[1][lane] = o == 2 ? -1 : (o == 3 ? -3 : -6);
                        coef[2][lane] = o == 3 ? 1 : 4;
                        coef[3][lane] = -1;
                        shift = 0;
                    }
                    int lg = 0;
                    while ((1 << lg) < u.order) ++lg;
                    wide = u.ebps + prec + lg > 32;   // else |sum| < 2^(ebps - 1 + prec - 1 + lg) <= 2^30: exact in 32 bits
                    const unsigned method = dfx_bits_get(r, 2);
                    pbits = method ? 5 : 4, esc = method ? 31 : 15;
                    const int po = (int)dfx_bits_get(r, 4);
                    psize = bs >> po;
                    parts_left = 1 << po;
                    prem = 0, first = true;
                }
                while (prem == 0 && parts_left > 0) {
                    k = (int)dfx_bits_get(r, pbits);
                    raw = k == esc;
                    if (raw) k = (int)dfx_bits_get(r, 5);
                    prem = psize - (first ? u.order : 0);
                    first = false;
                    --parts_left;
                }
                --prem;
                int res;
                if (raw) {
                    res = k ? dfx_bits_sget(r, k) : 0;
                } else {
                    const uint32_t qz = dfx_bits_unary(r);
                    const uint32_t uu = (qz << k) | dfx_bits_get(r, k);
                    res = (int)(uu >> 1) ^ -(int)(uu & 1u);
                }
                int pred;
                if (wide) {
                    int64_t acc = 0;
#pragma unroll 4
                    for (int j = 0; j < u.order; ++j) acc += (int64_t)coef[j][lane] * (int64_t)hist[(n - 1 - j) & 31][lane];
                    pred = (int)(acc >> shift);
                } else {
                    int acc = 0;
#pragma unroll 4
                    for (int j = 0; j < u.order; ++j) acc += coef[j][lane] * hist[(n - 1 - j) & 31][lane];
                    pred = acc >> shift;
                }
                v = (int)((unsigned)res + (unsigned)pred);
            }
            hist[n & 31][lane] = v;
            tile[lane][n - n0] = (int)((unsigned)v << u.wasted);
        }
        __syncthreads();
#pragma unroll 4
        for (int it = 0; it < DFX_FLAC_TILE; ++it) {
            const int idx = it * 64 + lane;
            const int row = idx / DFX_FLAC_TILE, j = idx - row * DFX_FLAC_TILE, n = n0 + j;
            if (n >= rvn[row]) continue;
            const int mode = rmode[row];
            int v = tile[row][j];
            if (mode) {
                const int a = tile[row & ~1][j], b = tile[row | 1][j];
                if (mode == 8)
                    v = (row & 1) ? a - b : a;
                else if (mode == 9)
                    v = (row & 1) ? b : a + b;
                else {
                    const int m = (int)((unsigned)a << 1) | (b & 1);
                    v = (row & 1) ? (m - b) >> 1 : (m + b) >> 1;
                }
            }
            const int64_t e = rbase[row] + n;
            if (i16)
                reinterpret_cast<int16_t *>(out + S.out_off)[e] = (int16_t)((unsigned)v << up);
            else
                reinterpret_cast<float *>(out + S.out_off)[e] = (float)v * scale;
        }
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static uint64_t flac_be(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; ++i) v = (v << 8) | p[i];
    return v;
}

extern "C" int dfx_flac_probe(const uint8_t *head, int64_t n, dfx_flac_info *out) {
    if (!head || !out || n < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: bad arguments");
    int64_t at = 0;
    if (n >= 10 && head[0] == 'I' && head[1] == 'D' && head[2] == '3') {   // ID3v2: 10 bytes, a sync-safe size, a footer when flag bit 4 is set
        const int64_t size = ((int64_t)(head[6] & 0x7F) << 21) | ((int64_t)(head[7] & 0x7F) << 14) | ((int64_t)(head[8] & 0x7F) << 7) | (head[9] & 0x7F);
        at = 10 + size + ((head[5] & 0x10) ? 10 : 0);
    }
    if (at + 4 <= n && memcmp(head + at, "OggS", 4) == 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: Ogg-FLAC is not decoded (native FLAC only)");
    if (at + 4 > n || memcmp(head + at, "fLaC", 4) != 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: not a FLAC stream (no 'fLaC' marker)");
    at += 4;
    bool have = false, last = false;
    dfx_flac_info I;
    memset(&I, 0, sizeof(I));
    while (!last) {
        if (at + 4 > n) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: the metadata blocks do not end inside the %lld bytes given", (long long)n);
        last = (head[at] & 0x80) != 0;
        const int type = head[at] & 0x7F;
        const int64_t size = (int64_t)flac_be(head + at + 1, 3);
        at += 4;
        if (at + size > n) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: the metadata blocks do not end inside the %lld bytes given", (long long)n);
        if (type == 0 && !have) {
            if (size < 34) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: STREAMINFO of %lld bytes (34 at least)", (long long)size);
            const uint8_t *p = head + at;
            I.min_block = (int32_t)flac_be(p, 2), I.max_block = (int32_t)flac_be(p + 2, 2);
            const uint64_t w = flac_be(p + 10, 8);   // rate 20, channels - 1 3, bps - 1 5, total 36
            I.sample_rate = (int32_t)(w >> 44);
            I.channels = (int32_t)((w >> 41) & 7) + 1;
            I.bits_per_sample = (int32_t)((w >> 36) & 31) + 1;
            I.total_samples = (int64_t)(w & (((uint64_t)1 << 36) - 1));
            memcpy(I.md5, p + 18, 16);
            have = true;
        }
        at += size;
    }
    if (!have) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: no STREAMINFO block");
    if (I.channels > 8) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: %d channels (8 at most)", I.channels);
    if (I.bits_per_sample < 8 || I.bits_per_sample > 24)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: %d bits per sample (8 to 24 are decoded)", I.bits_per_sample);
    if (I.max_block < 1 || I.min_block > I.max_block || I.sample_rate <= 0)
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_probe: inconsistent STREAMINFO (block sizes %d .. %d, rate %d)", I.min_block, I.max_block, I.sample_rate);
    I.first_frame = (int32_t)at;
    *out = I;
    return DFX_OK;
}

// candidates a stream's list holds: its frames (every one but the last has min_block samples at least), and room for look-alikes
static int64_t flac_cand_cap(int64_t len, const dfx_flac_info &I) {
    const int64_t mb = I.min_block < 16 ? 16 : I.min_block;
    return I.total_samples / mb + 18 + len / 1024;
}
static int64_t flac_align(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

extern "C" int dfx_flac_workspace_bytes(int64_t n_streams, const int64_t *lengths, const dfx_flac_info *infos, int64_t *bytes) {
    if (n_streams < 0 || !bytes || (n_streams > 0 && (!lengths || !infos))) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_workspace_bytes: bad arguments");
    int64_t cands = 0;
    for (int64_t i = 0; i < n_streams; ++i) {
        if (lengths[i] < 0 || lengths[i] > DFX_FLAC_MAX_LEN) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_workspace_bytes: stream %lld has %lld bytes (2^28 at most)", (long long)i, (long long)lengths[i]);
        cands += flac_cand_cap(lengths[i], infos[i]);
    }
    *bytes = flac_align(n_streams * (int64_t)sizeof(DfxFlacStream), 256) + flac_align(n_streams * 8, 256) + cands * (int64_t)sizeof(DfxFlacCand) + 256;
    return DFX_OK;
}

extern "C" int dfx_flac_decode(const uint8_t *blob, int64_t blob_bytes, int64_t n_streams, const int64_t *offsets, const int64_t *lengths,
                               const dfx_flac_info *infos, const int64_t *out_offsets, void *out, int64_t out_bytes, int64_t *status,
                               void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_streams < 0 || blob_bytes < 0 || out_bytes < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: bad arguments");
    if (n_streams == 0) return DFX_OK;
    if (!blob || !offsets || !lengths || !infos || !out_offsets || !status || !workspace || (!out && out_bytes > 0))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: null buffer");
    if (n_streams > 65535) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: %lld streams in one call (65535 at most)", (long long)n_streams);
    if (((uintptr_t)blob & 15) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 15))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: the byte buffer and the workspace must be 16-byte aligned, the output 4-byte aligned");
    int64_t need = 0;
    if (int rc = dfx_flac_workspace_bytes(n_streams, lengths, infos, &need)) return rc;
    if (workspace_bytes < need) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    std::vector<DfxFlacStream> desc((size_t)n_streams);
    int64_t cand_at = 0, most_lanes = 0;
    for (int64_t i = 0; i < n_streams; ++i) {
        const dfx_flac_info &I = infos[i];
        if (I.channels < 1 || I.channels > 8 || I.bits_per_sample < 8 || I.bits_per_sample > 24 || I.max_block < 1 || I.max_block > 65535 ||
            I.total_samples < 0 || I.first_frame < 0 || I.first_frame > lengths[i])
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: stream %lld: not a dfx_flac_probe result (1-8 channels, 8-24 bits)", (long long)i);
        if ((offsets[i] & 15) || offsets[i] < 0 || flac_align(offsets[i] + lengths[i], 16) > blob_bytes)
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: stream %lld: its offset must be a multiple of 16 and the buffer extend to the 16-byte chunk of its last byte", (long long)i);
        const int64_t elem = I.bits_per_sample <= 16 ? 2 : 4;
        if ((out_offsets[i] & 3) || out_offsets[i] < 0 || out_offsets[i] + elem * I.channels * I.total_samples > out_bytes)
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_flac_decode: stream %lld: its [C, T] block does not lie inside the output buffer at a multiple of 4", (long long)i);
        DfxFlacStream &S = desc[(size_t)i];
        memset(&S, 0, sizeof(S));
        S.off = offsets[i], S.total = I.total_samples, S.out_off = out_offsets[i];
        S.len = (int32_t)lengths[i], S.first = I.first_frame, S.channels = I.channels, S.bps = I.bits_per_sample;
        S.min_block = I.min_block, S.max_block = I.max_block;
        const int64_t cap = flac_cand_cap(lengths[i], I);
        if (cand_at + cap > 0x7fffffff) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_flac_decode: too many frames in one call");
        S.cand_base = (int32_t)cand_at, S.cand_cap = (int32_t)cap;
        cand_at += cap;
        if (cap * I.channels > most_lanes) most_lanes = cap * I.channels;
    }
    if (int rc = dfx_require_device()) return rc;
    hipStream_t s = dfx_stream(stream);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    DfxFlacStream *d_streams = reinterpret_cast<DfxFlacStream *>(ws);
    int *d_n = reinterpret_cast<int *>(ws + flac_align(n_streams * (int64_t)sizeof(DfxFlacStream), 256));
    int *d_lost = d_n + n_streams;
    DfxFlacCand *d_cands = reinterpret_cast<DfxFlacCand *>(ws + flac_align(n_streams * (int64_t)sizeof(DfxFlacStream), 256) + flac_align(n_streams * 8, 256));
    DfxKScope ks(DFX_K_PCM, s);
    // the descriptors travel as kernel arguments: the caller's arrays are not read after the return
    for (int64_t i0 = 0; i0 < n_streams; i0 += DFX_FLAC_DESC_CHUNK) {
        DfxFlacDescArgs A;
        A.dst = d_streams + i0;
        A.n = (int)(n_streams - i0 < DFX_FLAC_DESC_CHUNK ? n_streams - i0 : DFX_FLAC_DESC_CHUNK);
        for (int i = 0; i < A.n; ++i) A.s[i] = desc[(size_t)(i0 + i)];
        for (int i = A.n; i < DFX_FLAC_DESC_CHUNK; ++i) memset(&A.s[i], 0, sizeof(DfxFlacStream));
        dfx_launch(dfx_k_flac_desc, dim3(1), dim3(DFX_FLAC_DESC_CHUNK), 0, s, A);
        DFX_LAUNCH_CHECK();
    }
    if (out_bytes > 0) DFX_HIP(hipMemsetAsync(out, 0, (size_t)out_bytes, s));   // a lost frame's block, and what lies behind a chain that broke, are zeros
    const unsigned ns = (unsigned)n_streams;
    dfx_launch(dfx_k_flac_scan, dim3(1, ns), dim3(64), 0, s, blob, (const DfxFlacStream *)d_streams, d_cands, d_n, d_lost);
    DFX_LAUNCH_CHECK();
    int64_t most_cap = 0;
    for (int64_t i = 0; i < n_streams; ++i) most_cap = desc[(size_t)i].cand_cap > most_cap ? desc[(size_t)i].cand_cap : most_cap;
    dfx_launch(dfx_k_flac_measure, dim3((unsigned)dfx_ceil_div(most_cap, 64), ns), dim3(64), 0, s, blob, (const DfxFlacStream *)d_streams, d_cands,
               (const int *)d_n);
    DFX_LAUNCH_CHECK();
    dfx_launch(dfx_k_flac_walk, dim3((unsigned)dfx_ceil_div(n_streams, 64)), dim3(64), 0, s, (const DfxFlacStream *)d_streams, d_cands, (const int *)d_n,
               (const int *)d_lost, (int)n_streams, status);
    DFX_LAUNCH_CHECK();
    dfx_launch(dfx_k_flac_decode, dim3((unsigned)dfx_ceil_div(most_lanes, 64), ns), dim3(64), 0, s, blob, (const DfxFlacStream *)d_streams,
               (const DfxFlacCand *)d_cands, (const int *)d_n, out);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}
