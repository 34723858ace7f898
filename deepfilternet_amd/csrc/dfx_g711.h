// dfx: G.711 (one companded byte per sample, mu-law or A-law: what an RTP payload and a telephony WAVE file hold) <-> 16-bit linear / float32.
// A part of dfx_io.hip.  The four conversions are closed forms (include/dfx.h states them): arithmetic on the lane, no table in memory.
//
//   decode  mu: u = ~c & 0xFF;  t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);  s = (u & 0x80) ? 132 - t : t - 132          (|s| <= 32124)
//           A:  a = c ^ 0x55;   e = (a >> 4) & 7, m = a & 15;  t = e == 0 ? (m << 4) + 8 : ((m << 4) + 264) << (e - 1);
//               s = (a & 0x80) ? t : -t                                                                                    (|s| <= 32256)
//   encode  sign-magnitude, as G.711 defines it: the codes of s and -s differ in the sign bit only (s in 1 .. 32767)
//           mu: m = min(|s|, 32635) + 132;  e = msb(m) - 7;  c = ~((s < 0 ? 0x80 : 0) | e << 4 | ((m >> (e + 3)) & 15)) & 0xFF
//           A:  m = min(|s|, 32767) >> 3;   e = m < 32 ? 0 : msb(m) - 4;  mant = e == 0 ? (m >> 1) & 15 : (m >> e) & 15;
//               c = ((s < 0 ? 0 : 0x80) | e << 4 | mant) ^ 0x55
//   float -> s: trunc(clamp(x * 32768, -32768, 32767)), NaN -> 0: this rule SATURATES (dfx_f32_to_pcm16 wraps like save_audio's cast and stays
//           as it is): the encoders clip at their top segment anyway, and a wrapped sample is a full-scale click on a phone line.
//   Silence (s = 0) is 0xFF (mu-law) / 0xD5 (A-law).  encode(decode(c)) == c for every code but mu-law's 0x7F (negative zero -> 0xFF).
#pragma once

#define DFX_G711_CODES_PER_LANE 16

static __host__ __device__ __forceinline__ int dfx_ulaw_to_s16(unsigned c) {
    const unsigned u = ~c & 0xFFu;
    const int t = (int)((((u & 15u) << 3) + 132u) << ((u >> 4) & 7u));
    return (u & 0x80u) ? 132 - t : t - 132;
}
static __host__ __device__ __forceinline__ int dfx_alaw_to_s16(unsigned c) {
    const unsigned a = (c ^ 0x55u) & 0xFFu, e = (a >> 4) & 7u, m = a & 15u;
    const int t = (int)(e == 0 ? (m << 4) + 8u : ((m << 4) + 264u) << (e - 1u));
    return (a & 0x80u) ? t : -t;
}
static __host__ __device__ __forceinline__ unsigned dfx_s16_to_ulaw(int s) {
    const unsigned mag = (unsigned)(s < 0 ? -s : s);
    const unsigned m = (mag < 32635u ? mag : 32635u) + 132u;        // 132 .. 32767: msb in 7 .. 14
    const unsigned e = (unsigned)(31 - __builtin_clz(m)) - 7u;
    return ~((s < 0 ? 0x80u : 0u) | (e << 4) | ((m >> (e + 3u)) & 15u)) & 0xFFu;
}
static __host__ __device__ __forceinline__ unsigned dfx_s16_to_alaw(int s) {
    const unsigned mag = (unsigned)(s < 0 ? -s : s);
    const unsigned m = (mag < 32767u ? mag : 32767u) >> 3;           // 0 .. 4095
    const unsigned e = m < 32u ? 0u : (unsigned)(31 - __builtin_clz(m)) - 4u;
    const unsigned mant = e == 0 ? (m >> 1) & 15u : (m >> e) & 15u;
    return ((s < 0 ? 0u : 0x80u) | (e << 4) | mant) ^ 0x55u;
}
// law: DFX_G711_ULAW (1) or DFX_G711_ALAW (2), checked by the callers
static __host__ __device__ __forceinline__ int dfx_g711_to_s16(unsigned c, int law) { return law == DFX_G711_ULAW ? dfx_ulaw_to_s16(c) : dfx_alaw_to_s16(c); }
static __host__ __device__ __forceinline__ unsigned dfx_s16_to_g711(int s, int law) { return law == DFX_G711_ULAW ? dfx_s16_to_ulaw(s) : dfx_s16_to_alaw(s); }
static __host__ __device__ __forceinline__ int dfx_f32_to_s16_sat(float x) {
    float v = x * 32768.0f;
    v = v != v ? 0.f : fminf(fmaxf(v, -32768.0f), 32767.0f);
    return (int)v;   // truncation toward zero
}
static __host__ __device__ __forceinline__ unsigned dfx_g711_silence(int law) { return law == DFX_G711_ULAW ? 0xFFu : 0xD5u; }

struct alignas(16) DfxCodes16 {
    unsigned w[4];   // 16 codes, in memory order (little endian: code j is byte j & 3 of word j >> 2)
};

// Both kernels split [0, n) by the BYTE side's address: `head` single codes up to its first 16-byte boundary (all n where the array ends before
// it), then nvec runs of 16 codes — one 16-byte access per lane, grid-stride over int64 —, then the `n - head - 16 nvec` < 16 last ones singly.
// The head and the tail are the first 32 threads of the grid's; the wide side (float / int16) is addressed per sample, so it needs no more than
// its type's own alignment.
template <bool I16>
__global__ void __launch_bounds__(256) dfx_k_g711_decode(const uint8_t *__restrict__ codes, int law, int64_t n, int64_t head, int64_t nvec,
                                                         void *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
    auto put = [&](int64_t i, unsigned c) {
        const int s = dfx_g711_to_s16(c, law);
        if (I16)
            static_cast<int16_t *>(out)[i] = (int16_t)s;
        else
            static_cast<float *>(out)[i] = (float)s * (1.0f / 32768.0f);
    };
    if (gid < 32) {
        const int64_t i = gid < 16 ? gid : head + nvec * DFX_G711_CODES_PER_LANE + (gid - 16);
        if (gid < 16 ? i < head : i < n) put(i, codes[i]);
    }
    const DfxCodes16 *cv = reinterpret_cast<const DfxCodes16 *>(codes + head);
    for (int64_t v = gid; v < nvec; v += gsz) {
        const DfxCodes16 c = cv[v];
        const int64_t o = head + v * DFX_G711_CODES_PER_LANE;
#pragma unroll
        for (int j = 0; j < DFX_G711_CODES_PER_LANE; ++j) put(o + j, (c.w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    }
}

template <bool I16>
__global__ void __launch_bounds__(256) dfx_k_g711_encode(const void *__restrict__ x, int law, int64_t n, int64_t head, int64_t nvec,
                                                         uint8_t *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
    auto get = [&](int64_t i) -> unsigned {
        const int s = I16 ? (int)static_cast<const int16_t *>(x)[i] : dfx_f32_to_s16_sat(static_cast<const float *>(x)[i]);
        return dfx_s16_to_g711(s, law);
    };
    if (gid < 32) {
        const int64_t i = gid < 16 ? gid : head + nvec * DFX_G711_CODES_PER_LANE + (gid - 16);
        if (gid < 16 ? i < head : i < n) out[i] = (uint8_t)get(i);
    }
    DfxCodes16 *cv = reinterpret_cast<DfxCodes16 *>(out + head);
    for (int64_t v = gid; v < nvec; v += gsz) {
        const int64_t o = head + v * DFX_G711_CODES_PER_LANE;
        DfxCodes16 c;
#pragma unroll
        for (int q = 0; q < 4; ++q) c.w[q] = get(o + 4 * q) | (get(o + 4 * q + 1) << 8) | (get(o + 4 * q + 2) << 16) | (get(o + 4 * q + 3) << 24);
        cv[v] = c;
    }
}

// head / nvec of a byte array at address p with n codes
static void dfx_g711_split(const void *p, int64_t n, int64_t *head, int64_t *nvec) {
    int64_t h = (int64_t)((16 - ((uintptr_t)p & 15)) & 15);
    if (h > n) h = n;
    *head = h, *nvec = (n - h) / DFX_G711_CODES_PER_LANE;
}

extern "C" int dfx_g711_decode(const uint8_t *codes, int law, int64_t n, void *out, int out_is_pcm16, void *stream) {
    if (n < 0 || (law != DFX_G711_ULAW && law != DFX_G711_ALAW))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_g711_decode: bad arguments (law: DFX_G711_ULAW or DFX_G711_ALAW)");
    if (n > 0 && (!codes || !out)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_g711_decode: null buffer");
    if (int rc = dfx_require_device()) return rc;
    if (n == 0) return DFX_OK;
    int64_t head, nvec;
    dfx_g711_split(codes, n, &head, &nvec);
    DfxKScope ks(DFX_K_PCM, dfx_stream(stream));
    if (out_is_pcm16)
        dfx_launch(dfx_k_g711_decode<true>, dim3(io_grid(nvec)), dim3(256), 0, dfx_stream(stream), codes, law, n, head, nvec, out);
    else
        dfx_launch(dfx_k_g711_decode<false>, dim3(io_grid(nvec)), dim3(256), 0, dfx_stream(stream), codes, law, n, head, nvec, out);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}

extern "C" int dfx_g711_encode(const void *x, int x_is_pcm16, int law, int64_t n, uint8_t *out, void *stream) {
    if (n < 0 || (law != DFX_G711_ULAW && law != DFX_G711_ALAW))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_g711_encode: bad arguments (law: DFX_G711_ULAW or DFX_G711_ALAW)");
    if (n > 0 && (!x || !out)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_g711_encode: null buffer");
    if (int rc = dfx_require_device()) return rc;
    if (n == 0) return DFX_OK;
    int64_t head, nvec;
    dfx_g711_split(out, n, &head, &nvec);
    DfxKScope ks(DFX_K_PCM, dfx_stream(stream));
    if (x_is_pcm16)
        dfx_launch(dfx_k_g711_encode<true>, dim3(io_grid(nvec)), dim3(256), 0, dfx_stream(stream), x, law, n, head, nvec, out);
    else
        dfx_launch(dfx_k_g711_encode<false>, dim3(io_grid(nvec)), dim3(256), 0, dfx_stream(stream), x, law, n, head, nvec, out);
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}
