// dfx: the composite measures' parts on the device — segmental SNR, log-likelihood ratio (LLR), weighted spectral slope (WSS) and the
// frequency-weighted segmental SNR of df/sepm.py (SNRseg :28-51, fwSNRseg :54-182, lpcoeff / llr :200-277, findLocPeaks / wss :280-487).
// A part of dfx_io.hip, behind dfx_metrics.h, whose conventions hold: a row is scored as if it were alone (nothing depends on the rows around
// it, the padding or what the workspace held), the rows' lengths travel as kernel arguments, grids are sized by the longest row and
// workgroups past a row's own frames exit, no atomics, every sum in an order fixed by the row's own length.
//
// Arithmetic is float64 throughout, as sepm.py's is (float32 samples that numpy promotes).  The rate is 16 kHz: 480-sample frames at hop 120
// under the reference's own Hann 0.5 (1 - cos(2 pi k / 481)), k = 1..480; LPC order 16; a 1024-point transform; 25 critical bands.  A row of
// n samples has F = (n - 480) / 120 frames for all four measures (F < 1: the reference raises or averages nothing — every score NaN).
//   time      one wave per frame: the windowed frames in LDS; lane (signal, lag) sums one autocorrelation lag 0..16, one more lane the
//             error energy; lanes 0 / 1 run the Levinson recursion of the clean / processed frame with max(E, eps); lane 0 takes the two
//             17 x 17 forms a' T(R_clean) a in float64 from the float32-rounded a and R (the reference: in float32, in its BLAS's order),
//             frac <= 0 -> 1000, log; and 10 log10(sum c^2 / (sum (c - p)^2 + eps) + eps) clamped to [-10, 35]
//   spectrum  one wave per frame: (sample + eps) * window packed as 512 complex values, a radix-2 autosort transform in place in LDS (8 KB),
//             the split to bins 0..511 of the 1024-point real transform; |X|^2 (wss: |Zxx| / scale is the plain transform) and |X| / sum |X|
//             (fwSNRseg) through the 25 critical-band filters (host table, sepm.py:129-135), then wss :450-484 and fwSNRseg :171-180
//   rows      per row: the means over F frames; for LLR and WSS the mean of the K = round_half_even(0.95 F) smallest values: the K-th
//             smallest by a bitwise search over the ordered float64 keys, then the sum of the smaller values plus the ties
#pragma once

#define DFX_SEPM_FS 16000
#define DFX_SEPM_WIN 480
#define DFX_SEPM_HOP 120
#define DFX_SEPM_P 16
#define DFX_SEPM_NB 25           // critical bands
#define DFX_SEPM_TAPS 32         // the most non-zero taps of a band's filter (29 at 16 kHz)
#define DFX_SEPM_FPB 16          // frames per workgroup of the frame kernels
#define DFX_SEPM_EPS 2.220446049250313e-16   /* np.finfo(np.float64).eps */

struct DfxSepmTab {              // in the workspace, written by every call
    double win[DFX_SEPM_WIN];
    double twr[512], twi[512];   // exp(-2 pi i k / 1024)
    double crit[DFX_SEPM_NB][DFX_SEPM_TAPS];
    int lo[DFX_SEPM_NB], cnt[DFX_SEPM_NB];   // band i: crit[i][t] weighs bin lo[i] + t, t < cnt[i]
};

struct DfxSepmBands {
    double crit[DFX_SEPM_NB][DFX_SEPM_TAPS];
    int lo[DFX_SEPM_NB], cnt[DFX_SEPM_NB];
    bool ok;
};

// crit_filter of fwSNRseg / wss (sepm.py:68-135, :315-413) at fs = 16000: Gaussian filters cut at the -30 dB point, the non-zero run of each
static const DfxSepmBands &dfx_sepm_bands() {
    static const DfxSepmBands bands = [] {
        static const double cent[DFX_SEPM_NB] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,   540.0,   617.372, 703.378, 798.717, 904.128, 1020.38,
                                                 1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
        static const double bwid[DFX_SEPM_NB] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
                                                 140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};
        DfxSepmBands t;
        memset(&t, 0, sizeof(t));
        t.ok = true;
        const double max_freq = DFX_SEPM_FS / 2.0, min_factor = std::exp(-30.0 / (2.0 * 2.303));
        const int half = 512;
        for (int i = 0; i < DFX_SEPM_NB; ++i) {
            const double f0 = std::floor((cent[i] / max_freq) * half), bw = (bwid[i] / max_freq) * half;
            const double norm_factor = std::log(bwid[0]) - std::log(bwid[i]);
            int first = -1, last = -1;
            for (int j = 0; j < half; ++j) {
                const double u = ((double)j - f0) / bw, sq = u * u;
                const double e = -11.0 * sq;
                const double v = std::exp(e + norm_factor);
                if (v > min_factor) {
                    if (first < 0) first = j;
                    if (last >= 0 && j != last + 1) t.ok = false;
                    last = j;
                    if (j - first < DFX_SEPM_TAPS) t.crit[i][j - first] = v;
                }
            }
            t.lo[i] = first < 0 ? 0 : first;
            t.cnt[i] = first < 0 ? 0 : last - first + 1;
            if (t.cnt[i] > DFX_SEPM_TAPS) t.ok = false;
        }
        return t;
    }();
    return bands;
}

#define DFX_SEPM_CRIT_CHUNK 200
struct DfxSepmCritArgs {
    DfxSepmTab *tab;
    int part;                          // values [part * CHUNK, (part + 1) * CHUNK) of crit
    double v[DFX_SEPM_CRIT_CHUNK];
    int lo[DFX_SEPM_NB], cnt[DFX_SEPM_NB];
};
__global__ void __launch_bounds__(256) dfx_k_sepm_crit(DfxSepmCritArgs A) {
    const int i = (int)threadIdx.x;
    double *dst = &A.tab->crit[0][0];
    if (i < DFX_SEPM_CRIT_CHUNK && A.part * DFX_SEPM_CRIT_CHUNK + i < DFX_SEPM_NB * DFX_SEPM_TAPS) dst[A.part * DFX_SEPM_CRIT_CHUNK + i] = A.v[i];
    if (A.part == 0 && i >= 224 && i < 224 + DFX_SEPM_NB) A.tab->lo[i - 224] = A.lo[i - 224], A.tab->cnt[i - 224] = A.cnt[i - 224];
}

__global__ void __launch_bounds__(512) dfx_k_sepm_tables(DfxSepmTab *t) {
    const int i = (int)threadIdx.x;
    const double pi = 3.14159265358979323846;
    const double a = -2.0 * pi * (double)i / 1024.0;
    t->twr[i] = cos(a), t->twi[i] = sin(a);
    if (i < DFX_SEPM_WIN) t->win[i] = 0.5 * (1.0 - cos(2.0 * pi * (double)(i + 1) / (double)(DFX_SEPM_WIN + 1)));
}

// the rows' K = round_half_even(0.95 F), computed on the host in double; as kernel arguments like the lengths
struct DfxSepmTrim {
    int *krow;        // [B]
    int64_t row0;
    int n;
    int k[DFX_MT_ROWS];
};
__global__ void __launch_bounds__(DFX_MT_ROWS) dfx_k_sepm_trim(DfxSepmTrim A) {
    const int i = (int)threadIdx.x;
    if (i < A.n) A.krow[A.row0 + i] = A.k[i];
}

static __host__ __device__ __forceinline__ int64_t dfx_sepm_frames(int64_t n16) {
    return n16 >= DFX_SEPM_WIN + DFX_SEPM_HOP ? (n16 - DFX_SEPM_WIN) / DFX_SEPM_HOP : 0;
}

struct DfxSepmArgs {
    const float *clean, *proc;       // at 16 kHz
    int64_t stride, B, Fmax, tiles;
    const int64_t *rows;             // [2][B]; rows[B + b]: samples at 16 kHz
    const int *krow;                 // [B]
    const DfxSepmTab *tab;
    double *val;                     // [B][4][Fmax]: per frame ssnr, llr, wss, fwsnr
    double *out;                     // [B][4]
    int *info;                       // null or [B][2]: F, K
};

static __device__ __forceinline__ double dfx_sepm_clamp_db(double v) {   // sepm.py:48-49, :179-180 (a NaN stays)
    if (v < -10.0) v = -10.0;
    if (v > 35.0) v = 35.0;
    return v;
}

// lpcoeff's recursion (sepm.py:211-228) on the lags R[0..16]: products and sums rounded one by one, as numpy forms them -> lpparams[1..16]
static __device__ __forceinline__ void dfx_sepm_levinson(const double *R, float *lp) {
#pragma clang fp contract(off)
    double a[DFX_SEPM_P], t[DFX_SEPM_P];
    double E = R[0];
#pragma unroll
    for (int i = 0; i < DFX_SEPM_P; ++i) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const double pr = a[j] * R[i - j];
            sum = sum + pr;
        }
        const double rc = (R[i + 1] - sum) / (E > DFX_SEPM_EPS ? E : DFX_SEPM_EPS);
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const double pr = rc * a[i - 1 - j];
            t[j] = a[j] - pr;
        }
#pragma unroll
        for (int j = 0; j < i; ++j) a[j] = t[j];
        a[i] = rc;
        const double r2 = rc * rc;
        E = (1.0 - r2) * E;
    }
#pragma unroll
    for (int j = 0; j < DFX_SEPM_P; ++j) lp[1 + j] = (float)(-a[j]);
    lp[0] = 1.f;
}

// a' T(R) a with a and R the float32-rounded values, in float64: rows in order, each row's sum in order
static __device__ __forceinline__ double dfx_sepm_form(const float *a32, const double *R) {
    double a[DFX_SEPM_P + 1];
#pragma unroll
    for (int i = 0; i <= DFX_SEPM_P; ++i) a[i] = (double)a32[i];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i <= DFX_SEPM_P; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j <= DFX_SEPM_P; ++j) t += R[i > j ? i - j : j - i] * a[j];
        s += a[i] * t;
    }
    return s;
}

// Workgroup = DFX_SEPM_FPB frames of one row, one wave per frame at a time (sepm.py:36-49, :200-273).  Every LDS array is split by wave, so
// the steps of a frame are ordered by DFX_WAVE_SYNC alone: no workgroup barrier, a wave never waits for another
__global__ void __launch_bounds__(256) dfx_k_sepm_time(DfxSepmArgs A) {
    __shared__ double fr[4][2][DFX_SEPM_WIN];
    __shared__ double acc[4][36];    // clean lags 0..16, processed lags 0..16, sum (c - p)^2
    __shared__ float lp[4][2][DFX_SEPM_P + 2];
    const int64_t b = blockIdx.x / A.tiles, f0 = (blockIdx.x - b * A.tiles) * DFX_SEPM_FPB;
    const int64_t F = dfx_sepm_frames(A.rows[A.B + b]);
    if (f0 >= F) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *xc = A.clean + b * A.stride, *xp = A.proc + b * A.stride;
    double wv[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) wv[m] = lane + 64 * m < DFX_SEPM_WIN ? A.tab->win[lane + 64 * m] : 0.0;
    for (int it = 0; it < DFX_SEPM_FPB / 4; ++it) {
        const int64_t f = f0 + it * 4 + wave;
        const bool active = f < F;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int k = lane + 64 * m;
            if (k < DFX_SEPM_WIN) {
                fr[wave][0][k] = active ? wv[m] * (double)xc[f * DFX_SEPM_HOP + k] : 0.0;
                fr[wave][1][k] = active ? wv[m] * (double)xp[f * DFX_SEPM_HOP + k] : 0.0;
            }
        }
        DFX_WAVE_SYNC();
        if (lane < 35) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, tail = 0.0;
            if (lane < 34) {
                const int sig = lane >= 17 ? 1 : 0, lag = lane - 17 * sig, cnt = DFX_SEPM_WIN - lag;
                const double *v = fr[wave][sig];
                int k = 0;
                for (; k + 3 < cnt; k += 4) {
                    s0 += v[k] * v[k + lag];
                    s1 += v[k + 1] * v[k + 1 + lag];
                    s2 += v[k + 2] * v[k + 2 + lag];
                    s3 += v[k + 3] * v[k + 3 + lag];
                }
                for (; k < cnt; ++k) tail += v[k] * v[k + lag];
            } else {
                const double *c = fr[wave][0], *p = fr[wave][1];
                for (int k = 0; k < DFX_SEPM_WIN; k += 4) {
                    const double d0 = c[k] - p[k], d1 = c[k + 1] - p[k + 1], d2 = c[k + 2] - p[k + 2], d3 = c[k + 3] - p[k + 3];
                    s0 += d0 * d0, s1 += d1 * d1, s2 += d2 * d2, s3 += d3 * d3;
                }
            }
            acc[wave][lane] = ((s0 + s1) + (s2 + s3)) + tail;
        }
        DFX_WAVE_SYNC();
        if (lane < 2) {
            double R[DFX_SEPM_P + 1];
#pragma unroll
            for (int k = 0; k <= DFX_SEPM_P; ++k) R[k] = acc[wave][17 * lane + k];
            dfx_sepm_levinson(R, lp[wave][lane]);
        }
        DFX_WAVE_SYNC();
        if (lane == 0 && active) {
            double R[DFX_SEPM_P + 1];
#pragma unroll
            for (int k = 0; k <= DFX_SEPM_P; ++k) R[k] = (double)(float)acc[wave][k];
            const double num = dfx_sepm_form(lp[wave][1], R), den = dfx_sepm_form(lp[wave][0], R) + DFX_SEPM_EPS;
            double frac = num / den;
            if (frac <= 0.0) frac = 1000.0;
            const double snr = 10.0 * log10(acc[wave][0] / (acc[wave][34] + DFX_SEPM_EPS) + DFX_SEPM_EPS);
            A.val[(b * 4 + 0) * A.Fmax + f] = dfx_sepm_clamp_db(snr);
            A.val[(b * 4 + 1) * A.Fmax + f] = log(frac);
        }
    }
}

// one radix-2 autosort pass of a 512-point complex transform in place, 64 lanes (4 butterflies each): all reads, a wave sync, all writes
template <int NS>
static __device__ __forceinline__ void dfx_sepm_fft_pass(double *zr, double *zi, const double *twr, const double *twi, int lane) {
    double ar[4], ai[4], br[4], bi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q, k = j & (NS - 1);
        ar[q] = zr[j], ai[q] = zi[j];
        const double vr = zr[j + 256], vi = zi[j + 256];
        if (NS > 1) {
            const double cr = twr[k * (512 / NS)], ci = twi[k * (512 / NS)];
            br[q] = vr * cr - vi * ci, bi[q] = vr * ci + vi * cr;
        } else {
            br[q] = vr, bi[q] = vi;
        }
    }
    DFX_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q, k = j & (NS - 1), j0 = ((j - k) << 1) + k;
        zr[j0] = ar[q] + br[q], zi[j0] = ai[q] + bi[q];
        zr[j0 + NS] = ar[q] - br[q], zi[j0 + NS] = ai[q] - bi[q];
    }
    DFX_WAVE_SYNC();
}

// findLocPeaks (sepm.py:280-296) for slope index ii of the 25 log energies e: the nearest peak above
static __device__ __forceinline__ double dfx_sepm_loc_peak(const double *e, int ii) {
    int n = ii;
    if (e[ii + 1] - e[ii] > 0.0) {
        while (n < DFX_SEPM_NB - 1 && e[n + 1] - e[n] > 0.0) ++n;
        return e[n - 1];
    }
    while (n >= 0 && e[n + 1] - e[n] <= 0.0) --n;
    return e[n + 1];
}

// Workgroup = DFX_SEPM_FPB frames of one row, one wave per frame at a time, the clean and then the processed signal through the same 8 KB
__global__ void __launch_bounds__(256) dfx_k_sepm_spec(DfxSepmArgs A) {
    __shared__ double twr[512], twi[512];
    __shared__ double zr[4][512], zi[4][512];
    __shared__ double en[4][2][2][DFX_SEPM_NB];    // [signal][0: sum crit |X|^2, 1: sum crit |X| / sum |X|]
    __shared__ double lg[4][2][DFX_SEPM_NB + 1];
    __shared__ double term[4][4][DFX_SEPM_NB];     // wss: W d^2, W; fwSNRseg: W snr, W
    const int64_t b = blockIdx.x / A.tiles, f0 = (blockIdx.x - b * A.tiles) * DFX_SEPM_FPB;
    const int64_t F = dfx_sepm_frames(A.rows[A.B + b]);
    if (f0 >= F) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 512; i += 256) twr[i] = A.tab->twr[i], twi[i] = A.tab->twi[i];
    double wv[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) wv[m] = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {   // packed value lane + 64 m holds samples 2 (lane + 64 m) and the next
        const int k = 2 * (lane + 64 * m);
        if (k < DFX_SEPM_WIN) wv[2 * m] = A.tab->win[k], wv[2 * m + 1] = A.tab->win[k + 1];
    }
    int blo = 0, bcnt = 0, band = 0, kind = 0;
    if (lane < 2 * DFX_SEPM_NB) {
        kind = lane >= DFX_SEPM_NB ? 1 : 0, band = lane - DFX_SEPM_NB * kind;
        blo = A.tab->lo[band], bcnt = A.tab->cnt[band];
    }
    double *wr = zr[wave], *wi = zi[wave];
    __syncthreads();   // the twiddles: the only LDS the workgroup's waves share; everything below is a wave's own
    for (int it = 0; it < DFX_SEPM_FPB / 4; ++it) {
        const int64_t f = f0 + it * 4 + wave;
        const bool active = f < F;
        for (int sig = 0; sig < 2; ++sig) {
            const float *x = (sig ? A.proc : A.clean) + b * A.stride + (active ? f * DFX_SEPM_HOP : 0);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int j = lane + 64 * m, k = 2 * j;
                double re = 0.0, im = 0.0;
                if (m < 4 && active && k < DFX_SEPM_WIN) {
                    re = wv[2 * m] * ((double)x[k] + DFX_SEPM_EPS);
                    im = wv[2 * m + 1] * ((double)x[k + 1] + DFX_SEPM_EPS);
                }
                wr[j] = re, wi[j] = im;
            }
            DFX_WAVE_SYNC();
            dfx_sepm_fft_pass<1>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<2>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<4>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<8>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<16>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<32>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<64>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<128>(wr, wi, twr, twi, lane);
            dfx_sepm_fft_pass<256>(wr, wi, twr, twi, lane);
            // X[k] = (Z[k] + conj Z[512 - k]) / 2 - i / 2 exp(-2 pi i k / 1024) (Z[k] - conj Z[512 - k]), k = 0..511
            double pw[8], mg[8], msum = 0.0;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int k = lane + 64 * m, kc = (512 - k) & 511;
                const double ar = wr[k], ai = wi[k], cr = wr[kc], ci = wi[kc];
                const double er = 0.5 * (ar + cr), ei = 0.5 * (ai - ci);
                const double qr = 0.5 * (ai + ci), qi = -0.5 * (ar - cr);
                const double re = er + (qr * twr[k] - qi * twi[k]), im = ei + (qr * twi[k] + qi * twr[k]);
                pw[m] = re * re + im * im;
                mg[m] = sqrt(pw[m]);
                msum += mg[m];
            }
            msum = dfx_wave_sum(msum);
            DFX_WAVE_SYNC();
#pragma unroll
            for (int m = 0; m < 8; ++m) wr[lane + 64 * m] = pw[m], wi[lane + 64 * m] = mg[m];
            DFX_WAVE_SYNC();
            if (lane < 2 * DFX_SEPM_NB) {
                const double *src = kind ? wi : wr;
                const double *cf = A.tab->crit[band];
                double s = 0.0;
                for (int t = 0; t < bcnt; ++t) s += cf[t] * (kind ? src[blo + t] / msum : src[blo + t]);
                en[wave][sig][kind][band] = s;
            }
            DFX_WAVE_SYNC();
        }
        // log energies clipped at -100 dB (sepm.py:451-455)
        if (lane < 2 * DFX_SEPM_NB) {
            double v = 10.0 * log10(en[wave][kind][0][band]);   // (here `kind` is the signal)
            if (v < -100.0) v = -100.0;
            lg[wave][kind][band] = v;
        }
        DFX_WAVE_SYNC();
        if (lane < DFX_SEPM_NB - 1) {          // wss: slope lane (sepm.py:457-483)
            const double *ec = lg[wave][0], *ep = lg[wave][1];
            double mc = ec[0], mp = ep[0];
            for (int i = 1; i < DFX_SEPM_NB; ++i) {
                if (ec[i] > mc) mc = ec[i];
                if (ep[i] > mp) mp = ep[i];
            }
            const double wc = (20.0 / (20.0 + mc - ec[lane])) * (1.0 / (1.0 + dfx_sepm_loc_peak(ec, lane) - ec[lane]));
            const double wp = (20.0 / (20.0 + mp - ep[lane])) * (1.0 / (1.0 + dfx_sepm_loc_peak(ep, lane) - ep[lane]));
            const double w = (wc + wp) / 2.0, d = (ec[lane + 1] - ec[lane]) - (ep[lane + 1] - ep[lane]);
            term[wave][0][lane] = w * (d * d), term[wave][1][lane] = w;
        } else if (lane >= 32 && lane < 32 + DFX_SEPM_NB) {   // fwSNRseg: band lane - 32 (sepm.py:171-177)
            const int i = lane - 32;
            const double ce = en[wave][0][1][i], pe = en[wave][1][1][i], df = ce - pe;
            double err = df * df;
            if (err < DFX_SEPM_EPS) err = DFX_SEPM_EPS;
            const double w = pow(ce, 0.2);
            term[wave][2][i] = w * (10.0 * log10((ce * ce) / err)), term[wave][3][i] = w;
        }
        DFX_WAVE_SYNC();
        if (lane < 2 && active) {
            const int cntb = lane ? DFX_SEPM_NB : DFX_SEPM_NB - 1;
            const double *tn = term[wave][2 * lane], *td = term[wave][2 * lane + 1];
            double sn = 0.0, sd = 0.0;
            for (int i = 0; i < cntb; ++i) sn += tn[i], sd += td[i];
            const double v = sn / sd;
            A.val[(b * 4 + 2 + lane) * A.Fmax + f] = lane ? dfx_sepm_clamp_db(v) : v;
        }
    }
}

static __device__ __forceinline__ unsigned long long dfx_sepm_bits(double v) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return u;
}
static __device__ __forceinline__ double dfx_sepm_from_bits(unsigned long long u) {
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}
static __device__ __forceinline__ unsigned long long dfx_sepm_key(double v) {   // unsigned order = numeric order (-0 < +0, NaNs at the ends)
    const unsigned long long u = dfx_sepm_bits(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

static __device__ __forceinline__ double dfx_sepm_block_sum(double v, double *red) {   // 256 threads -> every thread the same sum; two barriers
    v = dfx_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// Workgroup (b, pair): pair 0 = the mean of ssnr and the trimmed mean of llr, pair 1 = the mean of fwsnr and the trimmed mean of wss
// (sepm.py:51, :182, :275-277, :485-487).  F < 1: NaN.
__global__ void __launch_bounds__(256) dfx_k_sepm_rows(DfxSepmArgs A) {
    __shared__ double red[4];
    __shared__ long long cred[4];
    const int64_t b = blockIdx.x >> 1;
    const int pair = (int)(blockIdx.x & 1);
    const int64_t F = dfx_sepm_frames(A.rows[A.B + b]);
    const int64_t K = F > 0 ? A.krow[b] : 0;
    double *out = A.out + 4 * b;
    if (pair == 0 && A.info && threadIdx.x == 0) A.info[2 * b] = (int)F, A.info[2 * b + 1] = (int)K;
    if (F < 1 || K < 1 || K > F) {
        if (threadIdx.x == 0) {
            const double nan = dfx_sepm_from_bits(0x7ff8000000000000ull);
            out[pair ? 3 : 0] = nan, out[pair ? 2 : 1] = nan;
        }
        return;
    }
    const double *mean_of = A.val + (b * 4 + (pair ? 3 : 0)) * A.Fmax, *trim_of = A.val + (b * 4 + (pair ? 2 : 1)) * A.Fmax;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < F; i += 256) s += mean_of[i];
    s = dfx_sepm_block_sum(s, red);
    if (threadIdx.x == 0) out[pair ? 3 : 0] = s / (double)F;
    // the key of the K-th smallest value, bit by bit from the top: the largest prefix that fewer than K keys lie below
    unsigned long long kth = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long trial = kth | (1ull << bit);
        long long c = 0;
        for (int64_t i = threadIdx.x; i < F; i += 256) c += dfx_sepm_key(trim_of[i]) < trial ? 1 : 0;
        c = dfx_wave_sum(c);
        if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = c;
        __syncthreads();
        c = cred[0] + cred[1] + cred[2] + cred[3];
        __syncthreads();
        if (c < K) kth = trial;
    }
    double below = 0.0;
    long long nb = 0;
    for (int64_t i = threadIdx.x; i < F; i += 256) {
        const double v = trim_of[i];
        if (dfx_sepm_key(v) < kth) below += v, nb += 1;
    }
    below = dfx_sepm_block_sum(below, red);
    nb = dfx_wave_sum(nb);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = nb;
    __syncthreads();
    nb = cred[0] + cred[1] + cred[2] + cred[3];
    if (threadIdx.x == 0) {
        // the K-th value from its key; the K - nb values that tie with it close the sum
        const unsigned long long u = (kth >> 63) ? (kth & 0x7fffffffffffffffull) : ~kth;
        out[pair ? 2 : 1] = (below + (double)(K - nb) * dfx_sepm_from_bits(u)) / (double)K;
    }
}

struct DfxSepmPlan {
    int orig, nw;                 // fs_source : 16000 after dividing by their gcd
    int64_t Tmax, S16, Fmax, tiles;
    int64_t off_krow, off_tab, off_rs, off_val, bytes;   // rows at offset 0
};
static int dfx_sepm_plan(int fs_source, int64_t B, const int64_t *lens, int64_t stride, DfxSepmPlan *P) {
    if (fs_source <= 0 || B < 0 || (B > 0 && !lens))
        DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm: bad arguments (fs_source > 0, B >= 0, lengths: a host array of B sample counts)");
    const int64_t g = gcd64(fs_source, DFX_SEPM_FS);
    P->orig = (int)(fs_source / g), P->nw = (int)(DFX_SEPM_FS / g);
    int64_t mx = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (lens[b] < 0 || (stride >= 0 && lens[b] > stride))
            DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm: lengths[%lld] = %lld outside [0, stride]", (long long)b, (long long)lens[b]);
        if (lens[b] > mx) mx = lens[b];
    }
    if (mx > ((int64_t)1 << 36)) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_sepm: a row of more than 2^36 samples");
    P->Tmax = mx;
    const int64_t n16 = (mx * P->nw + P->orig - 1) / P->orig;
    P->S16 = (n16 + 3) / 4 * 4;
    P->Fmax = dfx_sepm_frames(n16) > 0 ? dfx_sepm_frames(n16) : 1;
    if (P->Fmax > 0x7fffffff) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_sepm: a row of more than 2^31 frames");
    P->tiles = dfx_ceil_div(P->Fmax, DFX_SEPM_FPB);
    if (B * P->tiles > 0x7fffffff) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_sepm: grid too large");
    int64_t at = dfx_align256(2 * B * 8);
    P->off_krow = at, at += dfx_align256(B * 4);
    P->off_tab = at, at += dfx_align256((int64_t)sizeof(DfxSepmTab));
    P->off_rs = at, at += P->orig != P->nw ? dfx_align256(2 * B * P->S16 * 4) : 0;
    P->off_val = at, at += dfx_align256(B * 4 * P->Fmax * 8);
    P->bytes = at;
    return DFX_OK;
}

extern "C" int dfx_sepm_workspace_bytes(int fs_source, int64_t B, const int64_t *lengths_host, int64_t *bytes) {
    if (!bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm_workspace_bytes: null out");
    DfxSepmPlan P;
    if (int rc = dfx_sepm_plan(fs_source, B, lengths_host, -1, &P)) return rc;
    *bytes = P.bytes;
    return DFX_OK;
}

extern "C" int dfx_sepm(const dfx_resampler *r, const float *clean, const float *processed, int64_t B, int64_t stride, const int64_t *lengths_host,
                        double *out, int32_t *info, void *ws, int64_t ws_bytes, void *stream) {
    if (stride < 0) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm: bad arguments");
    if (r && r->new_sr != DFX_SEPM_FS) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm: the resampler must convert to %d Hz, not %d", DFX_SEPM_FS, r->new_sr);
    DfxSepmPlan P;
    if (int rc = dfx_sepm_plan(r ? r->orig_sr : DFX_SEPM_FS, B, lengths_host, stride, &P)) return rc;
    const DfxSepmBands &bands = dfx_sepm_bands();
    if (!bands.ok) DFX_FAIL(DFX_ERR_UNSUPPORTED, "dfx_sepm: a critical-band filter of more than %d taps", DFX_SEPM_TAPS);
    if (int rc = dfx_require_device()) return rc;
    if (B == 0) return DFX_OK;
    if (!clean || !processed || !out || !ws || ((uintptr_t)ws & 15)) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm: null buffer (the workspace: 16-byte aligned)");
    if (ws_bytes < P.bytes) DFX_FAIL(DFX_ERR_INVALID_ARG, "dfx_sepm: workspace of %lld bytes, %lld needed (dfx_sepm_workspace_bytes)", (long long)ws_bytes, (long long)P.bytes);
    hipStream_t s = dfx_stream(stream);
    char *w = static_cast<char *>(ws);
    int64_t *rows = reinterpret_cast<int64_t *>(w);
    if (int rc = dfx_launch_metric_rows(lengths_host, B, rows, P.orig, P.nw, s)) return rc;
    int *krow = reinterpret_cast<int *>(w + P.off_krow);
    for (int64_t r0 = 0; r0 < B; r0 += DFX_MT_ROWS) {
        DfxSepmTrim T;
        T.krow = krow, T.row0 = r0;
        T.n = (int)(B - r0 < DFX_MT_ROWS ? B - r0 : DFX_MT_ROWS);
        for (int i = 0; i < T.n; ++i) {
            const int64_t n16 = (lengths_host[r0 + i] * P.nw + P.orig - 1) / P.orig;
            T.k[i] = (int)std::nearbyint((double)dfx_sepm_frames(n16) * 0.95);   // int(round(len * alpha)): half to even
        }
        dfx_launch(dfx_k_sepm_trim, dim3(1), dim3(DFX_MT_ROWS), 0, s, T);
    }
    DfxSepmTab *tab = reinterpret_cast<DfxSepmTab *>(w + P.off_tab);
    dfx_launch(dfx_k_sepm_tables, dim3(1), dim3(512), 0, s, tab);
    for (int part = 0; part * DFX_SEPM_CRIT_CHUNK < DFX_SEPM_NB * DFX_SEPM_TAPS; ++part) {
        DfxSepmCritArgs C;
        C.tab = tab, C.part = part;
        const double *src = &bands.crit[0][0];
        for (int i = 0; i < DFX_SEPM_CRIT_CHUNK; ++i) {
            const int at = part * DFX_SEPM_CRIT_CHUNK + i;
            C.v[i] = at < DFX_SEPM_NB * DFX_SEPM_TAPS ? src[at] : 0.0;
        }
        for (int i = 0; i < DFX_SEPM_NB; ++i) C.lo[i] = bands.lo[i], C.cnt[i] = bands.cnt[i];
        dfx_launch(dfx_k_sepm_crit, dim3(1), dim3(256), 0, s, C);
    }
    DFX_LAUNCH_CHECK();
    DfxSepmArgs A;
    A.clean = clean, A.proc = processed, A.stride = stride;
    if (P.orig != P.nw) {   // both signals to 16 kHz, every row with its own length
        float *rs = reinterpret_cast<float *>(w + P.off_rs);
        if (int rc = dfx_resample_rows(r, clean, B, P.Tmax, stride, rs, P.S16, rows, stream)) return rc;
        if (int rc = dfx_resample_rows(r, processed, B, P.Tmax, stride, rs + B * P.S16, P.S16, rows, stream)) return rc;
        A.clean = rs, A.proc = rs + B * P.S16, A.stride = P.S16;
    }
    A.B = B, A.Fmax = P.Fmax, A.tiles = P.tiles;
    A.rows = rows, A.krow = krow, A.tab = tab;
    A.val = reinterpret_cast<double *>(w + P.off_val), A.out = out, A.info = info;
    {
        DfxKScope ks(DFX_K_SEPM_TIME, s);
        dfx_launch(dfx_k_sepm_time, dim3((unsigned)(B * P.tiles)), dim3(256), 0, s, A);
    }
    {
        DfxKScope ks(DFX_K_SEPM_SPEC, s);   // (with the rows' reductions: the timing mask has 32 bits, and this is the last)
        dfx_launch(dfx_k_sepm_spec, dim3((unsigned)(B * P.tiles)), dim3(256), 0, s, A);
        dfx_launch(dfx_k_sepm_rows, dim3((unsigned)(2 * B)), dim3(256), 0, s, A);
    }
    DFX_LAUNCH_CHECK();
    return DFX_OK;
}
