"""A plain numpy float64 restatement of the composite measures' parts (df/sepm.py), one clip at a time, written from the formulas:

    sepm(clean, processed, sr=16000) -> {"ssnr", "llr", "wss", "fwsnr", "F", "K", "runoff_up", "runoff_down", "min_frac", "llr_order_spread"}
    composite(measures, pesq)        -> {"pesq", "csig", "cbak", "covl", "ssnr", "llr", "wss"}   sepm.py:501-510

Frames: 480 samples at hop 120 under w[k] = 0.5 (1 - cos(2 pi k / 481)), k = 1..480; a clip of n samples has F = (n - 480) // 120 of them (n < 600:
none, every value NaN).  K = int(round(0.95 F)) is the number of smallest per-frame values LLR and WSS average.

    ssnr   mean of clamp(10 log10(sum c^2 / (sum (c - p)^2 + eps) + eps), -10, 35) over the windowed frames c, p
    llr    lags 0..16 of each windowed frame, the Levinson recursion with max(E, eps), a and R rounded to float32 (as the reference rounds
           them), then num = a_p' T(R_c) a_p and den = a_c' T(R_c) a_c + eps IN FLOAT64 (the reference takes these two forms in float32, in its
           BLAS's order: the library's documented difference), frac <= 0 -> 1000, log; the mean of the K smallest
    wss    |FFT_1024((x + eps) w)|^2, bins 0..511, through the 25 critical-band filters, 10 log10 clipped at -100, slopes, nearest peaks
           (runoff_up / runoff_down count the frames whose search ran off the top / bottom band), Klatt's weights; the mean of the K smallest
    fwsnr  |FFT| / sum |FFT| through the same filters, error floored at eps, weights energy^0.2, clamp to [-10, 35], mean

Other rates: ``resample(x float32, sr, 16000) -> float32`` comes first (the caller supplies it).  Test code: the product computes none of this on
the host."""
from __future__ import annotations

import numpy as np

FS, WIN, HOP, ORDER, NFFT, NB = 16_000, 480, 120, 16, 1024, 25
EPS = np.finfo(np.float64).eps
CENT = np.array([50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
                 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63])
BANDWIDTH = np.array([70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154,
                      183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136])
MIN_FACTOR = np.exp(-30.0 / (2.0 * 2.303))


def n_frames(n: int) -> int:
    return (n - WIN) // HOP if n >= WIN + HOP else 0


def trim_count(F: int) -> int:
    return int(round(F * 0.95))


def hann() -> np.ndarray:
    return 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, WIN + 1) / (WIN + 1)))


def crit_filter():
    """-> ([25, 512] filters, the smallest relative distance of a tap from the cut)"""
    half = NFFT // 2
    j = np.arange(half)
    out = np.zeros((NB, half))
    margin = np.inf
    for i in range(NB):
        f0 = np.floor((CENT[i] / (FS / 2)) * half)
        bw = (BANDWIDTH[i] / (FS / 2)) * half
        v = np.exp(-11 * (((j - f0) / bw) ** 2) + (np.log(BANDWIDTH[0]) - np.log(BANDWIDTH[i])))
        margin = min(margin, float(np.abs(v / MIN_FACTOR - 1).min()))
        out[i] = v * (v > MIN_FACTOR)
    return out, margin


def _frames(x: np.ndarray, F: int) -> np.ndarray:
    idx = np.arange(F)[:, None] * HOP + np.arange(WIN)[None, :]
    return x[idx]


def lpc(fr: np.ndarray, backwards: bool = False):
    """[F, 480] windowed frames -> (lpparams float32 [F, 17], lags float32 [F, 17]); the recursion in float64, the sums as numpy takes them.
    ``backwards``: each lag's products summed from the frame's end — the same numbers in another order, for ``llr_order_spread``"""
    F = fr.shape[0]
    flip = slice(None, None, -1) if backwards else slice(None)
    R = np.stack([np.sum(np.ascontiguousarray((fr[:, : WIN - k] * fr[:, k:])[:, flip]), axis=1) for k in range(ORDER + 1)], axis=1)
    a = np.ones((F, ORDER))
    E = R[:, 0].copy()
    for i in range(ORDER):
        past = a[:, :i].copy()
        s = np.sum(np.ascontiguousarray(past * R[:, i:0:-1]), axis=1) if i else np.zeros(F)
        rc = (R[:, i + 1] - s) / np.maximum(E, EPS)
        a[:, i] = rc
        if i:
            a[:, :i] = past - rc[:, None] * past[:, ::-1]
        E = (1 - rc * rc) * E
    lp = np.concatenate([np.ones((F, 1)), -a], axis=1).astype(np.float32)
    return lp, R.astype(np.float32)


def toeplitz_form(a32: np.ndarray, r32: np.ndarray) -> np.ndarray:
    """a' T(R) a per frame, float64 arithmetic on the float32-rounded values"""
    a, R = a32.astype(np.float64), r32.astype(np.float64)
    idx = np.abs(np.arange(ORDER + 1)[:, None] - np.arange(ORDER + 1)[None, :])
    t = np.einsum("fij,fj->fi", R[:, idx], a)
    return np.sum(a * t, axis=1)


def loc_peaks(slope, energy):
    """-> (peaks [24], ran off the top, ran off the bottom)"""
    out = np.zeros(NB - 1)
    up = down = False
    for ii in range(NB - 1):
        n = ii
        if slope[ii] > 0:
            while n < NB - 1 and slope[n] > 0:
                n += 1
            up |= n == NB - 1
            out[ii] = energy[n - 1]
        else:
            while n >= 0 and slope[n] <= 0:
                n -= 1
            down |= n < 0
            out[ii] = energy[n + 1]
    return out, up, down


def _band_spectra(x: np.ndarray, F: int) -> np.ndarray:
    """|FFT_1024| of the windowed frames of x + eps, bins 0..511: [F, 512]"""
    return np.abs(np.fft.rfft(_frames(x + EPS, F) * hann(), n=NFFT, axis=1))[:, : NFFT // 2]


def trimmed_mean(v: np.ndarray, K: int) -> float:
    return float(np.mean(np.sort(v)[:K]))


def sepm(clean, processed, sr: int = FS, resample=None) -> dict:
    c, p = np.asarray(clean), np.asarray(processed)
    assert c.shape == p.shape and c.ndim == 1
    if int(sr) != FS:
        c, p = resample(c.astype(np.float32), int(sr), FS), resample(p.astype(np.float32), int(sr), FS)
    c, p = c.astype(np.float64), p.astype(np.float64)
    F = n_frames(c.shape[0])
    K = trim_count(F)
    nan = float("nan")
    if F < 1:
        return {"ssnr": nan, "llr": nan, "wss": nan, "fwsnr": nan, "F": 0, "K": 0, "runoff_up": 0, "runoff_down": 0, "min_frac": nan, "llr_order_spread": 0.0}
    w = hann()
    cf, pf = _frames(c, F) * w, _frames(p, F) * w
    # segmental SNR
    snr = 10 * np.log10((cf ** 2).sum(1) / (((cf - pf) ** 2).sum(1) + EPS) + EPS)
    ssnr = float(np.mean(np.clip(snr, -10, 35)))
    # LLR
    ac, rc = lpc(cf)
    ap, _ = lpc(pf)
    frac = toeplitz_form(ap, rc) / (toeplitz_form(ac, rc) + EPS)
    live = rc[:, 0] != 0                       # (an all-zero clean frame gives 0 / eps exactly)
    min_frac = float(np.abs(frac[live]).min()) if live.any() else float("inf")
    frac = np.where(frac <= 0, 1000.0, frac)
    llr = trimmed_mean(np.log(frac), K)
    # the same with every lag summed in the opposite order: how far float64 rounding in the lags alone moves the value (the coefficients are
    # rounded to float32 behind an ill-conditioned recursion, so a last-bit change of a lag can move one of them by a float32 ulp)
    bc, rb = lpc(cf, backwards=True)
    bp, _ = lpc(pf, backwards=True)
    fb = toeplitz_form(bp, rb) / (toeplitz_form(bc, rb) + EPS)
    spread = abs(trimmed_mean(np.log(np.where(fb <= 0, 1000.0, fb)), K) - llr)
    # the two spectral measures
    crit, _ = crit_filter()
    sc, sp = _band_spectra(c, F), _band_spectra(p, F)
    ec, ep = 10 * np.log10((sc ** 2) @ crit.T), 10 * np.log10((sp ** 2) @ crit.T)
    ec, ep = np.maximum(ec, -100.0), np.maximum(ep, -100.0)
    dc, dp = np.diff(ec, axis=1), np.diff(ep, axis=1)
    dist = np.zeros(F)
    ups = downs = 0
    for f in range(F):
        pc, u1, d1 = loc_peaks(dc[f], ec[f])
        pp, u2, d2 = loc_peaks(dp[f], ep[f])
        ups += int(u1 or u2)
        downs += int(d1 or d2)
        wc = (20.0 / (20.0 + ec[f].max() - ec[f, :-1])) * (1.0 / (1.0 + pc - ec[f, :-1]))
        wp = (20.0 / (20.0 + ep[f].max() - ep[f, :-1])) * (1.0 / (1.0 + pp - ep[f, :-1]))
        ww = (wc + wp) / 2.0
        dist[f] = np.sum(ww * (dc[f] - dp[f]) ** 2) / np.sum(ww)
    wss = trimmed_mean(dist, K)
    nc, npr = (sc / sc.sum(1, keepdims=True)) @ crit.T, (sp / sp.sum(1, keepdims=True)) @ crit.T
    err = np.maximum((nc - npr) ** 2, EPS)
    wf = nc ** 0.2
    fw = np.sum(wf * (10 * np.log10(nc ** 2 / err)), axis=1) / np.sum(wf, axis=1)
    fwsnr = float(np.mean(np.clip(fw, -10, 35)))
    return {"ssnr": ssnr, "llr": llr, "wss": wss, "fwsnr": fwsnr, "F": F, "K": K, "runoff_up": ups, "runoff_down": downs, "min_frac": min_frac,
            "llr_order_spread": spread}


def composite(m: dict, pesq: float) -> dict:
    """sepm.py:501-510 from the measures and a caller's PESQ value"""
    def lim(v):
        return min(5.0, max(1.0, v))

    return {"pesq": pesq,
            "csig": lim(3.093 - 1.029 * m["llr"] + 0.603 * pesq - 0.009 * m["wss"]),
            "cbak": lim(1.634 + 0.478 * pesq - 0.007 * m["wss"] + 0.063 * m["ssnr"]),
            "covl": lim(1.594 + 0.805 * pesq - 0.512 * m["llr"] - 0.007 * m["wss"]),
            "ssnr": m["ssnr"], "llr": m["llr"], "wss": m["wss"]}
