"""A plain numpy restatement of the reference's scores, one clip at a time, in float64 or float32:

    si_sdr(reference, estimate)              df/evaluation_utils.py:599-619 (si_sdr_speechmetrics)
    stoi(clean, degraded, sr) -> value, info df/stoi.py:163-231 (remove_silent_frames :35-110, thirdoct :113-143, _stft :146-160)

``info`` is what ``deepfilternet_amd.metrics.stoi(return_info=True)`` reports: windows examined, windows kept, STFT frames L, segments J
(L = J = 0 where the reference skips the clip, stoi.py:195-197; the value is NaN there).  ``margin`` is the smallest
``|max(e) - 40 - e[w]|`` over the clip's windows in dB: how far the silent-frame mask is from flipping.

Test code: the product computes none of this on the host."""
from __future__ import annotations

import numpy as np

FS, DYN_RANGE, N_FRAME, N_FFT, N_BANDS, MIN_FREQ, N_SEG, BETA = 10_000, 40, 256, 512, 15, 150, 30, -15.0
EPS = np.finfo("float").eps


def si_sdr(reference, estimate, dtype=np.float64, eps=np.finfo(np.float32).eps) -> float:
    """The formula in ``dtype`` arithmetic; ``eps`` is that of the INPUT's type in the reference (float32 audio: float32's)."""
    r = np.asarray(reference, dtype=dtype).reshape(-1, 1)
    e = np.asarray(estimate, dtype=dtype).reshape(-1, 1)
    eps = dtype(eps)
    rss = np.dot(r.T, r)
    a = (eps + np.dot(r.T, e)) / (rss + eps)
    e_true = a * r
    e_res = e - e_true
    sss, snn = (e_true ** 2).sum(), (e_res ** 2).sum()
    return float(10 * np.log10((eps + sss) / (eps + snn)))


def thirdoct(fs=FS, nfft=N_FFT, num_bands=N_BANDS, min_freq=MIN_FREQ):
    """stoi.py:113-143 -> (obm [bands, nfft / 2 + 1], [(lo, hi)] per band)"""
    f = np.linspace(0, fs, nfft + 1)[: nfft // 2 + 1]
    k = np.arange(num_bands).astype(float)
    lo_f = min_freq * np.power(2.0, (2 * k - 1) / 6)
    hi_f = min_freq * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((num_bands, len(f)))
    edges = []
    for i in range(num_bands):
        lo = int(np.argmin(np.square(f - lo_f[i])))
        hi = int(np.argmin(np.square(f - hi_f[i])))
        obm[i, lo:hi] = 1
        edges.append((lo, hi))
    return obm, edges


def _hann(dtype):
    n = np.arange(N_FRAME + 2, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * np.pi * n / (N_FRAME + 1)))[1:-1].astype(dtype)


def remove_silent_frames(x, y, dtype):
    """stoi.py:35-110 for one clip -> (x, y without silent frames, windows, kept, margin in dB)"""
    hop = N_FRAME // 2
    pad = N_FRAME - x.shape[0] % N_FRAME
    pad_front = pad // 2
    pad_end = pad - pad_front
    x = np.concatenate([np.zeros(pad_front, dtype), x, np.zeros(pad_end, dtype)])
    y = np.concatenate([np.zeros(pad_front, dtype), y, np.zeros(pad_end, dtype)])
    w = _hann(dtype)
    nw = (x.shape[0] - N_FRAME + hop) // hop
    idx = np.arange(nw)[:, None] * hop + np.arange(N_FRAME)[None, :]
    x_w, y_w = x[idx] * w, y[idx] * w
    e = 20 * np.log10(np.sqrt((x_w * x_w).sum(1, dtype=dtype)) / dtype(np.sqrt(N_FRAME)) + dtype(EPS))
    d = e.max() - dtype(DYN_RANGE) - e
    mask = d < 0
    margin = float(np.abs(d.astype(np.float64)).min())
    x_w, y_w = x_w[mask], y_w[mask]
    k = int(mask.sum())
    n = (k - 1) * hop + N_FRAME
    xs, ys, ws = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    for i in range(k):
        xs[i * hop: i * hop + N_FRAME] += x_w[i]
        ys[i * hop: i * hop + N_FRAME] += y_w[i]
        ws[i * hop: i * hop + N_FRAME] += w
    xs, ys = xs / ws, ys / ws
    if mask[0]:
        xs, ys = xs[pad_front:], ys[pad_front:]
    if mask[-1]:
        xs, ys = xs[:-pad_end], ys[:-pad_end]
    return xs, ys, nw, k, margin


def _band_env(x, obm, dtype):
    """_stft (win 256 in the middle of 512, hop 128, / sum(w)) -> power -> third-octave bands -> sqrt: [bands, L]"""
    w = _hann(dtype)
    L = (x.shape[0] - N_FRAME) // (N_FRAME // 2) + 1
    idx = np.arange(L)[:, None] * (N_FRAME // 2) + np.arange(N_FRAME)[None, :]
    fr = np.zeros((L, N_FFT), dtype)
    fr[:, (N_FFT - N_FRAME) // 2: (N_FFT + N_FRAME) // 2] = x[idx] * w
    spec = np.fft.rfft(fr.astype(np.float64), axis=1)
    spec = spec / np.float64(w.sum(dtype=dtype))
    p = (spec.real.astype(dtype) ** 2 + spec.imag.astype(dtype) ** 2).T          # [F, L]
    return np.sqrt(np.matmul(obm.astype(dtype), p))


def stoi(clean, degraded, sr: int, dtype=np.float64, resample=None):
    """-> (value, info [4] int32, margin).  ``resample(x float32, sr, 10000) -> float32`` is used when sr != 10000 (the library's
    resampler has its own oracle, oracle.io_oracle.resample, which is the default)."""
    x, y = np.asarray(clean), np.asarray(degraded)
    assert x.shape == y.shape and x.ndim == 1
    if int(sr) != FS:
        if resample is None:
            from oracle.io_oracle import resample
        x, y = resample(x.astype(np.float32), int(sr), FS), resample(y.astype(np.float32), int(sr), FS)
    x, y = x.astype(dtype), y.astype(dtype)
    obm, _ = thirdoct()
    xs, ys, nw, k, margin = remove_silent_frames(x, y, dtype)
    if xs.shape[0] < N_FFT:
        return float("nan"), np.array([nw, k, 0, 0], np.int32), margin
    xb, yb = _band_env(xs, obm, dtype), _band_env(ys, obm, dtype)
    L = xb.shape[1]
    if L > N_SEG:
        seg = np.arange(L - N_SEG + 1)[:, None] + np.arange(N_SEG)[None, :]
        xq, yq = xb[:, seg].transpose(1, 2, 0), yb[:, seg].transpose(1, 2, 0)     # [J, N, bands]
    else:
        xq, yq = xb.T[None], yb.T[None]
    eps = dtype(EPS)

    def norm(v):
        return np.sqrt((v * v).sum(1, keepdims=True, dtype=dtype))

    yq = yq * (norm(xq) / (norm(yq) + eps))
    yq = np.minimum(yq, xq * dtype(1 + 10 ** (-BETA / 20)))
    yq = yq - yq.mean(1, keepdims=True, dtype=dtype)
    xq = xq - xq.mean(1, keepdims=True, dtype=dtype)
    xq = xq / (norm(xq) + eps)
    yq = yq / (norm(yq) + eps)
    J = xq.shape[0]
    return float((xq * yq).sum(dtype=dtype) / dtype(N_BANDS * J)), np.array([nw, k, L, J], np.int32), margin
