#!/usr/bin/env python3
"""Writes tests/golden/sepm.npz: the reference's own ``df/sepm.py`` (SNRseg, llr, wss, fwSNRseg) on clips that reach its branches, at 16 kHz, on
this machine's CPU.  ``sepm.py`` imports the third-party ``pesq`` package, which is not installed: the tool puts a stub module into
``sys.modules`` first (PESQ is no part of the fixture).

Each clip is 16-bit PCM (the fixture stores the int16 samples; the input is float32(sample) / 32768, which numpy promotes to float64 as it does
for the reference's callers).  Stored per case: clean, processed (int16); ``ssnr``, ``llr``, ``wss``, ``fwsnr`` — the reference's float64
results, NaN where it raises or averages nothing (fewer than 600 samples) —; ``info`` = F frames, K = int(round(0.95 F)); and for LLR, whose two
17 x 17 quadratic forms the reference takes in float32 in its BLAS's order, ``llr.f64`` — the same function with the forms taken in float64 from
the reference's own float32-rounded ``lpcoeff`` results — and the bar ``llr.tol = max(16 |llr - llr.f64|, 1e-6)``.

Conditions the tool asserts, so that no implementation's rounding can change a branch:
  * llr.tol <= 1e-4;
  * no frame's num / den lies within 1e-3 of 0 (the ``frac <= 0 -> 1000`` branch), all-zero clean frames aside, where it is 0 / eps exactly;
  * no critical-band tap lies within 1e-9 (relative) of the -30 dB cut;
  * the high-passed and the low-passed clip make findLocPeaks run off the top and the bottom band.

    python tools/gen_golden_sepm.py        (needs the reference tree)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import sepm_ref as R  # noqa: E402  (before the reference tree, which has a `tests` package of its own, joins sys.path)
from tools.ref_import import install_shims, reference_available  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "sepm.npz")
FS = 16_000


def install_pesq_stub() -> None:
    if "pesq" not in sys.modules:
        m = types.ModuleType("pesq")

        def pesq(*a, **k):
            raise RuntimeError("pesq is not installed: the stub of tools/gen_golden_sepm.py")

        m.pesq = pesq
        sys.modules["pesq"] = m


def noise(n: int, seed: int, amp: float = 0.2, kind: str = "ma8") -> np.ndarray:
    r = np.random.default_rng(seed)
    v = r.standard_normal(n + 16)
    if kind == "ma8":
        x = np.convolve(v, np.ones(8) / 8, mode="valid")[:n]
    elif kind == "high":
        x = np.diff(v)[:n]
    else:   # "low": one pole
        x = np.zeros(n + 16)
        s = 0.0
        for i, u in enumerate(v):
            s = 0.9 * s + u
            x[i] = s
        x = x[16:16 + n]
    return amp * x / np.abs(x).max() * (1 + 0.5 * np.sin(np.arange(n) / 300.0 + seed)) / 1.5


def pcm(x: np.ndarray) -> np.ndarray:
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def clip(n: int, seed: int, quiet=(), kind="ma8", mode="noisy"):
    x = noise(n, seed, kind=kind)
    for a, b in quiet:
        x[a:b] *= 1e-4
    xi = pcm(x)
    yi = pcm(xi / 32768.0 + noise(n, seed + 1000, 0.06))
    if mode == "identical":
        yi = xi.copy()
    elif mode == "zero_est":
        yi = np.zeros_like(xi)
    elif mode == "zero_clean":
        xi = np.zeros_like(xi)
    return xi, yi


# name -> (samples, seed, quiet sections, spectrum, mode)
CASES = {
    "n599": (599, 1, (), "ma8", "noisy"),                 # F = 0: every score NaN
    "n600": (600, 2, (), "ma8", "noisy"),                 # F = K = 1
    "n719": (719, 3, (), "ma8", "noisy"),                 # still one frame
    "n720": (720, 4, (), "ma8", "noisy"),                 # two
    "F10": (480 + 10 * 120 + 7, 5, (), "ma8", "noisy"),   # K = round(9.5) = 10
    "F30": (480 + 30 * 120 + 119, 6, (), "ma8", "noisy"),  # K = round(28.5) = 28
    "F50": (480 + 50 * 120, 7, (), "ma8", "noisy"),       # K = round(47.5) = 48
    "F70": (480 + 70 * 120 + 60, 8, (), "ma8", "noisy"),  # K = round(66.5) = 66
    "quiet_sections": (6000, 9, ((1000, 2200), (4000, 4700)), "ma8", "noisy"),
    "identical": (4000, 10, (), "ma8", "identical"),
    "zero_est": (4000, 11, (), "ma8", "zero_est"),
    "zero_clean": (4000, 12, (), "ma8", "zero_clean"),
    "highpass": (5000, 13, (), "high", "noisy"),
    "lowpass": (5000, 14, (), "low", "noisy"),
}


def reference_case(xi: np.ndarray, yi: np.ndarray):
    from df import sepm as S  # type: ignore

    c, p = xi.astype(np.float32) / np.float32(32768.0), yi.astype(np.float32) / np.float32(32768.0)
    F = R.n_frames(len(c))
    res = {"info": np.array([F, R.trim_count(F)], np.int32)}
    for key, fn in (("ssnr", S.SNRseg), ("llr", S.llr), ("wss", S.wss), ("fwsnr", S.fwSNRseg)):
        try:
            with np.errstate(all="ignore"):
                v = fn(c, p, FS)
            res[key] = float("nan") if v is None else float(v)
        except ValueError:
            res[key] = float("nan")
    if F < 1:
        assert all(res[k] != res[k] for k in ("ssnr", "llr", "wss", "fwsnr")), res
        res["llr.f64"], res["min_frac"] = float("nan"), float("nan")
        return res
    # LLR once more, the reference's own frames and lpcoeff, the two forms in float64
    w = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, 481) / 481))
    cf, pf = S.extractOverlappedWindows(c, 480, 360, w), S.extractOverlappedWindows(p, 480, 360, w)
    idx = np.abs(np.arange(17)[:, None] - np.arange(17)[None, :])
    fr = np.zeros(cf.shape[0] - 1)
    live = np.zeros(cf.shape[0] - 1, bool)
    for i in range(cf.shape[0] - 1):
        ac, rc = S.lpcoeff(cf[i], 16)
        ap, _ = S.lpcoeff(pf[i], 16)
        T = rc.astype(np.float64)[idx]
        a, b = ap.astype(np.float64), ac.astype(np.float64)
        fr[i] = a.dot(T.dot(a)) / (b.dot(T.dot(b)) + np.finfo(np.float64).eps)
        live[i] = rc[0] != 0
    assert len(fr) == F
    res["min_frac"] = float(np.abs(fr[live]).min()) if live.any() else float("inf")
    fr[fr <= 0] = 1000
    res["llr.f64"] = float(np.mean(np.sort(np.log(fr))[: int(round(len(fr) * 0.95))]))
    return res


def main() -> int:
    if not reference_available():
        print("gen_golden_sepm: the reference tree is not present")
        return 2
    install_shims()
    install_pesq_stub()
    _, tap_margin = R.crit_filter()
    assert tap_margin > 1e-9, f"a critical-band tap {tap_margin:.2e} (relative) from the cut"
    out = {"names": np.array(list(CASES))}
    for name, (n, seed, quiet, kind, mode) in CASES.items():
        xi, yi = clip(n, seed, quiet, kind, mode)
        r = reference_case(xi, yi)
        tol = max(16.0 * abs(r["llr"] - r["llr.f64"]), 1e-6) if r["llr"] == r["llr"] else 0.0
        assert tol <= 1e-4, f"{name}: LLR bar {tol}"
        assert not r["min_frac"] < 1e-3, f"{name}: a frame's frac {r['min_frac']:.2e} from 0"
        if name in ("highpass", "lowpass"):
            m = R.sepm(xi.astype(np.float32) / np.float32(32768.0), yi.astype(np.float32) / np.float32(32768.0))
            assert m["runoff_up"] > 0 and m["runoff_down"] > 0, (name, m["runoff_up"], m["runoff_down"])
        out[f"{name}.clean"], out[f"{name}.processed"] = xi, yi
        for k in ("ssnr", "llr", "wss", "fwsnr", "llr.f64"):
            out[f"{name}.{k}"] = np.float64(r[k])
        out[f"{name}.llr.tol"], out[f"{name}.info"] = np.float64(tol), r["info"]
        print(f"{name:16s} n {n:5d} info {r['info'].tolist()} ssnr {r['ssnr']:.9f} llr {r['llr']:.9f} |llr - f64| {abs(r['llr'] - r['llr.f64']):.2e} "
              f"bar {tol:.1e} wss {r['wss']:.9f} fwsnr {r['fwsnr']:.9f} min frac {r['min_frac']:.3g}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
