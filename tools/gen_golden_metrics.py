#!/usr/bin/env python3
"""Writes tests/golden/metrics.npz: the reference's own ``df.stoi.stoi`` (imported through tools/ref_import.py) on clips that reach every branch
of it, at fs_source = 10000, where the shimmed ``df.io.resample`` is the identity — the STOI core pinned with no resampler in between.

Each clip is amplitude-modulated low-passed noise, 16-bit PCM (the fixture stores the int16 samples; the float input is sample / 32768), with
sections scaled by 1e-4 so that their windows fall under the 40 dB silent-frame threshold.  The reference runs on every clip ALONE (a batch of
one: the library defines a row of a batch as that), in float64 and in float32.  Stored per case: clean, degraded (int16), the float64 and float32
results (NaN where the reference skips the clip and leaves its output uninitialised), info = windows examined, windows kept, STFT frames L,
segments J (read off the reference's intermediate tensors), and the bar for an implementation in float32 against the float64 value,
max(16 |ref32 - ref64|, 1e-6).

The silent-frame mask is a threshold: the generator asserts that every window of every clip is more than 0.5 dB away from it in float64, so
that no implementation's rounding can flip one.

    python tools/gen_golden_metrics.py        (needs the reference tree)
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.ref_import import install_shims, reference_available  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "metrics.npz")
MIN_MARGIN_DB = 0.5


def noise(n: int, seed: int, amp: float = 0.2) -> np.ndarray:
    r = np.random.default_rng(seed)
    x = np.convolve(r.standard_normal(n + 16), np.ones(8) / 8, mode="valid")[:n]
    return amp * x / np.abs(x).max() * (1 + 0.5 * np.sin(np.arange(n) / 300.0 + seed)) / 1.5


def pcm(x: np.ndarray) -> np.ndarray:
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def clip(n: int, seed: int, quiet=(), degraded="noisy"):
    """-> (clean, degraded) int16; quiet: [(from, to)] sections of the clean signal scaled by 1e-4"""
    x = noise(n, seed)
    for a, b in quiet:
        x[a:b] *= 1e-4
    if degraded == "zero_clean":
        x[:] = 0.0
    xi = pcm(x)
    yi = xi.copy() if degraded == "same" else pcm(xi / 32768.0 + noise(n, seed + 1000, 0.06))
    return xi, yi


# name -> (samples, seed, quiet sections, degraded); the comments name the branch a case is there for
CASES = {
    "mult256_nothing_removed": (5120, 1, (), "noisy"),                 # pad = 256; first and last window kept; the silence-free signal is the input
    "odd_pad_gap": (6001, 2, ((2000, 3000),), "noisy"),                # pad = 143; a gap in the middle
    "first_removed_last_kept": (5000, 3, ((0, 700),), "noisy"),
    "first_kept_last_removed": (5000, 4, ((4300, 5000),), "noisy"),
    "first_removed_last_removed": (5000, 5, ((0, 600), (4400, 5000)), "noisy"),
    "L31": (4100, 6, (), "noisy"),                                     # J = 2
    "L30": (4000, 7, (), "noisy"),                                     # one segment of exactly 30 frames
    "L29": (3900, 8, (), "noisy"),                                     # (below the 4000 of the other clips: nothing removed, 29 frames)
    "L6": (4500, 9, ((0, 1500), (2060, 4500)), "noisy"),               # one segment of 6 frames
    "too_short": (4500, 10, ((0, 2000), (2080, 4500)), "noisy"),       # fewer than 512 samples left: skipped
    "zero_clean": (4500, 11, (), "zero_clean"),                        # the reference gives exactly 0
    "same": (7000, 12, ((5000, 5600),), "same"),                       # degraded == clean
}


def reference_case(xi: np.ndarray, yi: np.ndarray):
    import torch
    from df import stoi as S  # type: ignore

    res = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        x = (torch.from_numpy(xi.astype(np.float64)) / 32768.0).to(dt).unsqueeze(0)
        y = (torch.from_numpy(yi.astype(np.float64)) / 32768.0).to(dt).unsqueeze(0)
        out = S.stoi(x, y, 10_000)
        xs, _ = S.remove_silent_frames(x, y, 40, 256, 128)
        n = int(xs[0].numel())
        skipped = n < 512
        res[name] = float("nan") if skipped else float(out[0])
        if name == "f64":
            # the integers, and the mask's distance from flipping, from the reference's own intermediate values
            pad = 256 - x.shape[1] % 256
            xp = torch.nn.functional.pad(x, (pad // 2, pad - pad // 2)).t()
            w = torch.hann_window(258, periodic=False, dtype=dt)[1:-1].view(-1, 1)
            x_w = S.as_windowed(xp, 256, 128) * w
            e = 20 * torch.log10(x_w.norm(dim=1) / np.sqrt(256) + S.EPS)
            d = (torch.max(e, dim=0)[0] - 40 - e)[:, 0]
            windows, kept = int(d.numel()), int((d < 0).sum())
            L = 0 if skipped else (n - 256) // 128 + 1
            J = 0 if skipped else (L - 29 if L > 30 else 1)
            res["info"] = np.array([windows, kept, L, J], np.int32)
            res["margin"] = float(d.abs().min())
            res["first_last"] = (bool(d[0] < 0), bool(d[-1] < 0))
    return res


def main() -> int:
    if not reference_available():
        print("gen_golden_metrics: the reference tree is not present")
        return 2
    install_shims()
    out = {"names": np.array(list(CASES))}
    for name, (n, seed, quiet, degraded) in CASES.items():
        xi, yi = clip(n, seed, quiet, degraded)
        r = reference_case(xi, yi)
        assert r["margin"] > MIN_MARGIN_DB, f"{name}: a window {r['margin']:.3f} dB from the silent-frame threshold"
        tol = max(16.0 * abs(r["f32"] - r["f64"]), 1e-6) if r["f64"] == r["f64"] else 0.0
        assert tol <= 1e-4, f"{name}: bar {tol} looser than test_df's 1e-4"
        out[f"{name}.clean"], out[f"{name}.degraded"] = xi, yi
        out[f"{name}.f64"], out[f"{name}.f32"], out[f"{name}.tol"] = np.float64(r["f64"]), np.float64(r["f32"]), np.float64(tol)
        out[f"{name}.info"], out[f"{name}.margin"] = r["info"], np.float64(r["margin"])
        print(f"{name:28s} n {n:5d} pad {256 - n % 256:3d} info {r['info'].tolist()} first/last kept {r['first_last']} margin {r['margin']:6.2f} dB "
              f"f64 {r['f64']:.12f} |f32 - f64| {abs(r['f32'] - r['f64']):.2e} bar {tol:.2e}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
