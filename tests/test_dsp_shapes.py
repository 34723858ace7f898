"""Every kind of transform dfx_state_create accepts, on both backends, against the float64 restatement oracle/dsp64.py.

The other DSP tests run six (fft, hop) pairs, all with an even hop and an even M = fft / 2 of 48 ... 480.  SHAPES below adds what the kernels
also accept and the suite never ran: odd M (the real post-pass pairs bin k with M - k and then has no self-paired bin), plans of 0, 1, 2, 5 and 6
Stockham passes (the result buffer alternates with the pass count), plans of radix 3 or 5 only, M below the 64 lanes of a frame's wave, odd hops
(every second frame misses the 8-byte alignment test of dfx_k_analysis), hops that do not divide the size, 3 to 8 overlapping frames (with 8,
dfx_k_synthesis emits one frame per chunk), the in-place 480-point plan at other hops, and the largest size whose LDS carve fits a workgroup.

The bound is tests/helpers.py hold_to_f64: |kernel - dsp64| <= 4 * max(E32, 2^-23 max|dsp64|) with E32 = |C oracle - dsp64| over the case; the
ratio is printed per case (pytest -s) and docs/measurements.md records the GPU's.  test_dsp64_matches_c_oracle pins the restatement itself.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import dsp64 as R
from oracle import libdf_oracle as L
from tests.helpers import hold_to_f64

SR = 48000


def _nb(N):
    return max(1, min(8, (N // 2 + 1) // 2))


# (fft, hop, ERB bands): what the entry is the first to reach.  M = fft / 2; the plan takes radix 4, then 2, 3, 5.
SHAPES = [
    (2, 1, _nb(2)),          # M = 1: a plan of no pass at all, one bin pair (DC, Nyquist) only; hop 1
    (4, 2, _nb(4)),          # M = 2: one radix-2 pass
    (4, 1, _nb(4)),          # four overlapping frames, odd hop
    (6, 3, _nb(6)),          # M = 3: one radix-3 pass, odd M (no self-paired bin)
    (10, 5, _nb(10)),        # M = 5: one radix-5 pass
    (12, 4, _nb(12)),        # M = 6: passes 2, 3; three overlapping frames
    (30, 15, _nb(30)),       # M = 15: passes 3, 5 (no power of two), odd hop at two frames
    (30, 7, _nb(30)),        # five overlapping frames, a hop that does not divide the size
    (50, 25, _nb(50)),       # M = 25: radix 5 only, two passes
    (90, 45, _nb(90)),       # M = 45: three odd passes
    (90, 13, _nb(90)),       # seven overlapping frames
    (162, 81, _nb(162)),     # M = 81: radix 3 only, four passes; M above the 64 lanes and odd
    (250, 125, _nb(250)),    # M = 125: radix 5 only, three passes
    (450, 225, _nb(450)),    # M = 225: passes 3, 3, 5, 5
    (486, 243, _nb(486)),    # M = 243: radix 3 only, five passes
    (640, 80, _nb(640)),     # eight overlapping frames: one output frame per synthesis chunk; passes 4, 4, 4, 5
    (640, 81, _nb(640)),     # eight overlapping frames with an odd hop that does not divide the size
    (960, 400, _nb(960)),    # the in-place 480-point plan with a hop that does not divide the size
    (960, 320, _nb(960)),    # the in-place plan with three overlapping frames
    (960, 137, _nb(960)),    # the in-place plan with eight overlapping frames and an odd hop
    (1024, 512, 64),         # M = 512: passes 4, 4, 4, 4, 2; 513 bins (a frame no longer fits one round of eight loads per lane); 64 bands: segment tables
    (1250, 625, 80),         # M = 625: radix 5 only, four passes; more than 64 bands: no segment table, the second round of lanes
    (1458, 729, _nb(1458)),  # M = 729: radix 3 only, six passes
    (2048, 1024, _nb(2048)),  # the largest power of two whose LDS carve fits a workgroup (155 904 bytes and the band tables)
    (2048, 256, _nb(2048)),   # the same with eight overlapping frames
]
IDS = [f"{n}_{h}_{e}" for n, h, e in SHAPES]
CUTS = (0, 1, 3, 4, 11)   # one long call against the same stream cut at these frames


@functools.lru_cache(maxsize=None)
def reference(N, hop, nb):
    """Inputs, the C oracle's results and dsp64's for one shape; computed once and left unchanged."""
    rng = np.random.default_rng([N, hop, nb])
    F = N // 2 + 1
    x = (0.3 * rng.standard_normal((3, 11 * hop + 3))).astype(np.float32)
    Y = (rng.standard_normal((2, 11, F)) + 1j * rng.standard_normal((2, 11, F))).astype(np.complex64)
    o = L.DF(SR, N, hop, nb, 1)
    widths = o.erb_widths()
    assert int(widths.sum()) == F
    nb_df = min(96, F)
    from deepfilternet_amd.config import ModelParams

    alpha = ModelParams(sr=SR, hop_size=hop).norm_alpha()   # (as df_features takes it)
    c = {"spec": o.analysis(x), "y": o.synthesis(Y.copy())}
    c["erb"] = L.erb(c["spec"], widths)
    c["fe"] = L.erb_norm(c["erb"].copy(), alpha)
    c["fs"] = L.unit_norm(np.ascontiguousarray(c["spec"][..., :nb_df]), alpha)
    r = {"spec": R.analysis(x, N, hop)[0], "y": R.synthesis(Y, N, hop)[0]}
    r["erb"] = R.erb_db(r["spec"], widths)
    r["fe"] = R.erb_norm(r["erb"], alpha)[0]
    r["fs"] = R.unit_norm(r["spec"][..., :nb_df], alpha)[0]
    for v in list(c.values()) + list(r.values()) + [x, Y]:
        v.setflags(write=False)
    return {"x": x, "Y": Y, "widths": widths, "nb_df": nb_df, "alpha": alpha, "c": c, "r": r}


@pytest.mark.parametrize("N,hop,nb", SHAPES, ids=IDS)
def test_dsp64_matches_c_oracle(N, hop, nb):
    """The restatement against the C oracle, per stage: |C oracle - dsp64| <= 1e-6 max|dsp64|.  (Float32's own error is a few 1e-7 of the
    scale; a wrong restatement — the window over N instead of N / 2, say — sits at 1e-2 or more.)"""
    ref = reference(N, hop, nb)
    c, a, w = ref["c"], ref["alpha"], ref["widths"]
    # per stage: every stage of the restatement is given what the C oracle's stage was given (float32 values are exact in float64), so that a
    # stage's deviation is its own and not what a one-bin band's logarithm makes of the spectrum's
    low = np.ascontiguousarray(c["spec"][..., :ref["nb_df"]])
    pairs = {
        "spec": (c["spec"], ref["r"]["spec"]),
        "y": (c["y"], ref["r"]["y"]),
        "erb": (c["erb"], R.erb_db(c["spec"], w)),
        "erb power": (L.erb(c["spec"], w, False), R.erb_db(c["spec"], w, db=False)),
        "erb_norm": (L.erb_norm(c["erb"].copy(), a), R.erb_norm(c["erb"], a)[0]),
        "unit_norm": (L.unit_norm(low, a), R.unit_norm(low, a)[0]),
    }
    for k, (c32, r64) in pairs.items():
        assert c32.shape == r64.shape, k
        d, scale = float(np.abs(c32 - r64).max()), float(np.abs(r64).max())
        print(f"  {N}/{hop} {k}: |C - f64| = {d:.2e} = {d / scale:.2e} of max|f64|")
        assert d <= 1e-6 * scale, (k, d, scale)
    # the memories the two directions hand on, and a call that starts from them
    x, Y = ref["x"], ref["Y"]
    cut = 4 * hop
    s0, m0 = R.analysis(x[:, :cut], N, hop)
    s1, _ = R.analysis(x[:, cut:], N, hop, m0)
    assert np.abs(np.concatenate([s0, s1], 1) - ref["r"]["spec"]).max() <= 1e-12 * np.abs(ref["r"]["spec"]).max()
    y0, m0 = R.synthesis(Y[:, :4], N, hop)
    y1, _ = R.synthesis(Y[:, 4:], N, hop, m0)
    assert np.abs(np.concatenate([y0, y1], 1) - ref["r"]["y"]).max() <= 1e-12 * np.abs(ref["r"]["y"]).max()
    # the two scans: the state after 4 frames, fed into a second call, continues the scan
    e = R.erb_db(c["spec"], w)
    e0, s0 = R.erb_norm(e[:, :4], a)
    assert np.abs(np.concatenate([e0, R.erb_norm(e[:, 4:], a, s0)[0]], 1) - R.erb_norm(e, a)[0]).max() <= 1e-12
    u0, s0 = R.unit_norm(low[:, :4], a)
    u = R.unit_norm(low, a)[0]
    assert np.abs(np.concatenate([u0, R.unit_norm(low[:, 4:], a, s0)[0]], 1) - u).max() <= 1e-12 * np.abs(u).max()


def _libdf():
    from deepfilternet_amd import libdf

    return libdf


@pytest.mark.parametrize("N,hop,nb", SHAPES, ids=IDS)
def test_transforms_hold_to_float64(backend, N, hop, nb):
    """analysis, synthesis and the fused features of df_features (the spectrum, the ERB feature in dB through its norm, the unit-normed bins) at
    every shape of the table; then one long call against the same stream cut at frames 1, 3, 4 and 11 with reset=False, both directions."""
    from deepfilternet_amd.enhance import df_features

    D = _libdf()
    ref = reference(N, hop, nb)
    x, Y, c, r = ref["x"], ref["Y"], ref["c"], ref["r"]
    tag = f"{N}/{hop}/{nb} [{backend}]"
    d = D.DF(SR, N, hop, nb, 1)
    assert d.erb_widths().tolist() == ref["widths"].tolist()
    assert np.array_equal(d.fft_window().astype(np.float64), R.window(N)) and d.wnorm() == R.wnorm(N, hop)
    S = d.analysis(x.copy())
    assert S.dtype == np.complex64
    hold_to_f64(S, c["spec"], r["spec"], f"{tag} analysis")
    keep = Y.copy()
    y = d.synthesis(keep)
    assert np.array_equal(keep, Y) and y.dtype == np.float32
    hold_to_f64(y, c["y"], r["y"], f"{tag} synthesis")
    spec, fe, fs = df_features(torch.from_numpy(x.copy()), d, ref["nb_df"])
    hold_to_f64(torch.view_as_complex(spec.squeeze(1).cpu()).numpy(), c["spec"], r["spec"], f"{tag} df_features spec")
    hold_to_f64(fe.squeeze(1).cpu().numpy(), c["fe"], r["fe"], f"{tag} df_features feat_erb")
    hold_to_f64(torch.view_as_complex(fs.squeeze(1).cpu()).numpy(), c["fs"], r["fs"], f"{tag} df_features feat_spec")
    # cut streams: every row with a state of its own (without a reset pyDF's one DFState would run on from row to row)
    for row in range(x.shape[0]):
        ds = D.DF(SR, N, hop, nb, 1)
        parts = [ds.analysis(x[row:row + 1, a * hop:b * hop].copy(), reset=False) for a, b in zip(CUTS[:-1], CUTS[1:])]
        assert np.array_equal(np.concatenate(parts, 1), S[row:row + 1, :CUTS[-1]]), (tag, "analysis cut", row)   # (a hop below 4: the 3 odd samples are frames)
    for row in range(Y.shape[0]):
        ds = D.DF(SR, N, hop, nb, 1)
        parts = [ds.synthesis(Y[row:row + 1, a:b].copy(), reset=False) for a, b in zip(CUTS[:-1], CUTS[1:])]
        assert np.array_equal(np.concatenate(parts, 1), y[row:row + 1]), (tag, "synthesis cut", row)


@pytest.mark.parametrize("N,hop", [(2160, 1080), (4096, 2048)])
def test_oversized_transforms_are_refused_at_creation(backend, N, hop):
    """76 N + 256 bytes of dynamic LDS and the band tables against the 160 KB a workgroup can have: 2048 fits (155 904 and the tables), 2160
    needs 164 416, 4096 needs 311 552.  The state is refused when it is created, on both backends alike, and nothing is launched."""
    D = _libdf()
    with pytest.raises(RuntimeError, match=r"bytes of LDS per workgroup.*limit is 163840"):
        D.DF(SR, N, hop, 8, 1)
