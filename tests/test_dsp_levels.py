"""The level ladder: one batch whose rows are the same signal at 0.3, 3e-3, 3e-5 and 3e-7 of full scale, plus digital silence, a burst between
silences, DC, a full-scale square wave and a single full-scale sample — through the features and through enhance(), every ROW held to a bound of
its own against the float64 restatement (oracle/dsp64.py).

Why: every other DSP and enhance() test feeds white noise at 0.1 ... 0.3 with an absolute bar (2e-5, 1e-6, RMS 2e-6 over the batch).  Such a bar
is a thousand times too loose for a row at -80 dBFS, an RMS over a batch is set by its loudest row, and at those levels the ERB feature's
+ 1e-10 floor is five orders below the band energies and the unit-norm state leaves its initial ramp at once.

  (a) df_features (960 / 480 / 32 bands, nb_df 96) and dfx_erb(db=True): per row |kernel - dsp64| <= 4 * max(E32, 2^-23 max|dsp64|), E32 and the
      maximum taken per row (tests/helpers.py hold_to_f64); the silent row's spectrum and unit-normed bins are exact zeros.
  (b) enhance() against dsp64.enhance64 under lively weights (tests/helpers.py lively_state_dict): per row
      max|y - y64| <= 4 * max(E32, S21), E32 = |dfnet_oracle.enhance - enhance64| and S21 the weights-times-(1 +- 2^-21) perturbation of
      tests/test_gru_precision.py, both per row; the silent row comes back as exact zeros.  The test shows that it sees what it is for:
      three mutants of enhance64 (dsp64.MUTANTS) must each move at least one row by 10 * 4 * max(E32, S21).
Nothing in the bounds comes from what the kernels return.  The ratios are printed (pytest -s); docs/measurements.md records the GPU's."""
import functools

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from oracle import dsp64 as R
from oracle import libdf_oracle as L
from tests.helpers import DSP_MARGIN, hold_to_f64, lively_state_dict, named_params
from tests.test_gru_precision import _perturbed

HOP, FRAMES = 480, 13
ROWS = ("0.3", "3e-3", "3e-5", "3e-7", "silence", "burst", "DC 0.5", "square +-1", "one sample")
SILENT = ROWS.index("silence")
SEES = 10.0
SEED = 11


@functools.lru_cache(maxsize=None)
def ladder():
    n = HOP * FRAMES
    rng = np.random.default_rng(5)
    t = np.arange(n) / 48000.0
    sig = rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 7.0 * t))   # seeded noise under a slow envelope
    x = np.zeros((len(ROWS), n))
    for i, g in enumerate((0.3, 3e-3, 3e-5, 3e-7)):
        x[i] = g * sig
    x[5, 2500:3300] = 0.5 * rng.standard_normal(800)
    x[6] = 0.5
    x[7] = np.where((np.arange(n) // 240) % 2 == 0, 1.0, -1.0)   # 100 Hz at 48 kHz
    x[8, 3001] = 1.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def test_features_hold_per_row(backend):
    from deepfilternet_amd import libdf as D
    from deepfilternet_amd.enhance import _norm_alpha, df_features

    x = ladder()
    d, o = D.DF(48000, 960, 480, 32, 2), L.DF(48000, 960, 480, 32, 2)
    w, alpha = o.erb_widths(), _norm_alpha(d)
    Sc = o.analysis(x.copy())
    c = {"spec": Sc, "feat_erb": L.erb_norm(L.erb(Sc, w), alpha), "feat_spec": L.unit_norm(np.ascontiguousarray(Sc[..., :96]), alpha)}
    Sr = R.analysis(x, 960, 480)[0]
    r = {"spec": Sr, "feat_erb": R.erb_norm(R.erb_db(Sr, w), alpha)[0], "feat_spec": R.unit_norm(Sr[..., :96], alpha)[0]}
    spec, fe, fs = df_features(torch.from_numpy(x.copy()), d, 96)
    got = {"spec": torch.view_as_complex(spec.squeeze(1).cpu()).numpy(), "feat_erb": fe.squeeze(1).cpu().numpy(),
           "feat_spec": torch.view_as_complex(fs.squeeze(1).cpu()).numpy()}
    loud = [i for i in range(len(ROWS)) if i != SILENT]
    for k in ("spec", "feat_erb", "feat_spec"):
        e32 = np.abs(c[k] - r[k]).reshape(len(ROWS), -1).max(1)
        assert np.all(e32[loud] > 0), (k, e32)
        hold_to_f64(got[k], c[k], r[k], f"[{backend}] df_features {k} per row", rows=True, need_e32=False)
    assert not got["spec"][SILENT].any() and not got["feat_spec"][SILENT].any()
    # the band energies in dB by the kernel of their own, on one spectrum for all three (the C oracle's: float32 values are exact in float64)
    hold_to_f64(D.erb(Sc, w, True), L.erb(Sc, w, True), R.erb_db(Sc, w), f"[{backend}] dfx_erb(db=True) per row", rows=True, need_e32=False)


CASES = [("df3", None), ("df3", 12.0), ("pf32", None), ("pf32", 12.0), ("df3_o10", None)]


def _rowmax(a):
    return np.abs(a).reshape(a.shape[0], -1).max(1)


@functools.lru_cache(maxsize=None)
def reference(name, lim):
    """The oracle's side of one enhance() case, computed once and left unchanged: y64, the per-row base max(E32, S21) and what each mutant of
    enhance64 moves per row in units of DSP_MARGIN * base."""
    p = named_params(name)
    sd = lively_state_dict(p, SEED)
    sd32 = {k: torch.as_tensor(v) for k, v in sd.items()}
    sd64 = O.to_dtype(sd32, torch.float64)
    x = ladder()
    y64 = R.enhance64(p, sd64, x, pad=False, atten_lim_db=lim, check_finish=True)
    y32 = O.enhance(p, sd32, x.copy(), pad=False, atten_lim_db=lim)
    assert y32.dtype == np.float32 and y64.dtype == np.float64 and y32.shape == y64.shape == x.shape
    e32 = _rowmax(y32 - y64)
    s21 = _rowmax(R.enhance64(p, _perturbed(sd64), x, pad=False, atten_lim_db=lim) - y64)
    base = np.maximum(e32, s21)
    loud = np.arange(len(ROWS)) != SILENT
    assert np.all(base[loud] > 0) and base[SILENT] == 0 and not y64[SILENT].any(), base
    assert np.all(base[loud] < 1e-4 * np.maximum(_rowmax(x)[loud], 1e-3)), base   # (float32-sized at every row's own level)
    moved = {}
    for m in R.MUTANTS:
        dm = _rowmax(R.enhance64(p, sd64, x, pad=False, atten_lim_db=lim, mutant=m) - y64)
        moved[m] = np.where(loud, dm / (DSP_MARGIN * np.where(loud, base, 1.0)), 0.0)
    return {"p": p, "sd": sd, "y64": y64, "e32": e32, "s21": s21, "base": base, "moved": moved}


@pytest.mark.parametrize("name,lim", CASES, ids=[f"{n}{'' if l is None else '_lim12'}" for n, l in CASES])
def test_enhance_holds_per_row(backend, name, lim):
    """df3 takes the fused finishing kernel, pf32 has the post filter, each with and without the attenuation limit; df3_o10 the two-kernel
    finish.  13 frames without end padding, so that the deep filter's look-ahead taps at the last frames read behind the clip."""
    from deepfilternet_amd.enhance import enhance, init_df

    ref = reference(name, lim)
    fmt = lambda v: np.array2string(np.asarray(v), precision=1, separator=" ", max_line_width=200, formatter={"float_kind": lambda z: f"{z:.1e}"})
    print(f"  {name} lim {lim}: oracle only, per row ({', '.join(ROWS)})\n    E32 {fmt(ref['e32'])}\n    S21 {fmt(ref['s21'])}")
    for m, moved in ref["moved"].items():
        print(f"    mutant {m:10s} moves, in units of {DSP_MARGIN:g} * max(E32, S21): {fmt(moved)}")
        assert moved.max() >= SEES, (name, lim, m, moved)
    model, df_state, _, _ = init_df(params=ref["p"], state_dict=ref["sd"], epoch="none")
    y = enhance(model, df_state, torch.from_numpy(ladder().copy()), pad=False, atten_lim_db=lim)
    model.check()
    y = y.cpu().numpy()
    assert y.shape == ref["y64"].shape and y.dtype == np.float32 and np.isfinite(y).all()
    assert not y[SILENT].any(), "digital silence must come back as exact zeros"
    err = _rowmax(y - ref["y64"])
    ratio = np.where(ref["base"] > 0, err / np.where(ref["base"] > 0, ref["base"], 1.0), 0.0)
    print(f"  {name} lim {lim} [{backend}]: max|y - y64| / max(E32, S21) per row: {np.array2string(ratio, precision=2, separator=' ')}")
    assert np.all(err <= DSP_MARGIN * ref["base"]), (name, lim, ratio)
