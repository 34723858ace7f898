"""deepfilternet_amd.metrics: the composite measures' parts — segmental SNR, LLR, WSS, frequency-weighted segmental SNR (df/sepm.py) — on the device.

The kernels are pinned to the reference's own ``df/sepm.py`` through tests/golden/sepm.npz (tools/gen_golden_sepm.py, 16 kHz); everything that is
not in the fixture is held to tests/sepm_ref.py, a numpy float64 restatement that a CPU test holds to the same fixture at 1e-9.

Bars.  Segmental SNR, WSS, fwSNR: 1e-8 max(1, |ref|) against the reference's value.  Derived, not measured: the chain is float64 with sums of at
most 1024 terms (about 1e-13 relative), and the reference's own amplification is known — with every input sample moved by one float32 ulp (6e-8
relative) it moved by at most 1.1e-5 (fwSNR), 1.3e-6 (WSS) and 3e-7 (segmental SNR), under 200 per unit of relative error — so about 2e-11 is
expected and the bar leaves about 500 x for the device's log10 / pow / sqrt and the transform, a thousand times finer than one float32 ulp of
the input.  LLR: the two 17 x 17 quadratic forms are taken in float64 from the float32-rounded coefficients and lags (the reference: float32, in
its BLAS's order), so the fixture stores that value (``llr.f64``) and the bar max(16 |llr - llr.f64|, 1e-6) per case.  Against the restatement,
which takes the forms in float64 too, the bar is that floor, 1e-6, or — where it is larger — 32 x the restatement's own change when it sums
every lag's products in the opposite order (``llr_order_spread``).  The reason: lpcoeff rounds its coefficients to float32 behind a
recursion whose condition is that of the clean frame's Toeplitz matrix, so two float64 evaluations that differ in the last bit of a lag can
differ by a float32 ulp in a coefficient.  For the clips here that spread is 0 except where the matrix is nearly singular: 3e-9 for the tonal
clip and 2.7e-7 for the 8 kHz clip brought to 16 kHz (an empty upper half band; condition 3e8 — the reference's own float32 forms are 1.4
away from the float64 value there)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import sepm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sepm.npz")
KEYS = ("ssnr", "llr", "wss", "fwsnr")
REL_BAR = 1e-8
LLR_BAR = 1e-6      # against the restatement: the floor of the fixture's llr.tol, or 32 x the restatement's own order spread


@functools.lru_cache(maxsize=None)
def _fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


CASE_NAMES = [str(n) for n in _fixture()["names"]]


def _case(name):
    g = _fixture()
    c = g[f"{name}.clean"].astype(np.float32) / np.float32(32768.0)
    p = g[f"{name}.processed"].astype(np.float32) / np.float32(32768.0)
    return c, p


def _want(name):
    """the values a float64 implementation is held to, and their bars"""
    g = _fixture()
    want = {k: float(g[f"{name}.{k}"]) for k in KEYS}
    want["llr"] = float(g[f"{name}.llr.f64"])
    bars = {k: REL_BAR * max(1.0, abs(want[k])) if want[k] == want[k] else 0.0 for k in KEYS}
    bars["llr"] = float(g[f"{name}.llr.tol"])
    return want, bars


@functools.lru_cache(maxsize=None)
def _restated(name):
    return R.sepm(*_case(name))


def _clip(n, seed, quiet=(), amp=0.2, noise=0.06):
    """amplitude-modulated low-passed noise, sections scaled by 1e-4 -> (clean, processed) float32"""
    r = np.random.default_rng(seed)

    def lp(k):
        return np.convolve(r.standard_normal(n + 16), np.ones(k) / k, mode="valid")[:n]

    x = lp(8)
    x = amp * x / np.abs(x).max() * (1 + 0.5 * np.sin(np.arange(n) / 300.0 + seed)) / 1.5
    for a, b in quiet:
        x[a:b] *= 1e-4
    d = lp(8)
    y = x + noise * d / np.abs(d).max()
    return x.astype(np.float32), y.astype(np.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).tolist()


def _close(got, want, bar):
    if want != want:
        return got != got
    return abs(got - want) <= bar


def _check_values(tag, got, want, bars):
    ok = True
    for k in KEYS:
        d = abs(got[k] - want[k])
        print(f"{tag} {k:5s}: got {got[k]!r} want {want[k]!r} |diff| {d:.3e} bar {bars[k]:.1e}" + (f" ratio {d / bars[k]:.2e}" if bars[k] else ""))
        ok &= _close(got[k], want[k], bars[k])
    return ok


def _rest_bars(m):
    bars = {k: REL_BAR * max(1.0, abs(m[k])) for k in KEYS}
    bars["llr"] = max(LLR_BAR, 32.0 * m["llr_order_spread"])
    return bars


def _raw_call(x, y, lens, sr=16_000, resampler=None, fill=None, short=0):
    """dfx_sepm itself on [B, T] float32 tensors -> (out float64 [B, 4], info int32 [B, 2]) on the device"""
    from deepfilternet_amd import _lib

    L, dev = _lib.lib(), _lib.device()
    x, y = x.to(dev).contiguous(), y.to(dev).contiguous()
    B, T = x.shape
    cl = (C.c_int64 * max(B, 1))(*lens)
    need = C.c_int64()
    _lib.check(L.dfx_sepm_workspace_bytes(sr, B, cl, C.byref(need)))
    ws = torch.empty(need.value - short, dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    info = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    rc = L.dfx_sepm(resampler, _lib.ptr(x), _lib.ptr(y), B, T, cl, _lib.ptr(out), _lib.ptr(info), _lib.ptr(ws), int(ws.numel()), _lib.stream())
    return rc, out, info


# ---- 0. the restatement against the reference's numbers (no library) ----------------------------------------------------------------------------------
def test_restatement_matches_fixture():
    g = _fixture()
    ups = downs = 0
    for name in CASE_NAMES:
        m = _restated(name)
        assert [m["F"], m["K"]] == g[f"{name}.info"].tolist(), name
        for k in KEYS:
            want = float(g[f"{name}.llr.f64"]) if k == "llr" else float(g[f"{name}.{k}"])
            assert _close(m[k], want, 1e-9 * max(1.0, abs(want)) if want == want else 0.0), (name, k, m[k], want)
        assert float(g[f"{name}.llr.tol"]) <= 1e-4, name
        if name in ("highpass", "lowpass"):
            assert m["runoff_up"] > 0 and m["runoff_down"] > 0, (name, m["runoff_up"], m["runoff_down"])
            ups, downs = ups + m["runoff_up"], downs + m["runoff_down"]
        if m["F"]:
            assert not m["min_frac"] < 1e-3, name
    assert ups > 0 and downs > 0
    assert R.crit_filter()[1] > 1e-9
    assert [R.trim_count(F) for F in (1, 10, 30, 50, 70)] == [1, 10, 28, 48, 66]


@pytest.mark.needs_reference
def test_restatement_matches_reference():
    """df/sepm.py itself, re-run (pesq stubbed): the fixture's values exactly, the restatement at 1e-9"""
    from tools.gen_golden_sepm import install_pesq_stub
    from tools.ref_import import install_shims

    install_shims()
    install_pesq_stub()
    from df import sepm as S  # type: ignore

    g = _fixture()
    for name in CASE_NAMES:
        c, p = _case(name)
        m = _restated(name)
        if m["F"] < 1:
            continue   # (the reference raises)
        for k, fn in (("ssnr", S.SNRseg), ("wss", S.wss), ("fwsnr", S.fwSNRseg), ("llr", S.llr)):
            with np.errstate(all="ignore"):
                ref = float(fn(c, p, 16_000))
            assert abs(ref - float(g[f"{name}.{k}"])) <= 1e-12 * max(1.0, abs(ref)), (name, k)
            if k != "llr":
                assert abs(m[k] - ref) <= 1e-9 * max(1.0, abs(ref)), (name, k, m[k], ref)
            else:
                assert abs(m[k] - ref) <= float(g[f"{name}.llr.tol"]), (name, m[k], ref)


# ---- 1. the fixture: the reference's own numbers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_case(backend, name):
    from deepfilternet_amd import _lib, metrics

    g = _fixture()
    c, p = _case(name)
    tc, tp = torch.from_numpy(c), torch.from_numpy(p)
    m, info = metrics.sepm(tc, tp, 16_000, dtype=torch.float64, return_info=True)
    assert all(m[k].dtype == torch.float64 and tuple(m[k].shape) == (1,) for k in KEYS) and info.dtype == torch.int32 and tuple(info.shape) == (1, 2)
    got = {k: float(m[k][0]) for k in KEYS}
    want, bars = _want(name)
    assert info[0].tolist() == g[f"{name}.info"].tolist()
    assert _check_values(name, got, want, bars)
    if name == "n599":
        assert all(got[k] != got[k] for k in KEYS) and info[0].tolist() == [0, 0]
    if name == "identical":
        assert got["ssnr"] == 35.0 and got["fwsnr"] == 35.0 and got["wss"] == 0.0
    if name == "zero_clean":
        assert abs(got["llr"] - np.log(1000.0)) <= 1e-12 and got["ssnr"] == -10.0
    if name == "zero_est":   # every band of the processed signal sits on the -100 dB clip: the restatement's log energies say so
        sp = R._band_spectra(p.astype(np.float64), R.n_frames(len(p)))
        assert (10 * np.log10((sp ** 2) @ R.crit_filter()[0].T) < -100).all()
    # the raw C call, and the single-measure functions (float32 by default): the same pass
    rc, out, rinfo = _raw_call(tc[None], tp[None], [len(c)])
    assert rc == _lib.DFX_OK and rinfo.tolist() == info.tolist()
    for i, k in enumerate(KEYS):
        assert _bits(out[:, i]) == _bits(m[k]), k
    for k, fn in zip(KEYS, (metrics.seg_snr, metrics.llr, metrics.wss, metrics.fw_seg_snr)):
        v = fn(tc, tp, 16_000)
        assert v.dtype == torch.float32 and torch.equal(v.isnan(), m[k].isnan())
        assert torch.equal(v[~v.isnan()], m[k].to(torch.float32)[~v.isnan()]), k
    # int16 PCM is the same input
    mi = metrics.sepm(torch.from_numpy(g[f"{name}.clean"]), torch.from_numpy(g[f"{name}.processed"]), 16_000, dtype=torch.float64)
    assert all(_bits(mi[k]) == _bits(m[k]) for k in KEYS)


# ---- 2. a strongly tonal clip: where the reference's float32 forms are inexact --------------------------------------------------------------------------
def test_tonal_clip_llr(backend):
    """A harmonic stack plus 0.1 % noise: the clean frame's Toeplitz matrix is nearly singular, the forms cancel to about 1e-6 of R[0] |a|^2, and
    the reference's float32 evaluation of them is about 1e-3 away in the clip's LLR (1.2e-3 .. 3.8e-3 measured on the reference) — not in the
    fixture for that reason.  The float64 value is held to the restatement at 1e-6."""
    from deepfilternet_amd import metrics

    n = 3000
    r = np.random.default_rng(5)
    t = np.arange(n) / 16_000.0
    x = sum(np.sin(2 * np.pi * 200.0 * h * t + h) / h for h in range(1, 9))
    x = 0.2 * x / np.abs(x).max()
    c = (x + 1e-3 * 0.2 * r.standard_normal(n)).astype(np.float32)
    p = (0.9 * x + 1e-3 * 0.2 * r.standard_normal(n) + 0.01 * np.sin(2 * np.pi * 1234.0 * t)).astype(np.float32)
    m, info = metrics.sepm(torch.from_numpy(c), torch.from_numpy(p), 16_000, dtype=torch.float64, return_info=True)
    want = R.sepm(c, p)
    got = {k: float(m[k][0]) for k in KEYS}
    assert info[0].tolist() == [want["F"], want["K"]]
    bars = _rest_bars(want)
    assert bars["llr"] == 1e-6
    assert _check_values("tonal", got, want, bars)


# ---- 3. the trimmed mean across sizes ------------------------------------------------------------------------------------------------------------------------
def test_trimmed_mean_sizes(backend):
    """300 and 3 000 frames (more than one value per thread of the row reduction, 188 workgroups of frames); the 300-frame clip twice in the
    batch, at different row positions: equal bits"""
    from deepfilternet_amd import metrics

    n_small, n_big = 480 + 300 * 120 + 11, 480 + 3000 * 120
    small, big = _clip(n_small, 21, quiet=((9000, 14_000),)), _clip(n_big, 22, quiet=((50_000, 90_000), (200_000, 201_000)))
    cx = [torch.from_numpy(small[0]), torch.from_numpy(big[0]), torch.from_numpy(small[0])]
    cy = [torch.from_numpy(small[1]), torch.from_numpy(big[1]), torch.from_numpy(small[1])]
    m, info = metrics.sepm(cx, cy, 16_000, dtype=torch.float64, return_info=True)
    assert info.tolist() == [[300, 285], [3000, 2850], [300, 285]]
    for k in KEYS:
        assert _bits(m[k][0:1]) == _bits(m[k][2:3]), k
    for i, (x, y) in ((0, small), (1, big)):
        want = R.sepm(x, y)
        assert [want["F"], want["K"]] == info[i].tolist()
        assert _check_values(f"F {want['F']}", {k: float(m[k][i]) for k in KEYS}, want, _rest_bars(want))


# ---- 4. a row is the row alone -----------------------------------------------------------------------------------------------------------------------------------
def test_batch_rows_are_the_rows_alone(backend):
    from deepfilternet_amd import _lib, metrics

    lens = [2000, 599, 3333, 600, 1500]
    T = max(lens) + 41
    clips = [_clip(n, 40 + i, quiet=((n // 4, n // 3),) if i == 2 else ()) for i, n in enumerate(lens)]
    r = np.random.default_rng(3)
    cx = torch.from_numpy(r.standard_normal((5, T)).astype(np.float32))      # whatever lies behind a row's samples is not the row
    cy = torch.from_numpy((1e3 * r.standard_normal((5, T))).astype(np.float32))
    for i, (x, y) in enumerate(clips):
        cx[i, :lens[i]], cy[i, :lens[i]] = torch.from_numpy(x), torch.from_numpy(y)
    rc, out, info = _raw_call(cx, cy, lens, fill=0xFF)
    assert rc == _lib.DFX_OK
    assert info.tolist() == [[R.n_frames(n), R.trim_count(R.n_frames(n))] for n in lens]
    assert out[1].isnan().all() and not out[[0, 2, 3, 4]].isnan().any()
    as_list = metrics.sepm([torch.from_numpy(x) for x, _ in clips], [torch.from_numpy(y) for _, y in clips], 16_000, dtype=torch.float64)
    padded = metrics.sepm(cx, cy, 16_000, lengths=lens, dtype=torch.float64)
    for i, (x, y) in enumerate(clips):
        rc1, alone, info1 = _raw_call(torch.from_numpy(x)[None], torch.from_numpy(y)[None], [lens[i]], fill=0)
        assert rc1 == _lib.DFX_OK and info1[0].tolist() == info[i].tolist()
        assert _bits(alone[0]) == _bits(out[i]), i
        for j, k in enumerate(KEYS):
            assert _bits(as_list[k][i:i + 1]) == _bits(out[i, j:j + 1]) and _bits(padded[k][i:i + 1]) == _bits(out[i, j:j + 1]), (i, k)
    want = R.sepm(*clips[2])
    assert _check_values("row 2", {k: float(out[2, j]) for j, k in enumerate(KEYS)}, want, _rest_bars(want))


# ---- 5. other rates: the resampler in front ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n", [(48_000, 24_001), (8_000, 4_003)])
def test_other_rates(backend, sr, n):
    """The restatement is fed io.resample(row alone, sr, 16000) downloaded from the device, so the resampler (pinned by test_io.py) is outside
    the comparison and the bars are the 16 kHz ones.  That holds because the rows-aware resampler in front of the kernels gives a row the
    bits of io.resample of the row alone — asserted first: the row inside a padded batch at ``sr`` scores the bits of its resampled self at
    16 kHz."""
    from deepfilternet_amd import io, metrics

    x, y = _clip(n, sr // 1000, quiet=((n // 3, n // 2),))
    other = _clip(n + 500, 77)
    rx = io.resample(torch.from_numpy(x)[None], sr, 16_000)[0]
    ry = io.resample(torch.from_numpy(y)[None], sr, 16_000)[0]
    T = n + 500
    cx, cy = torch.full((2, T), 3.0), torch.full((2, T), -7.0)
    cx[0], cy[0] = torch.from_numpy(other[0]), torch.from_numpy(other[1])
    cx[1, :n], cy[1, :n] = torch.from_numpy(x), torch.from_numpy(y)
    m, info = metrics.sepm(cx, cy, sr, lengths=[T, n], dtype=torch.float64, return_info=True)
    at16 = metrics.sepm(rx, ry, 16_000, dtype=torch.float64)
    for k in KEYS:
        assert _bits(m[k][1:2]) == _bits(at16[k]), k
    want = R.sepm(rx.cpu().numpy(), ry.cpu().numpy())
    assert info[1].tolist() == [want["F"], want["K"]] and want["F"] > 60
    assert _check_values(f"sr {sr}", {k: float(m[k][1]) for k in KEYS}, want, _rest_bars(want))


# ---- 6. composite ------------------------------------------------------------------------------------------------------------------------------------------------
def test_composite(backend):
    from deepfilternet_amd import metrics

    names = ["F30", "identical", "zero_est", "zero_clean", "n599"]
    pesq = [2.5, 4.5, 1.0, 1.0, 3.0]
    cs, ps = [torch.from_numpy(_case(n)[0]) for n in names], [torch.from_numpy(_case(n)[1]) for n in names]
    res = metrics.composite(cs, ps, 16_000, pesq=pesq, dtype=torch.float64)
    assert sorted(res) == sorted(["pesq", "csig", "cbak", "covl", "ssnr", "llr", "wss"]) and all(tuple(v.shape) == (5,) for v in res.values())
    clamped = set()
    for i, name in enumerate(names):
        want, bars = _want(name)
        if name == "n599":
            assert all(float(res[k][i]) != float(res[k][i]) for k in ("csig", "cbak", "covl", "ssnr", "llr", "wss")) and float(res["pesq"][i]) == 3.0
            continue
        raw = {"csig": 3.093 - 1.029 * want["llr"] + 0.603 * pesq[i] - 0.009 * want["wss"],
               "cbak": 1.634 + 0.478 * pesq[i] - 0.007 * want["wss"] + 0.063 * want["ssnr"],
               "covl": 1.594 + 0.805 * pesq[i] - 0.512 * want["llr"] - 0.007 * want["wss"]}
        bar = 1.029 * bars["llr"] + 0.009 * bars["wss"] + 0.063 * bars["ssnr"] + 1e-12
        for k, v in raw.items():
            w = min(5.0, max(1.0, v))
            if w != v:
                clamped.add(w)
            got = float(res[k][i])
            print(f"{name} {k}: got {got!r} want {w!r} (unclamped {v!r}) bar {bar:.1e}")
            assert abs(got - w) <= bar and 1.0 <= got <= 5.0
            if abs(v - w) > bar:
                assert got == w          # a clamped value is exactly the limit
        assert float(res["pesq"][i]) == pesq[i]
        for k in ("ssnr", "llr", "wss"):
            assert _close(float(res[k][i]), want[k], bars[k])
    assert clamped == {1.0, 5.0}
    # no PESQ given: the NaN pattern; float32 by default
    none = metrics.composite(cs[:2], ps[:2], 16_000)
    assert all(v.dtype == torch.float32 for v in none.values())
    assert all(none[k].isnan().all() for k in ("pesq", "csig", "cbak", "covl")) and not any(none[k].isnan().any() for k in ("ssnr", "llr", "wss"))
    # a tensor of values on the device is taken too
    dev = metrics.composite(cs[:2], ps[:2], 16_000, pesq=torch.tensor(pesq[:2]).to(res["csig"].device), dtype=torch.float64)
    assert _bits(dev["csig"]) == _bits(res["csig"][:2])


# ---- 7. what is refused --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend):
    from deepfilternet_amd import _lib, io, metrics

    x, y = (torch.from_numpy(a) for a in _clip(2000, 1))
    with pytest.raises(TypeError, match="float32 or int16"):
        metrics.sepm(x.double(), y.double(), 16_000)
    with pytest.raises(TypeError, match="float32 or int16"):
        metrics.llr(x.to(torch.int32), y.to(torch.int32), 16_000)
    with pytest.raises(TypeError, match="float32 or float64"):
        metrics.sepm(x, y, 16_000, dtype=torch.float16)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.sepm(x, y[:-1], 16_000)
    with pytest.raises(ValueError, match="rows' lengths"):
        metrics.wss([x, x[:700]], [y, y[:699]], 16_000)
    with pytest.raises(ValueError, match="2 entries for 1 rows"):
        metrics.seg_snr(x, y, 16_000, lengths=[2000, 2000])
    with pytest.raises(ValueError, match="outside"):
        metrics.fw_seg_snr(x, y, 16_000, lengths=[2001])
    for sr in (0, -16_000):
        with pytest.raises(ValueError, match="positive"):
            metrics.sepm(x, y, sr)
    with pytest.raises(ValueError, match="pesq has 2 entries for 1 rows"):
        metrics.composite(x, y, 16_000, pesq=[1.0, 2.0])
    L = _lib.lib()
    need = C.c_int64()
    cl = (C.c_int64 * 1)(2000)
    _lib.check(L.dfx_sepm_workspace_bytes(16_000, 1, cl, C.byref(need)))
    short = torch.empty(need.value - 1, dtype=torch.uint8, device=_lib.device())
    with pytest.raises(ValueError, match=f"workspace of {need.value - 1} bytes, {need.value} needed"):
        metrics.sepm(x, y, 16_000, workspace=short)
    assert _raw_call(x[None], y[None], [2000], short=1)[0] == _lib.DFX_ERR_INVALID_ARG
    # the C calls themselves
    assert L.dfx_sepm_workspace_bytes(0, 1, cl, C.byref(need)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_sepm_workspace_bytes(16_000, 1, (C.c_int64 * 1)(-1), C.byref(need)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_sepm_workspace_bytes(16_000, 1, None, C.byref(need)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_sepm_workspace_bytes(16_000, 1, cl, None) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_sepm_workspace_bytes(16_000, 0, None, C.byref(need)) == _lib.DFX_OK
    assert _raw_call(x[None], y[None], [2001])[0] == _lib.DFX_ERR_INVALID_ARG                       # a length outside the stride
    wrong = io._resampler(48_000, 10_000, "sinc_fast", _lib.library_path())                         # a resampler to another rate
    assert _raw_call(x[None], y[None], [2000], sr=48_000, resampler=wrong.h)[0] == _lib.DFX_ERR_INVALID_ARG
    dev = _lib.device()
    xd, yd = x[None].to(dev).contiguous(), y[None].to(dev).contiguous()
    _lib.check(L.dfx_sepm_workspace_bytes(16_000, 1, cl, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = torch.empty((1, 4), dtype=torch.float64, device=dev)
    for args in ((None, _lib.ptr(yd), _lib.ptr(out), _lib.ptr(ws)), (_lib.ptr(xd), None, _lib.ptr(out), _lib.ptr(ws)),
                 (_lib.ptr(xd), _lib.ptr(yd), None, _lib.ptr(ws)), (_lib.ptr(xd), _lib.ptr(yd), _lib.ptr(out), None)):
        assert L.dfx_sepm(None, args[0], args[1], 1, 2000, cl, args[2], None, args[3], need.value, _lib.stream()) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_sepm(None, _lib.ptr(xd), _lib.ptr(yd), 1, 2000, None, _lib.ptr(out), None, _lib.ptr(ws), need.value, _lib.stream()) == _lib.DFX_ERR_INVALID_ARG
    # nothing to score is not an error
    assert all(v.numel() == 0 for v in metrics.sepm([], [], 16_000).values())


# ---- 8. files and the command line ---------------------------------------------------------------------------------------------------------------------------------
def test_score_files_and_cli(backend, tmp_path, capsys):
    from deepfilternet_amd import metrics
    from deepfilternet_amd.io import save_audio

    cdir, edir = tmp_path / "clean", tmp_path / "enh"
    cdir.mkdir(), edir.mkdir()
    want = {}
    for i, n in enumerate((3000, 2500)):
        x, y = _clip(n, 90 + i)
        save_audio(str(cdir / f"c{i}.wav"), torch.from_numpy(x), 16_000, dtype=torch.float32)
        save_audio(str(edir / f"c{i}_DeepFilterNet3.wav"), torch.from_numpy(y[: n - 3 * i]), 16_000, dtype=torch.float32)
        want[f"c{i}.wav"] = R.sepm(x[: n - 3 * i], y[: n - 3 * i])
    pairs = metrics.pair_directories(str(cdir), str(edir))
    plain = metrics.score_files(pairs)
    assert all(sorted(s) == ["sisdr", "stoi"] for s in plain)
    full = metrics.score_files(pairs, composite=True)
    for (c, _), s, q in zip(pairs, full, plain):
        assert sorted(s) == sorted(["sisdr", "stoi", "ssnr", "llr", "wss", "fwsnr"])
        assert s["sisdr"] == q["sisdr"] and (s["stoi"] == q["stoi"] or (s["stoi"] != s["stoi"] and q["stoi"] != q["stoi"]))
        w = want[os.path.basename(c)]
        assert _check_values(os.path.basename(c), s, w, _rest_bars(w))
    csv = tmp_path / "scores.csv"
    assert metrics.main([str(cdir), str(edir), "--csv", str(csv), "--composite"]) == 0
    lines = csv.read_text().strip().split("\n")
    assert lines[0] == "file,sisdr,stoi,ssnr,llr,wss,fwsnr" and [ln.split(",")[0] for ln in lines[1:]] == ["c0.wav", "c1.wav"]
    assert all(len(ln.split(",")) == 7 for ln in lines[1:])
    assert abs(float(lines[1].split(",")[3]) - want["c0.wav"]["ssnr"]) < 1e-5
    assert metrics.main([str(cdir), str(edir), "--csv", str(csv)]) == 0
    assert csv.read_text().split("\n")[0] == "file,sisdr,stoi"
    capsys.readouterr()
