"""deepfilternet_amd.metrics: SI-SDR (df/evaluation_utils.py:599-619) and STOI (df/stoi.py:163-231) on the device.

The STOI core is pinned to the reference's own ``df.stoi.stoi`` through tests/golden/metrics.npz (tools/gen_golden_metrics.py: fs_source = 10000,
so no resampler in between; every clip more than 0.5 dB away from the silent-frame threshold, so the integers in ``info`` must match exactly);
other rates are held to tests/metrics_ref.py, a numpy restatement of the same file that resamples with the resampler's oracle.

Bars.  Fixture cases: the generator's max(16 |ref32 - ref64|, 1e-6) per case, against the reference's float64 value.  Other rates: the largest of
those bars (CORE_BAR, 1.9e-6 — the core in float32 against float64) plus RESAMPLE_BAR = 2e-6 for the resampler: the kernel's float32 chain of up
to ~200 taps differs from the oracle's float64 sum by about sqrt(200) * 2^-24 = 1e-6 of a sample's scale, an error that is independent from
sample to sample, and STOI — a mean of correlation coefficients of band envelopes, each over thousands of samples — moves by no more than the
relative error of its input.  SI-SDR: atol = rtol = 1e-4 dB (test_df.py:20-21) against the formula in float64."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
RESAMPLE_BAR = 2e-6
SDR_TOL = 1e-4
F32_EPS = float(np.finfo(np.float32).eps)


def _fixture():
    return np.load(GOLDEN)


CASE_NAMES = [str(n) for n in _fixture()["names"]]
CORE_BAR = max(float(_fixture()[f"{n}.tol"]) for n in CASE_NAMES)   # 1.9e-6


def _clip(n, seed, quiet=(), amp=0.2, noise=0.06):
    """amplitude-modulated low-passed noise, sections scaled by 1e-4 -> (clean, degraded) float32"""
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


def _ref_stoi(x, y, sr):
    v, info, margin = R.stoi(x, y, sr)
    assert margin > 0.5, f"test input {margin:.3f} dB from the silent-frame threshold: choose another"
    return v, info


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


def _close(got, want, bar):
    if want != want:
        return got != got
    return abs(got - want) <= bar


# ---- 1. the fixture: the reference's own numbers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stoi_fixture_case(backend, name):
    from deepfilternet_amd import metrics

    g = _fixture()
    x = torch.from_numpy(g[f"{name}.clean"].astype(np.float32) / 32768.0)
    y = torch.from_numpy(g[f"{name}.degraded"].astype(np.float32) / 32768.0)
    v, info = metrics.stoi(x, y, 10_000, return_info=True)
    assert v.dtype == torch.float32 and tuple(v.shape) == (1,) and info.dtype == torch.int32 and tuple(info.shape) == (1, 4)
    got, want, bar = float(v[0]), float(g[f"{name}.f64"]), float(g[f"{name}.tol"])
    print(f"{name}: got {got!r} reference float64 {want!r} |diff| {abs(got - want):.3e} bar {bar:.1e} info {info[0].tolist()}")
    assert info[0].tolist() == g[f"{name}.info"].tolist()
    assert _close(got, want, bar)
    if name == "zero_clean":
        assert got == 0.0
    if name == "too_short":
        assert got != got and info[0, 3].item() == 0


def test_restatement_matches_fixture():
    """the numpy restatement against the stored reference values (float64: 1e-9), integers and margins included; no library involved"""
    g = _fixture()
    for name in CASE_NAMES:
        x, y = g[f"{name}.clean"].astype(np.float64) / 32768.0, g[f"{name}.degraded"].astype(np.float64) / 32768.0
        v, info, margin = R.stoi(x, y, 10_000)
        assert info.tolist() == g[f"{name}.info"].tolist(), name
        assert _close(v, float(g[f"{name}.f64"]), 1e-9), (name, v, float(g[f"{name}.f64"]))
        assert abs(margin - float(g[f"{name}.margin"])) < 1e-6 and margin > 0.5, name
        assert float(g[f"{name}.tol"]) <= 1e-4 + 1e-4 * abs(float(g[f"{name}.f64"])) or v != v, name   # never looser than test_df's own bar


@pytest.mark.needs_reference
def test_restatement_matches_reference():
    """df.stoi.stoi itself, re-run: the fixture's values and the restatement at 1e-9 in float64"""
    from tools.ref_import import install_shims

    install_shims()
    from df.stoi import stoi as ref_stoi  # type: ignore

    g = _fixture()
    for name in CASE_NAMES:
        x, y = g[f"{name}.clean"].astype(np.float64) / 32768.0, g[f"{name}.degraded"].astype(np.float64) / 32768.0
        v, info, _ = R.stoi(x, y, 10_000)
        if info[3] == 0:
            continue   # (the reference leaves its output uninitialised)
        ref = float(ref_stoi(torch.from_numpy(x)[None], torch.from_numpy(y)[None], 10_000)[0])
        assert abs(ref - float(g[f"{name}.f64"])) <= 1e-12, name
        assert abs(v - ref) <= 1e-9, (name, v, ref)


# ---- 2. other rates: the resampler in front ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n", [(16_000, 12_000), (48_000, 38_400), (8_000, 6_001)])
def test_stoi_other_rates(backend, sr, n):
    """0.8 s or less; 8 kHz: rates below 10 kHz are accepted and up-sampled, as the reference does"""
    from deepfilternet_amd import metrics

    x, y = _clip(n, sr, quiet=((n // 3, n // 2),))
    v, info = metrics.stoi(torch.from_numpy(x), torch.from_numpy(y), sr, return_info=True)
    want, winfo = _ref_stoi(x, y, sr)
    print(f"sr {sr}: got {float(v[0])!r} restatement {want!r} |diff| {abs(float(v[0]) - want):.3e} info {info[0].tolist()}")
    assert info[0].tolist() == winfo.tolist()
    assert abs(float(v[0]) - want) <= CORE_BAR + RESAMPLE_BAR


# ---- 3. a row is the row alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [10_000, 16_000])
def test_batch_rows_are_the_rows_alone(backend, sr):
    from deepfilternet_amd import _lib, metrics

    k = sr // 10_000 if sr > 10_000 else 1
    lens = [4100 * sr // 10_000, 6001 * sr // 10_000 + k, 5000 * sr // 10_000]
    T = max(lens) + 37
    clips = [_clip(n, 40 + i, quiet=((n // 4, n // 3),) if i != 1 else ()) for i, n in enumerate(lens)]
    cx = torch.full((3, T), float("nan"))          # whatever lies behind a row's samples is not the row
    cy = torch.full((3, T), 1.0e30)
    for i, (x, y) in enumerate(clips):
        cx[i, :lens[i]], cy[i, :lens[i]] = torch.from_numpy(x), torch.from_numpy(y)
    v, info = metrics.stoi(cx, cy, sr, lengths=lens, return_info=True)
    s = metrics.si_sdr(cx, cy, lengths=lens)
    assert not torch.isnan(v).any() and not torch.isnan(s).any()
    for i, (x, y) in enumerate(clips):
        va, ia = metrics.stoi(cx[i:i + 1, :lens[i]], cy[i:i + 1, :lens[i]], sr, return_info=True)
        assert _bits(va) == _bits(v[i:i + 1]) and ia[0].tolist() == info[i].tolist(), i
        assert _bits(metrics.si_sdr(torch.from_numpy(x), torch.from_numpy(y))) == _bits(s[i:i + 1]), i
        want, winfo = _ref_stoi(x, y, sr)
        assert info[i].tolist() == winfo.tolist() and abs(float(v[i]) - want) <= CORE_BAR + (RESAMPLE_BAR if sr != 10_000 else 0.0)
    # the same bits out of a workspace full of 0xFF bytes, and of NaNs
    need = C.c_int64()
    cl = (C.c_int64 * 3)(*lens)
    _lib.check(_lib.lib().dfx_stoi_workspace_bytes(sr, 3, cl, C.byref(need)))
    ws = torch.empty(need.value + (-need.value) % 4, dtype=torch.uint8, device=_lib.device())
    need2 = C.c_int64()
    _lib.check(_lib.lib().dfx_si_sdr_workspace_bytes(3, cl, C.byref(need2)))
    assert need2.value <= need.value
    for fill in ("ff", "nan"):
        if fill == "ff":
            ws.fill_(0xFF)
        else:
            ws.view(torch.float32).fill_(float("nan"))
        v2, info2 = metrics.stoi(cx, cy, sr, lengths=lens, return_info=True, workspace=ws)
        assert _bits(v2) == _bits(v) and info2.tolist() == info.tolist(), fill
        if fill == "ff":
            ws.fill_(0xFF)
        else:
            ws.view(torch.float32).fill_(float("nan"))
        assert _bits(metrics.si_sdr(cx, cy, lengths=lens, workspace=ws)) == _bits(s), fill


# ---- 4. the input forms ---------------------------------------------------------------------------------------------------------------------------------
def test_list_and_pcm16_forms(backend):
    from deepfilternet_amd import metrics

    g = _fixture()
    names = ["L31", "odd_pad_gap", "first_removed_last_kept"]
    xi = [torch.from_numpy(g[f"{n}.clean"]) for n in names]
    yi = [torch.from_numpy(g[f"{n}.degraded"]) for n in names]
    lens = [int(t.shape[0]) for t in xi]
    T = max(lens)
    fx, fy = torch.zeros((3, T)), torch.zeros((3, T))
    px, py = torch.zeros((3, T), dtype=torch.int16), torch.zeros((3, T), dtype=torch.int16)
    for i in range(3):
        fx[i, :lens[i]], fy[i, :lens[i]] = xi[i].float() / 32768.0, yi[i].float() / 32768.0
        px[i, :lens[i]], py[i, :lens[i]] = xi[i], yi[i]
    v = metrics.stoi(fx, fy, 10_000, lengths=lens)
    s = metrics.si_sdr(fx, fy, lengths=lens)
    for form, (a, b, kw) in {"list of float32": ([t.float() / 32768.0 for t in xi], [t.float() / 32768.0 for t in yi], {}),
                             "list of int16": (xi, yi, {}), "int16 [B, T]": (px, py, {"lengths": lens})}.items():
        assert _bits(metrics.stoi(a, b, 10_000, **kw)) == _bits(v), form
        assert _bits(metrics.si_sdr(a, b, **kw)) == _bits(s), form
    for i, n in enumerate(names):
        assert _close(float(v[i]), float(g[f"{n}.f64"]), float(g[f"{n}.tol"]))
    # [T] is one row
    assert _bits(metrics.stoi(fx[0, :lens[0]], fy[0, :lens[0]], 10_000)) == _bits(v[0:1])


# ---- 5. SI-SDR -------------------------------------------------------------------------------------------------------------------------------------------
def test_si_sdr(backend):
    from deepfilternet_amd import metrics

    snrs = [0.0, 7.5, 20.0, 35.0, 47.0, 60.0]
    lens = [9000, 4097, 8191, 4096, 12_345, 5003]
    T = max(lens) + 5
    r = np.random.default_rng(7)
    ref, est = np.full((len(snrs), T), np.nan, np.float32), np.full((len(snrs), T), np.nan, np.float32)
    for i, (snr, n) in enumerate(zip(snrs, lens)):
        # The formula is scale-invariant only while eps = 1.2e-7 is nothing next to the residual's energy snn: amplitudes of a few units and
        # 4 000 samples or more keep snn > 0.1 at 60 dB, so eps moves the value by less than 1e-5 dB.
        x, _ = _clip(n, 70 + i, amp=20.0)
        d = r.standard_normal(n).astype(np.float32)
        d *= np.sqrt((x.astype(np.float64) ** 2).sum() / max((d.astype(np.float64) ** 2).sum(), 1e-30)) * 10 ** (-snr / 20)
        ref[i, :n], est[i, :n] = x, 0.7 * (x + d)
    tr, te = torch.from_numpy(ref), torch.from_numpy(est)
    got = metrics.si_sdr(tr, te, lengths=lens).cpu().numpy()
    got3 = metrics.si_sdr(tr, 3.0 * te, lengths=lens).cpu().numpy()
    assert got.dtype == np.float32
    for i, n in enumerate(lens):
        want = R.si_sdr(ref[i, :n], est[i, :n])
        print(f"row {i} ({n} samples): got {got[i]!r} float64 formula {want!r} |diff| {abs(got[i] - want):.3e}; 3 x estimate: {got3[i]!r}")
        assert abs(got[i] - want) <= SDR_TOL + SDR_TOL * abs(want)
        assert abs(snrs[i] - want) < 1.0     # (the inputs span 0 to 60 dB)
        assert abs(got3[i] - got[i]) <= SDR_TOL + SDR_TOL * abs(want)
    # estimate == reference: a = 1 exactly, nothing is left: 10 log10((eps + rss) / eps)
    same = metrics.si_sdr(tr, tr.clone(), lengths=lens).cpu().numpy()
    for i, n in enumerate(lens):
        rss = float((ref[i, :n].astype(np.float64) ** 2).sum())
        want = 10 * np.log10((F32_EPS + rss) / F32_EPS)
        assert abs(same[i] - want) <= SDR_TOL + SDR_TOL * abs(want), (i, same[i], want)


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(backend):
    from deepfilternet_amd import _lib, metrics

    x, y = (torch.from_numpy(a) for a in _clip(4000, 1))
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.stoi(x, y[:-1], 10_000)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.si_sdr(x[None], torch.stack([y, y]))
    with pytest.raises(ValueError, match="rows' lengths"):
        metrics.si_sdr([x, x[:100]], [y, y[:99]])
    with pytest.raises(ValueError, match="2 entries for 1 rows"):
        metrics.stoi(x, y, 10_000, lengths=[4000, 4000])
    with pytest.raises(ValueError, match="outside"):
        metrics.si_sdr(x, y, lengths=[4001])
    with pytest.raises(TypeError, match="integers"):
        metrics.stoi(x, y, 10_000, lengths=[4000.0])
    with pytest.raises(TypeError, match="float32 or int16"):
        metrics.stoi(x.double(), y.double(), 10_000)
    with pytest.raises(TypeError, match="tensors"):
        metrics.si_sdr(x.numpy(), y.numpy())
    with pytest.raises(ValueError, match="positive"):
        metrics.stoi(x, y, 0)
    with pytest.raises(ValueError, match="\\[T\\], \\[B, T\\]"):
        metrics.stoi(x[None, None], y[None, None], 10_000)
    small = torch.empty(256, dtype=torch.uint8, device=_lib.device())
    with pytest.raises(ValueError, match="workspace of 256 bytes"):
        metrics.stoi(x, y, 10_000, workspace=small)
    with pytest.raises(ValueError, match="workspace of 256 bytes"):
        metrics.si_sdr(x, y, workspace=small)
    # the C calls themselves
    L = _lib.lib()
    need = C.c_int64()
    assert L.dfx_stoi_workspace_bytes(0, 1, (C.c_int64 * 1)(4000), C.byref(need)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_stoi_workspace_bytes(10_000, 1, (C.c_int64 * 1)(-1), C.byref(need)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_si_sdr_workspace_bytes(1, None, C.byref(need)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_stoi_workspace_bytes(10_000, 0, None, C.byref(need)) == _lib.DFX_OK
    # nothing to score is not an error
    assert tuple(metrics.si_sdr(torch.zeros((0, 10)), torch.zeros((0, 10))).shape) == (0,)
    assert metrics.stoi([], [], 10_000).numel() == 0


def test_score_files_and_cli(backend, tmp_path, capsys):
    from deepfilternet_amd import metrics
    from deepfilternet_amd.io import save_audio

    cdir, edir = tmp_path / "clean", tmp_path / "enh"
    cdir.mkdir(), edir.mkdir()
    want = {}
    for i, n in enumerate((9000, 6500)):
        x, y = _clip(n, 90 + i)
        save_audio(str(cdir / f"c{i}.wav"), torch.from_numpy(x), 16_000, dtype=torch.float32)
        save_audio(str(edir / f"c{i}_DeepFilterNet3.wav"), torch.from_numpy(y[: n - 3 * i]), 16_000, dtype=torch.float32)
        m = n - 3 * i
        want[f"c{i}.wav"] = (R.si_sdr(x[:m], y[:m]), _ref_stoi(x[:m], y[:m], 16_000)[0])
    pairs = metrics.pair_directories(str(cdir), str(edir))
    assert [os.path.basename(e) for _, e in pairs] == ["c0_DeepFilterNet3.wav", "c1_DeepFilterNet3.wav"]
    for (c, _), s in zip(pairs, metrics.score_files(pairs)):
        sd, st = want[os.path.basename(c)]
        assert abs(s["sisdr"] - sd) <= SDR_TOL + SDR_TOL * abs(sd) and abs(s["stoi"] - st) <= CORE_BAR + RESAMPLE_BAR
    csv = tmp_path / "scores.csv"
    assert metrics.main([str(cdir), str(edir), "--csv", str(csv)]) == 0
    lines = csv.read_text().strip().split("\n")
    assert lines[0] == "file,sisdr,stoi" and [ln.split(",")[0] for ln in lines[1:]] == ["c0.wav", "c1.wav"]
    assert "mean over 2 files" in capsys.readouterr().out


def test_lazy_attribute():
    import deepfilternet_amd as d

    assert callable(d.metrics.stoi) and callable(d.metrics.si_sdr) and "metrics" in d.__all__


# ---- GPU only: more than one workgroup per row in every kernel ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_long_rows_on_the_gpu(hip_backend):
    from deepfilternet_amd import metrics

    sr, n = 48_000, 480_000
    clips = [_clip(n - 1000 * i, 200 + i, quiet=((100_000 + 7000 * i, 190_000),)) for i in range(8)]
    lens = [c[0].shape[0] for c in clips]
    cx, cy = torch.zeros((8, n)), torch.zeros((8, n))
    for i, (x, y) in enumerate(clips):
        cx[i, :lens[i]], cy[i, :lens[i]] = torch.from_numpy(x), torch.from_numpy(y)
    v, info = metrics.stoi(cx, cy, sr, lengths=lens, return_info=True)
    s = metrics.si_sdr(cx, cy, lengths=lens)
    for i in (0, 7):
        x, y = clips[i]
        want, winfo = _ref_stoi(x, y, sr)
        print(f"row {i}: got {float(v[i])!r} restatement {want!r} |diff| {abs(float(v[i]) - want):.3e} info {info[i].tolist()}")
        assert info[i].tolist() == winfo.tolist() and abs(float(v[i]) - want) <= CORE_BAR + RESAMPLE_BAR
        va, ia = metrics.stoi(torch.from_numpy(x), torch.from_numpy(y), sr, return_info=True)
        assert _bits(va) == _bits(v[i:i + 1]) and ia[0].tolist() == info[i].tolist()
        assert _bits(metrics.si_sdr(torch.from_numpy(x), torch.from_numpy(y))) == _bits(s[i:i + 1])
        sd = R.si_sdr(x, y)
        assert abs(float(s[i]) - sd) <= SDR_TOL + SDR_TOL * abs(sd)
    # 70 s at 10 kHz: 5 500 windows
    x, y = _clip(700_000, 300, quiet=((50_000, 120_000), (400_000, 400_700)))
    v, info = metrics.stoi(torch.from_numpy(x), torch.from_numpy(y), 10_000, return_info=True)
    want, winfo = _ref_stoi(x, y, 10_000)
    print(f"70 s: got {float(v[0])!r} restatement {want!r} |diff| {abs(float(v[0]) - want):.3e} info {info[0].tolist()}")
    assert info[0].tolist() == winfo.tolist() and info[0, 0].item() > 5400 and abs(float(v[0]) - want) <= CORE_BAR
