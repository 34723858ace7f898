"""The pre-split copy of feat_spec (8 bytes per complex value: the f16 hi halves of (re, im), then the lo halves — dfx_pack_h3, written by the
norm scan in enhance() and by dfx_k_pack_h3 for a caller's own features) and the PS instances of dfx_k_df_enc_h3 / dfx_k_df_convp_h3 that read
it in batch passes, against the instances that split every 3x3 patch themselves (test hook DFX_C0_PRESPLIT=0, read when the model handle is
created): the same operand bits in, so the same bits out, everywhere.

Shapes: the smallest at which these kernels take another path.  Frames per clip of the pass: 5 (shorter than df_convp's five-frame window plus
the lookahead: every frame is an edge frame), 17 (a 16-frame tile of dfx_k_df_enc_h3 plus one live lane in the next), 41 and 83 (df_convp's
segments of 40 frames: one and two boundaries).  Clips: 1, 3, and 17 (B * T no multiple of 16: dead lanes in the last tile)."""
import numpy as np
import pytest
import torch

from tests.helpers import named_params

HOP = 480
SEED = 23


def _noise(shape, seed):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32))


def _init(monkeypatch, presplit):
    """(p, model, df_state) of DeepFilterNet3 with seeded weights; presplit False: DFX_C0_PRESPLIT=0 while the handle is created"""
    from deepfilternet_amd.enhance import init_df

    if presplit:
        monkeypatch.delenv("DFX_C0_PRESPLIT", raising=False)
    else:
        monkeypatch.setenv("DFX_C0_PRESPLIT", "0")
    p = named_params("df3")
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=SEED)
    monkeypatch.delenv("DFX_C0_PRESPLIT", raising=False)
    return p, model, df_state


@pytest.fixture
def both(backend, monkeypatch):
    """(p, default model, its state, DFX_C0_PRESPLIT=0 model, its state) on the fixture's backend"""
    p, ps, st_p = _init(monkeypatch, True)
    _, un, st_u = _init(monkeypatch, False)
    return p, ps, st_p, un, st_u


def _ran(ps, un, passes):
    """the two handles ran the two forms: every pass of the default handle read the pre-split copy, none of the other's did"""
    assert ps.query(ps.Q_PASSES_C0_PRESPLIT) == passes and un.query(un.Q_PASSES_C0_PRESPLIT) == 0


def _samples(frames):
    return HOP * (frames - 2)   # enhance(pad=True) adds fft_size = 2 hops: `frames` STFT frames per clip in the pass


def _cases(emu, hip):
    """(backend, B, frames) triples: `emu` on the CPU interpreter (a pass costs ~0.5 s per frame there), `emu + hip` on the GPU"""
    return [pytest.param("emu", b, t) for b, t in emu] + [pytest.param("hip", b, t, marks=pytest.mark.gpu) for b, t in emu + hip]


@pytest.mark.parametrize("backend,B,frames", _cases([(1, 5), (3, 17), (17, 5), (1, 41)], [(1, 83), (17, 41), (3, 83), (17, 83)]), indirect=["backend"])
def test_enhance_waveforms_bit_equal(both, B, frames):
    from deepfilternet_amd.enhance import enhance

    p, ps, st_p, un, st_u = both
    x = _noise((B, _samples(frames) + 7), 100 * B + frames)
    y_p, y_u = enhance(ps, st_p, x), enhance(un, st_u, x)
    ps.check(), un.check()
    _ran(ps, un, 1)
    assert float(y_p.abs().max()) > 1e-5
    assert torch.equal(y_p, y_u)


@pytest.mark.parametrize("backend,B,T", _cases([(17, 5), (1, 17), (1, 41)], [(3, 41), (1, 83), (17, 17)]), indirect=["backend"])
def test_forward_outputs_bit_equal(both, B, T):
    """DfNet.forward on the caller's own features (the copy is made by dfx_k_pack_h3): enhanced spectrum, mask, lsnr and DF coefficients"""
    p, ps, _, un, _ = both
    rng = np.random.default_rng(1000 * B + T)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy(rng.standard_normal((B, 1, T, p.nb_df, 2)).astype(np.float32))
    out_p, out_u = ps(spec, fe, fs), un(spec, fe, fs)
    ps.check(), un.check()
    _ran(ps, un, 1)
    for name, a, b in zip(("spec_e", "mask", "lsnr", "df_coefs"), out_p, out_u):
        assert float(a.abs().max()) > 0, name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("backend,frames", [pytest.param("emu", (17, 7, 5)), pytest.param("hip", (17, 7, 5), marks=pytest.mark.gpu),
                                            pytest.param("hip", (83, 41, 5), marks=pytest.mark.gpu)], indirect=["backend"])
def test_rows_of_different_lengths(both, frames):
    """One enhance_batch call with rows of 83, 41 and 5 frames (17, 7 and 5 on the interpreter too): one pass over the frames of the longest
    row; the pre-split copy past a row's end is zero words, as feat_spec is zeros there."""
    from deepfilternet_amd.enhance import enhance_batch

    p, ps, st_p, un, st_u = both
    clips = [_noise((_samples(f) + k,), 40 + f) for f, k in zip(frames, (3, 0, 11))]
    ys_p, ys_u = enhance_batch(ps, st_p, clips), enhance_batch(un, st_u, clips)
    ps.check(), un.check()
    _ran(ps, un, 1)
    for c, a, b in zip(clips, ys_p, ys_u):
        assert a.shape == c.shape and float(a.abs().max()) > 1e-5
        assert torch.equal(a, b)
    # and the shortest row equals a pass of its own
    from deepfilternet_amd.enhance import enhance

    assert torch.equal(ys_p[2], enhance(ps, st_p, clips[2][None])[0])


@pytest.mark.parametrize("presplit", [True, False])
def test_range_guard(backend, monkeypatch, presplit):
    """The range guard of the patch split sits where the split is made: one feature value of 6.1e4 (>= DFX_H3_LIMIT = 6e4) fails check() with the
    fp16-split range error in both settings of the hook; with 5e4 as the largest value the pass is clean."""
    from deepfilternet_amd import _lib

    p, model, _ = _init(monkeypatch, presplit)
    B, T = 1, 17
    rng = np.random.default_rng(9)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy((1e-3 * rng.standard_normal((B, 1, T, p.nb_df, 2))).astype(np.float32))   # (small: c0 itself stays far from the limit)
    hot = fs.clone()
    hot[0, 0, 9, 50, 1] = 6.1e4
    with pytest.raises(_lib.DfxError, match="fp16-split"):
        model(spec, fe, hot)
        model.check()
    try:            # (a later kernel of the same pass may raise the word again after the first report)
        model.check()
    except _lib.DfxError:
        pass
    model.check()   # the report cleared the word
    ok = fs.clone()
    ok[0, 0, 9, 50, 1] = 5.0e4
    out = model(spec, fe, ok)
    model.check()
    assert all(bool(torch.isfinite(o).all()) for o in out)


@pytest.mark.parametrize("presplit", [True, False])
def test_range_guard_in_enhance(backend, monkeypatch, presplit):
    """enhance() of samples around 1e12 (spectrum magnitudes around 2e10): the unit-normed features, x / sqrt(running mean of |x|) — 10 sqrt|x| in
    the first frame, sqrt|x| later: 1e5 ... 1e6 — leave the f16 range.  In a default pass the
    guard of the patch split is the norm scan's (dfx_k_norm_scan4 with the model's error words: 17 frames), with the hook the c0 kernels' own; both
    report through check().  (Not an isolated trigger of the scan's guard: c0 of such features is out of range for the later splits as well.)"""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import enhance

    p, model, df_state = _init(monkeypatch, presplit)
    x = 1e13 * _noise((1, _samples(17)), 77)
    with pytest.raises(_lib.DfxError, match="fp16-split"):
        enhance(model, df_state, x)
        model.check()
    try:
        model.check()
    except _lib.DfxError:
        pass
    model.check()
    y = enhance(model, df_state, _noise((1, _samples(17)), 78))   # the handle is fine afterwards
    model.check()
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 1e-5


def test_range_guard_outputs_equal_below_the_limit(both):
    """Features with 5e4 as the largest value: clean in both forms, and the same bits."""
    p, ps, _, un, _ = both
    B, T = 1, 17
    rng = np.random.default_rng(10)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy((1e-3 * rng.standard_normal((B, 1, T, p.nb_df, 2))).astype(np.float32))
    fs[0, 0, 3, 0, 0] = -5.0e4
    out_p, out_u = ps(spec, fe, fs), un(spec, fe, fs)
    ps.check(), un.check()
    for name, a, b in zip(("spec_e", "mask", "lsnr", "df_coefs"), out_p, out_u):
        assert torch.equal(a, b), name


def test_exact_fp32_and_streams_keep_the_fp32_features(backend, monkeypatch):
    """DFX_EXACT_FP32=1 and the streaming runtime never read the pre-split copy."""
    from deepfilternet_amd.enhance import enhance
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _init(monkeypatch, True)
    x = _noise((2, HOP * 6), 5)
    rt = DfStream(model, df_state, streams=2, max_frames=3)
    for c in x.split(3 * HOP, dim=1):
        rt.process(c)
    model.check()
    assert model.query(model.Q_PASSES_C0_PRESPLIT) == 0
    monkeypatch.setenv("DFX_EXACT_FP32", "1")
    _, exact, st_e = _init(monkeypatch, True)
    enhance(exact, st_e, x)
    exact.check()
    assert exact.query(exact.Q_PASSES_C0_PRESPLIT) == 0
