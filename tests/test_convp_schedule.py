"""The frame loop of the PS instance of dfx_k_df_convp_h3 (what every batch pass runs: a frame's outputs held and stored in the next frame's body,
the patch loads requested two frames ahead and zero-selected where they are used, the older frames' taps in front of c0's epilogue, the frames of
a round nested) against the unsplit instance, which keeps
the loop as it was (test hook DFX_C0_PRESPLIT=0, read when the model handle is created): the same products in the same order per accumulator, so
the same bits, at the shapes where the new loop has seams.

Frames per clip of the pass: 1, 2, 3 (shorter than the five-frame window and than the distance the patches are requested ahead: every frame is a
first, a last and a warm-up neighbour at once), 6 ... 9 (one segment whose last group of five is partial: 1 ... 4 frames), 42 and 44 (segments of
40 frames: a boundary — the held outputs of a segment's last frame are flushed, the next segment starts with none — and a partial tail), three
clips with DFX_CONVP_ELEMS small enough that df_convp runs as one launch per clip, and one enhance_batch call with rows of 9, 7 and 1 frames."""
import numpy as np
import pytest
import torch

from tests.helpers import named_params

HOP = 480
SEED = 29


def _noise(shape, seed):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32))


def _init(monkeypatch, presplit, env=()):
    """(p, model, df_state) of DeepFilterNet3 with seeded weights; presplit False: DFX_C0_PRESPLIT=0 while the handle is created (`env`: further
    hooks set for that time)"""
    from deepfilternet_amd.enhance import init_df

    if presplit:
        monkeypatch.delenv("DFX_C0_PRESPLIT", raising=False)
    else:
        monkeypatch.setenv("DFX_C0_PRESPLIT", "0")
    for k, v in env:
        monkeypatch.setenv(k, v)
    p = named_params("df3")
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=SEED)
    monkeypatch.delenv("DFX_C0_PRESPLIT", raising=False)
    for k, _ in env:
        monkeypatch.delenv(k, raising=False)
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


def _cases(emu, hip):
    """(backend, B, T) triples: `emu` on the CPU interpreter (a pass costs ~0.5 s per frame there), `emu + hip` on the GPU"""
    return [pytest.param("emu", b, t) for b, t in emu] + [pytest.param("hip", b, t, marks=pytest.mark.gpu) for b, t in emu + hip]


def _features(p, B, T):
    rng = np.random.default_rng(1000 * B + T)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy(rng.standard_normal((B, 1, T, p.nb_df, 2)).astype(np.float32))
    return spec, fe, fs


def _forward_equal(p, ps, un, B, T):
    """DfNet.forward on the caller's own features: the DF coefficients (df_convp's output through df_out) and everything else, bit for bit"""
    spec, fe, fs = _features(p, B, T)
    out_p, out_u = ps(spec, fe, fs), un(spec, fe, fs)
    ps.check(), un.check()
    _ran(ps, un, 1)
    names = ("spec_e", "mask", "lsnr", "df_coefs")
    assert float(out_p[3].abs().max()) > 0
    for name, a, b in zip(names, out_p, out_u):
        assert a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("backend,B,T", _cases([(1, 1), (1, 2), (2, 3)], [(3, 1), (3, 2)]), indirect=["backend"])
def test_passes_shorter_than_the_window(both, B, T):
    p, ps, _, un, _ = both
    _forward_equal(p, ps, un, B, T)


@pytest.mark.parametrize("backend,B,T", _cases([(1, 6), (1, 7), (1, 8), (1, 9)], [(3, 6), (3, 7), (3, 8), (3, 9)]), indirect=["backend"])
def test_one_segment_with_a_partial_last_group(both, B, T):
    p, ps, _, un, _ = both
    _forward_equal(p, ps, un, B, T)


@pytest.mark.parametrize("backend,B,T", _cases([], [(1, 42), (1, 44), (3, 42), (3, 44)]), indirect=["backend"])
def test_two_segments(both, B, T):
    p, ps, _, un, _ = both
    _forward_equal(p, ps, un, B, T)


@pytest.mark.parametrize("backend,B,T", _cases([(3, 6)], [(3, 9), (3, 44)]), indirect=["backend"])
def test_launch_split_over_clips(backend, monkeypatch, B, T):
    """DFX_CONVP_ELEMS one above a clip's element count: one clip per launch, three launches"""
    from deepfilternet_amd import _lib

    p = named_params("df3")
    env = (("DFX_CONVP_ELEMS", str(T * p.nb_df + 1)),)
    _, ps, _ = _init(monkeypatch, True, env)
    _, un, _ = _init(monkeypatch, False, env)
    _forward_equal(p, ps, un, B, T)
    if not _lib.is_emulator():   # (a third handle and pass: on the GPU only) and the three launches give what one launch gives
        _, whole, _ = _init(monkeypatch, True)
        spec, fe, fs = _features(p, B, T)
        assert torch.equal(ps(spec, fe, fs)[3], whole(spec, fe, fs)[3])


@pytest.mark.parametrize("backend,frames", [pytest.param("emu", (7,)), pytest.param("hip", (6, 9), marks=pytest.mark.gpu),
                                            pytest.param("hip", (42, 44), marks=pytest.mark.gpu)], indirect=["backend"])
def test_enhance_waveforms_bit_equal(both, frames):
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import enhance

    p, ps, st_p, un, st_u = both
    for n, f in enumerate(frames):
        x = _noise((1 if _lib.is_emulator() else 2, HOP * (f - 2) + 7), 100 + f)   # enhance(pad=True) adds fft_size = 2 hops: f STFT frames per clip in the pass
        y_p, y_u = enhance(ps, st_p, x), enhance(un, st_u, x)
        ps.check(), un.check()
        _ran(ps, un, n + 1)
        assert float(y_p.abs().max()) > 1e-5
        assert torch.equal(y_p, y_u)


@pytest.mark.parametrize("backend", [pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)
def test_rows_of_9_7_and_1_frames(both):
    """One enhance_batch call (pad=False: a row of 480 ... 959 samples is one frame) with rows of 9, 7 and 1 frames: one pass over the frames of the
    longest row; the shortest row's only frame is its first and its last."""
    from deepfilternet_amd.enhance import enhance, enhance_batch

    p, ps, st_p, un, st_u = both
    clips = [_noise((HOP * f + k,), 40 + f) for f, k in ((9, 3), (7, 0), (1, 11))]
    ys_p, ys_u = enhance_batch(ps, st_p, clips, pad=False), enhance_batch(un, st_u, clips, pad=False)
    ps.check(), un.check()
    _ran(ps, un, 1)
    for c, a, b in zip(clips, ys_p, ys_u):
        assert a.shape == (c.shape[0] // HOP * HOP,)
        assert torch.equal(a, b)
    assert float(ys_p[0].abs().max()) > 1e-5
    assert torch.equal(ys_p[2], enhance(ps, st_p, clips[2][None], pad=False)[0])   # and the shortest row equals a pass of its own
