"""enhance_long: enhance() of clips of any length through the slots of one DfStream in bounded memory, and the routing that takes enhance(),
enhance_batch() and enhance_files() there with a clip whose workspace does not fit the cap alone — where they raised MemoryError before.

The reference is the oracle's enhance() of each clip on its own; the bound 3e-6 RMS is the one of tests/test_stream_ends.py (2e-6 batch path
against oracle + 1e-6 stream against batch, tests/test_streaming.py:35-36).  16-bit results are compared with float_to_pcm16 of the oracle's
float result: at most one LSB apart at every sample (a rounding difference that crosses a truncation boundary), no cap on how many."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from tests.helpers import emu_subset, named_params, rms, torch_sd
from tests.scratch_fill import FILLS, assert_same_bits, fresh_memory, set_fill

HOP = 480
BOUND = 3e-6
SEED = 9
LENGTHS = (0, 77, 960, 961, HOP * 6 + 5, HOP * 23 + 100)
# (length index, channels — 0: a 1-D clip —, 16-bit, on the device where there is one, page-locked)
LAYOUT = ((0, 1, False, False, False), (1, 2, False, True, False), (2, 0, True, False, False), (3, 1, False, False, True),
          (4, 2, True, True, False), (5, 0, False, False, False), (3, 1, True, False, True))
_refs = {}


def _model_name(backend):
    return "pf32_nopf" if backend == "emu" else "df3"


def _clips(backend):
    """7 clips, 9 rows — more rows than the 3 slots — float32 and int16, host (pageable and page-locked) and device mixed."""
    from deepfilternet_amd import _lib

    rng = np.random.default_rng(4)
    cuda = _lib.device().type == "cuda"
    clips = []
    for li, ch, pcm16, on_dev, pinned in LAYOUT:
        a = torch.from_numpy((0.1 * rng.standard_normal((max(ch, 1), LENGTHS[li]))).astype(np.float32))
        if pcm16:
            a = (a * 32768).to(torch.int16)
        if ch == 0:
            a = a[0]
        if cuda and on_dev:
            a = a.to(_lib.device())
        elif cuda and pinned:
            a = a.pin_memory()
        clips.append(a)
    return clips


def _oracle(name, clip_id, clip, pad, atten):
    """The oracle's float result [C, out] of one clip, computed once per (model, clip, pad, limit)."""
    key = (name, clip_id, pad, atten)
    if key not in _refs:
        p = named_params(name)
        x = clip.detach().cpu()
        x = (x.float() / 32768 if x.dtype == torch.int16 else x)
        x = (x if x.dim() == 2 else x[None]).numpy()
        out_len = x.shape[1] if pad else x.shape[1] // HOP * HOP
        _refs[key] = O.enhance(p, torch_sd(p, SEED), x, pad=pad, atten_lim_db=atten) if out_len else np.zeros((x.shape[0], 0), np.float32)
    return _refs[key]


def _check(got, clip, ref, what):
    assert got.dtype == clip.dtype and got.device == clip.device and got.dim() == clip.dim(), what
    assert got.is_pinned() == clip.is_pinned(), what
    g = got.detach().cpu()
    g = (g if g.dim() == 2 else g[None]).numpy()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    if g.size == 0:
        return
    if got.dtype == torch.int16:
        want = np.trunc(ref.astype(np.float32) * np.float32(32768)).astype(np.int64)   # float_to_pcm16: truncation toward zero
        d = np.abs(g.astype(np.int64) - want)
        print(f"  {what}: 16-bit, {int((d > 0).sum())} of {d.size} samples one LSB off")
        assert d.max() <= 1, (what, int(d.max()))
    else:
        err = rms(g - ref)
        print(f"  {what}: rms error {err:.3e}")
        assert err < BOUND, (what, err)


CASES = [(pad, atten) for pad in (True, False) for atten in (None, 12, 0.005)]
EMU_CASES = {(True, None), (False, 12), (True, 0.005)}


@pytest.mark.parametrize("pad,atten", CASES)
def test_enhance_long_matches_the_oracle(backend, pad, atten):
    from deepfilternet_amd import enhance as E
    from deepfilternet_amd.enhance import enhance_long, init_df

    if emu_subset(backend) and (pad, atten) not in EMU_CASES:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it); every case runs on the GPU")
    name = _model_name(backend)
    model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=SEED)
    clips = _clips(backend)
    outs = enhance_long(model, df_state, clips, pad=pad, atten_lim_db=atten, slots=3, hops_per_call=5)
    assert E.last_long_plan["slots"] == 3 and E.last_long_plan["hops_per_call"] == 5
    assert len(outs) == len(clips)
    for i, (o, c) in enumerate(zip(outs, clips)):
        _check(o, c, _oracle(name, i, c, pad, atten), f"clip {i} {tuple(c.shape)} pad={pad} atten={atten}")
    # (atten 0.005: the runtime's handle-wide rule would pass the input through UNDELAYED — every window one lookahead off, far outside the
    # bound — and the per-stream rule would mix with 0.99999994; enhance()'s own mix is 10^(-0.005 / 20) = 0.99942, which is what the oracle applies)
    model.check()


def test_a_limit_of_100_db_is_a_limit(backend):
    """enhance() mixes with 10^(-|dB| / 20) whatever the value (df/enhance.py:238-240): at 100 dB that is 1e-5 of the noisy signal, where the
    stream runtime's own rule (tract.rs:387-398) switches the limit off.  Against the oracle the two lie inside one bound of each other, so the
    mix itself is checked: result(100 dB) - result(no limit) = 1e-5 * (noisy - result(no limit)), to a tenth of its size (float32 rounding of
    samples of 0.1 is 1e-8, the term 1e-6).  And the handle reports what is in force."""
    from deepfilternet_amd.enhance import enhance_long, init_df
    from deepfilternet_amd.streaming import DfStream

    name = _model_name(backend)
    model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=SEED)
    x = torch.from_numpy((0.1 * np.random.default_rng(3).standard_normal((2, HOP * (4 if backend == "emu" else 9) + 33))).astype(np.float32))
    (y_off,) = enhance_long(model, df_state, [x], slots=2, hops_per_call=5)
    (y_100,) = enhance_long(model, df_state, [x], atten_lim_db=100, slots=2, hops_per_call=5)
    ref = _oracle(name, "lim100", x, True, 100)
    assert rms(y_100.numpy() - ref) < BOUND
    term = 1e-5 * (x - y_off).numpy()
    miss = rms((y_100 - y_off).numpy() - term)
    print(f"  100 dB: the mixed-in term has {rms(term):.3e} rms, the result misses it by {miss:.3e}")
    assert rms(term) > 3e-7 and miss < 0.1 * rms(term), (miss, rms(term))
    rt = DfStream(model, df_state, streams=2, max_frames=2)
    for given, said in ((120.0, 120.0), (-12.0, 12.0), (0.005, 0.005), (None, 100.0), (0.0, 100.0)):
        rt.set_atten_lim_enhance(given)
        assert rt.settings["atten_lim_db"].tolist() == pytest.approx([said] * 2), given
    model.check()


def test_two_plans_agree(backend):
    """(3 slots, 5 hops) and (2 slots, 7 hops): other cuts, other slot assignments, the same samples to 1e-6 RMS (tests/test_streaming.py:36)."""
    from deepfilternet_amd.enhance import enhance_long, init_df

    name = _model_name(backend)
    model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=SEED)
    clips = [c for c in _clips(backend) if c.dtype == torch.float32 and c.shape[-1] >= 960][: (2 if backend == "emu" else 4)]
    a = enhance_long(model, df_state, clips, slots=3, hops_per_call=5)
    b = enhance_long(model, df_state, clips, slots=2, hops_per_call=7)
    for u, v in zip(a, b):
        err = rms((u.cpu() - v.cpu()).numpy())
        print(f"  {tuple(u.shape)}: the two plans differ by {err:.3e} rms")
        assert err < 1e-6, err
    model.check()


def test_post_filter_models_are_served(backend):
    """mask_pf: the stream runtime's post filter is libDF's, which leaves the last (ch * F) % 4 bins of a frame alone, enhance()'s the PyTorch
    model's on every bin: 1e-4 apart at most, as tests/test_streaming.py:43 grants."""
    from deepfilternet_amd.enhance import enhance, enhance_long, init_df

    model, df_state, _, _ = init_df(params=named_params("pf32"), epoch="none", seed=SEED)
    x = torch.from_numpy((0.1 * np.random.default_rng(6).standard_normal((2, HOP * 6 + 5))).astype(np.float32))
    (y,) = enhance_long(model, df_state, [x], slots=3, hops_per_call=4)
    ref = enhance(model, df_state, x)
    err = rms((y - ref).numpy())
    print(f"  pf32: enhance_long against enhance() {err:.3e} rms")
    assert y.shape == ref.shape and err < 1e-4, err
    model.check()


def _bytes(fn, *args):
    from deepfilternet_amd import _lib

    n = C.c_int64()
    _lib.check(getattr(_lib.lib(), fn)(*args, C.byref(n)))
    return int(n.value)


def _write_wav(path, pcm, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1]), w.setsampwidth(2), w.setframerate(sr)
        w.writeframes(pcm.astype("<i2").tobytes())


def test_a_clip_that_does_not_fit_takes_the_long_path(backend, monkeypatch, tmp_path):
    """Under a cap below one clip's enhance() workspace but above a one-slot, 16-hop stream handle, enhance(), enhance_batch() and
    enhance_files() return — each raised MemoryError before — within the bound, on a handle under the cap; under a cap of one byte
    MemoryError stays."""
    from deepfilternet_amd import enhance as E
    from deepfilternet_amd.io import load_audio

    name = _model_name(backend)
    p = named_params(name)
    sd = torch_sd(p, SEED)
    model, df_state, _, _ = E.init_df(params=p, epoch="none", seed=SEED)
    T = HOP * 30 + 33
    ws_one = _bytes("dfx_enhance_workspace_bytes", model.handle, df_state.handle, 1, T, 1)
    handle_min = _bytes("dfx_stream_memory_bytes", model.handle, df_state.handle, 1, 16)
    assert handle_min < ws_one, (handle_min, ws_one)
    cap = (handle_min + ws_one) // 2
    rng = np.random.default_rng(12)
    x = torch.from_numpy((0.1 * rng.standard_normal((1, T))).astype(np.float32))
    short = torch.from_numpy((0.1 * rng.standard_normal((2, HOP * 3 + 9))).astype(np.float32))
    ref, ref_short = O.enhance(p, sd, x.numpy()), O.enhance(p, sd, short.numpy())
    monkeypatch.setenv("DFX_WORKSPACE_CAP_GB", repr(cap / (1 << 30)))
    model._ws = None

    def under_cap():
        plan = dict(E.last_long_plan)
        E.last_long_plan.clear()
        assert plan and plan["bytes"] <= cap, (plan, cap)
        assert plan["bytes"] == _bytes("dfx_stream_memory_bytes", model.handle, df_state.handle, plan["slots"], plan["hops_per_call"])

    y = E.enhance(model, df_state, x)
    assert y.shape == x.shape and y.dtype == x.dtype and y.device == x.device
    err = rms(y.numpy() - ref)
    print(f"  enhance() under a cap of {cap} bytes (workspace of the clip {ws_one}, smallest handle {handle_min}): rms error {err:.3e}")
    assert err < BOUND, err
    under_cap()
    # enhance_batch: the clip that fits keeps its pass, the one that does not takes the long path
    got_short, got = E.enhance_batch(model, df_state, [short, x[0]])
    assert got.shape == (T,) and rms(got.numpy() - ref[0]) < BOUND and rms(got_short.numpy() - ref_short) < 2e-6
    under_cap()
    # enhance_files: one 16-bit file at the model's rate
    pcm = (0.1 * rng.standard_normal((T, 1)) * 32768).astype("<i2")
    path = str(tmp_path / "long.wav")
    _write_wav(path, pcm, p.sr)
    (out,) = E.enhance_files(model, df_state, [path], output_dir=str(tmp_path), suffix="x")
    under_cap()
    monkeypatch.delenv("DFX_WORKSPACE_CAP_GB")
    back, _ = load_audio(out, sr=p.sr, verbose=False, pcm16=True)
    want = np.trunc(O.enhance(p, sd, (pcm.T.astype(np.float32) / 32768)) * np.float32(32768)).astype(np.int64)
    d = np.abs(back.cpu().numpy().astype(np.int64) - want)
    print(f"  enhance_files: {int((d > 0).sum())} of {d.size} samples one LSB off")
    assert back.dtype == torch.int16 and d.shape == (1, T) and d.max() <= 1
    monkeypatch.setenv("DFX_WORKSPACE_CAP_GB", "1e-9")
    for call in (lambda: E.enhance(model, df_state, x), lambda: E.enhance_batch(model, df_state, [x]), lambda: E.enhance_long(model, df_state, [x])):
        with pytest.raises(MemoryError):
            call()
    model.check()


def test_enhance_long_ignores_scratch_contents(backend, monkeypatch):
    """Staging buffers, call inputs and outputs from filled memory, the handle's model workspace filled by the engine: the same bits whatever
    the fill (tests/test_scratch_contents.py)."""
    from deepfilternet_amd.enhance import enhance_long, init_df

    name = _model_name(backend)
    clips = [c for c in _clips(backend) if c.shape[-1] in (77, 961, HOP * 6 + 5)][: (3 if backend == "emu" else 4)]   # (float and 16-bit rows in both)
    assert len(clips) >= 3
    outs = {}
    for fill in (None,) + FILLS:
        set_fill(monkeypatch, fill)
        model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=SEED)
        with fresh_memory(fill):
            y = enhance_long(model, df_state, clips, slots=3, hops_per_call=4)
        model.check()
        outs[fill] = tuple(o.cpu() for o in y)
    set_fill(monkeypatch, None)
    assert_same_bits(outs, "enhance_long")
