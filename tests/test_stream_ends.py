"""Clips that end inside a stream call (dfx_stream_process_ends, DfStream.process(valid_hops=...)): behind a row's last frame the pass sees
the batch path's zero padding — spectrum and normalised features — so the row's output is enhance(pad=False) of exactly its own frames,
delayed by the lookahead, the last `lookahead` frames included: the part no stream call could produce before.

The reference is the oracle's enhance() of each clip on its own.  The bound is the sum of two the project already holds at this signal
scale (0.1 * standard_normal): 2e-6 RMS batch path against oracle (tests/test_streaming.py:35) + 1e-6 stream against batch (:36) = 3e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from tests.helpers import emu_subset, named_params, rms, torch_sd

HOP, N_FFT = 480, 960
BOUND = 3e-6
LENGTHS = (HOP * 9 + 17, HOP * 5, HOP * 7 + 479)
SEED = 9
# Call sizes (16 hops in all; 3 slots, max_frames 7).  With the rows' frame counts — 11, 7, 9 padded and 9, 5, 7 unpadded — an end falls
#   [4,4,4,4]   on the first hop of a call (v = 1: 9 frames) and on the hop before a call's last (v = n - 1: 11, 7);
#   [7,4,5]     exactly on a call boundary (v = n, then v = 0: 7 and 11 frames) and in the middle (9: v = 2 of 4; 5: v = 5 of 7);
#   [6,5,5]     on the first hop (7 frames: v = 1), on a boundary (11) and on the hop before the last (5 frames: v = 5 of 6);
#   [5,4,2,5]   on boundaries of short calls (9, 11 frames; 5, 9 unpadded);   [1] * 16: one-hop calls, every end a boundary.
CUTS = ([4, 4, 4, 4], [7, 4, 5], [6, 5, 5], [5, 4, 2, 5], [1] * 16)
EMU_CUTS = CUTS[:2]   # (the interpreter is slow: first hop, hop before the last and call boundary are all in these two)


def _models(backend):
    return ("pf32_nopf",) if backend == "emu" else ("defaults", "df3", "pf32_nopf")


def _rows(seed=2):
    rng = np.random.default_rng(seed)
    return [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in LENGTHS]


def _frames(t, pad):
    return (t + (N_FFT if pad else 0)) // HOP   # enhance.py:230-235


def _feed(rt, rows, pad, cuts, ends=True, dtype=torch.float32, first=0):
    """The rows through the handle as enhance_long feeds them: zeros behind a row's own samples, valid_hops from its frame count.
    first[b]: hops the slot's row starts behind the feed's start (a row that takes a slot later).  -> the stream's output [rows, hops * HOP]"""
    total = sum(cuts)
    first = [first] * len(rows) if isinstance(first, int) else first
    x = torch.zeros((len(rows), total * HOP), dtype=dtype)
    for b, r in enumerate(rows):
        t = torch.from_numpy(r) if isinstance(r, np.ndarray) else r
        x[b, first[b] * HOP: first[b] * HOP + t.shape[0]] = t[: (total - first[b]) * HOP]
    out, pos = [], 0
    for n in cuts:
        valid = None
        if ends:
            valid = [min(n, max(0, first[b] + _frames(len(r), pad) - pos)) for b, r in enumerate(rows)]
        out.append(rt.process(x[:, pos * HOP:(pos + n) * HOP], valid_hops=valid))
        pos += n
    return torch.cat(out, dim=1)


def _window(y, t, pad, look, first=0):
    """A row's part of the stream's output: enhance.py:248-249 behind the lookahead"""
    o0 = (first + look) * HOP + (N_FFT - HOP if pad else 0)
    return y[o0: o0 + (t if pad else t // HOP * HOP)]


@pytest.mark.parametrize("pad", [True, False])
def test_ends_give_the_whole_clip(backend, pad):
    """Every row within 3e-6 RMS of the oracle over the whole clip and over its last (lookahead + 2) hops alone, under every cut; and the test
    can see the rule: the same feed without valid_hops — plain zeros behind the clips — misses a tail by at least 20 bounds (models with a
    lookahead).  On the interpreter, pf32_nopf with seed 9: 5.0e-3 to 5.2e-3 on every row unpadded; padded 3.7e-4 on the row whose last hop
    is nearly full (480 * 7 + 479 samples) and nothing on the others — enhance()'s own padding is two frames, so with one frame of lookahead only
    the samples of a clip's last, partial hop read a frame behind the end.  So there, and only there, the largest row's figure is asserted;
    unpadded, and with two frames of lookahead (df3: 2.8e-4 to 1.6e-3 padded, 7.9e-3 to 1.4e-2 unpadded on the GPU), every row must miss."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    rows = _rows()
    for name in _models(backend):
        p = named_params(name)
        sd = torch_sd(p, SEED)
        model, df_state, _, _ = init_df(params=p, epoch="none", seed=SEED)
        refs = [O.enhance(p, sd, r[None], pad=pad)[0] for r in rows]
        rt = DfStream(model, df_state, streams=3, max_frames=7)
        look = rt.delay_frames
        tail = (look + 2) * HOP
        for cuts in (EMU_CUTS if emu_subset(backend) else CUTS):
            rt.reset()
            y = _feed(rt, rows, pad, cuts).numpy()
            for b, (r, ref) in enumerate(zip(rows, refs)):
                got = _window(y[b], len(r), pad, look)
                assert got.shape == ref.shape
                e_all, e_tail = rms(got - ref), rms(got[-tail:] - ref[-tail:])
                print(f"  {name} pad={pad} cuts={cuts} row {b}: rms error {e_all:.3e}, last {look + 2} hops {e_tail:.3e}")
                assert e_all < BOUND and e_tail < BOUND, (name, cuts, b, e_all, e_tail)
        if look > 0:
            rt.reset()
            y = _feed(rt, rows, pad, CUTS[0], ends=False).numpy()
            blind = [rms(_window(y[b], len(r), pad, look)[-tail:] - ref[-tail:]) for b, (r, ref) in enumerate(zip(rows, refs))]
            print(f"  {name} pad={pad}, zeros without valid_hops: last {look + 2} hops " + ", ".join(f"{e:.3e}" for e in blind))
            # every row must show it — except padded with ONE frame of lookahead (see above), where only the fullest last hop can
            seen = max(blind) if (pad and look == 1) else min(blind)
            assert seen >= 20 * BOUND, (name, blind)
        model.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "pcm16"])
def test_no_ends_is_plain_process(backend, dtype):
    """valid_hops=None and valid_hops=[n] * streams enqueue what process() enqueues: the same bits, float and 16-bit."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    name = "pf32_nopf" if backend == "emu" else "df3"
    model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=SEED)
    T = 9
    x = torch.from_numpy((0.1 * np.random.default_rng(5).standard_normal((3, HOP * T))).astype(np.float32))
    if dtype == torch.int16:
        x = (x * 32768).to(torch.int16)
    cuts = [1, 3, 1, 4]
    outs = []
    for mode in ("plain", "none", "all"):
        rt = DfStream(model, df_state, streams=3, max_frames=4)
        out, pos = [], 0
        for n in cuts:
            fr = x[:, pos * HOP:(pos + n) * HOP]
            out.append(rt.process(fr) if mode == "plain" else rt.process(fr, valid_hops=None if mode == "none" else [n] * 3))
            pos += n
        outs.append(torch.cat(out, dim=1))
    assert outs[0].dtype == dtype and float(outs[0].float().abs().max()) > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    model.check()


def test_an_ended_slot_serves_a_second_clip(backend):
    """Row 1 ends, its slot is reset while the others run on and takes a second clip, which ends too — inside the one-hop passes of the others'
    calls that its warm-up forces; an ended row refuses a count other than 0 until it is reset."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    name = "pf32_nopf" if backend == "emu" else "df3"
    p = named_params(name)
    sd = torch_sd(p, SEED)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=SEED)
    rng = np.random.default_rng(11)
    # (slot 2's clip has 9 frames: it ends on the first hop behind the reset, inside the one-hop passes of slot 1's warm-up)
    long_a, long_b = [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in (HOP * 13 + 5, HOP * 7 + 40)]
    first_clip, second_clip = [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in (HOP * 2 + 100, HOP * 3 + 7)]
    rt = DfStream(model, df_state, streams=3, max_frames=5)
    look = rt.delay_frames
    pad = True
    # calls of 5, 3 | reset of slot 1 | 4, 5: the second clip starts at hop 8
    y1 = _feed(rt, [long_a, first_clip, long_b], pad, [5, 3])
    assert _frames(len(first_clip), pad) == 4 and 4 + look <= 8       # the first clip is out before the slot is reused
    assert _frames(len(long_b), pad) == 9
    with pytest.raises(RuntimeError, match="has ended"):
        rt.process(torch.zeros(3, HOP), valid_hops=[1, 1, 1])
    assert rt.frames.tolist() == [8, 8, 8]                            # (the refused call did not advance the handle)
    rt.reset([1])
    assert rt.frames.tolist() == [8, 0, 8]
    rest = [long_a[8 * HOP:], second_clip, long_b[8 * HOP:]]
    x = torch.zeros((3, 9 * HOP))
    for b, r in enumerate(rest):
        x[b, : len(r)] = torch.from_numpy(r)
    fr = {0: _frames(len(long_a), pad) - 8, 1: _frames(len(second_clip), pad), 2: _frames(len(long_b), pad) - 8}
    out, pos = [], 0
    for n in (4, 5):
        out.append(rt.process(x[:, pos * HOP:(pos + n) * HOP], valid_hops=[min(n, max(0, fr[b] - pos)) for b in range(3)]))
        pos += n
    y = torch.cat([y1] + out, dim=1).numpy()
    for b, clip, first in ((0, long_a, 0), (1, first_clip, 0), (1, second_clip, 8), (2, long_b, 0)):
        ref = O.enhance(p, sd, clip[None], pad=pad)[0]
        got = _window(y[b], len(clip), pad, look, first)
        err = rms(got - ref)
        print(f"  slot {b}, clip of {len(clip)} samples from hop {first}: rms error {err:.3e}")
        assert err < BOUND, (b, first, err)
    model.check()


def test_handles_that_refuse_ends(backend):
    """Gated, pausable, multi-channel and rate-converting handles refuse valid_hops and do not advance."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    model, df_state, _, _ = init_df(params=named_params("pf32_nopf"), epoch="none", seed=SEED)
    kinds = [dict(gating=True), dict(pausable=True), dict(channels=2)]
    if not emu_subset(backend):
        kinds.append(dict(sr=16000))
    for kw in kinds:
        rt = DfStream(model, df_state, streams=2, max_frames=2, **kw)
        x = torch.zeros(2, rt.frame_length)
        with pytest.raises(RuntimeError):
            rt.process(x, valid_hops=[1, 0])
        assert rt.frames.tolist() == [0] * (2 // rt.channels), kw
    rt = DfStream(model, df_state, streams=2, max_frames=2)
    with pytest.raises(RuntimeError):
        rt.process(torch.zeros(2, HOP), valid_hops=[2, 0])      # a count above n_frames
    with pytest.raises(ValueError):
        rt.process(torch.zeros(2, HOP), valid_hops=[1])         # one entry per stream
    with pytest.raises(TypeError):
        rt.process(torch.zeros(2, HOP), valid_hops=[1.0, 1.0])
    assert rt.frames.tolist() == [0, 0]


def _memory_bytes(model, df_state, streams, hops):
    from deepfilternet_amd import _lib

    n = C.c_int64()
    _lib.check(_lib.lib().dfx_stream_memory_bytes(model.handle, df_state.handle, streams, hops, C.byref(n)))
    return int(n.value)


def test_stream_memory_bytes_is_monotonic(backend):
    from deepfilternet_amd.enhance import init_df

    model, df_state, _, _ = init_df(params=named_params("pf32_nopf"), epoch="none", seed=SEED)
    sizes = [[_memory_bytes(model, df_state, s, h) for h in (1, 16, 17, 64, 256)] for s in (1, 3, 16, 17, 256)]
    for row in sizes:
        assert all(a < b for a, b in zip(row, row[1:])), sizes
    for a, b in zip(sizes, sizes[1:]):
        assert all(u < v for u, v in zip(a, b)), sizes
    with pytest.raises(RuntimeError):
        _memory_bytes(model, df_state, 0, 16)


@pytest.mark.gpu
def test_stream_memory_bytes_is_what_a_handle_takes(hip_backend):
    """The drop in free device memory across dfx_stream_create and the first 16-bit call (the staging rows) is at most the reported bytes plus
    the allocator's granularity: hipMalloc hands out whole 2 MiB pages here, and the handle makes three allocations (its buffer and the two
    staging rows), so 3 x 2 MiB."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    model, df_state, _, _ = init_df(params=named_params("df3"), epoch="none", seed=SEED)
    warm = DfStream(model, df_state, streams=1, max_frames=1)   # (whatever the first handle of a process makes the runtime allocate)
    warm.process(torch.zeros(1, HOP, dtype=torch.int16).cuda())
    for streams, hops in ((3, 7), (64, 33), (256, 128)):
        x = torch.zeros(streams, HOP, dtype=torch.int16).cuda()
        del_me = torch.empty_like(x)   # (the block process() takes for its output is in torch's pool before the measurement)
        del del_me
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info(_lib.device())
        rt = DfStream(model, df_state, streams=streams, max_frames=hops)
        rt.process(x)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info(_lib.device())
        said = _memory_bytes(model, df_state, streams, hops)
        print(f"  {streams} streams x {hops} hops: reported {said} bytes, free memory fell by {free0 - free1}")
        assert free0 - free1 <= said + 3 * (2 << 20), (streams, hops, free0 - free1, said)
        del rt
