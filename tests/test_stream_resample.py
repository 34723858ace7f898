"""The resampler in step form (``deepfilternet_amd.io.StreamResampler`` / ``dfx_stream_resampler_*``) against oracle/io_oracle.py.

Contract: whatever the cut into calls, a row's concatenated output equals the whole-signal resampler applied to P zeros followed by the
row's signal, cut to whole frames (P = ceil(width / block) * block input samples); the outputs of different cuts are bit-identical."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import io_oracle as IO
from tests.helpers import rms

# rates, method, block:phases, P (input samples), D (output samples), history
PAIRS = [
    (16000, 48000, "sinc_fast", 1, 3, 17, 51, 34),
    (48000, 16000, "sinc_fast", 3, 1, 51, 17, 100),
    (44100, 48000, "sinc_fast", 147, 160, 147, 160, 164),
    (48000, 44100, "kaiser_best", 160, 147, 160, 147, 179),
    (8000, 48000, "sinc_fast", 1, 6, 17, 102, 34),
    (48000, 8000, "sinc_fast", 6, 1, 102, 17, 199),
    (32000, 48000, "kaiser_fast", 2, 3, 20, 30, 39),
    (48000, 32000, "sinc_best", 3, 2, 99, 66, 196),
]


def _cuts(frames, block, hist, hop_frames):
    """Three cuts of `frames` frames, in frames per call: single frames (shorter than the history), hop-sized, irregular with one call
    longer than the history."""
    single = [1] * frames
    hop = [hop_frames] * (frames // hop_frames) + ([frames % hop_frames] if frames % hop_frames else [])
    long = hist // block + 2
    assert long * block > hist and long + 6 <= frames
    irregular, left, k = [2, long, 1, 3], frames - long - 6, 0
    while left > 0:
        c = min(left, (5, 1, 7, 2)[k % 4])
        irregular.append(c)
        left -= c
        k += 1
    assert sum(single) == sum(hop) == sum(irregular) == frames
    return single, hop, irregular


def _run(rs, x, cut, block, active=None):
    out, pos = [], 0
    for c in cut:
        out.append(rs.process(x[:, pos * block:(pos + c) * block], active=active))
        pos += c
    return torch.cat(out, dim=1)


@pytest.mark.parametrize("orig_sr,new_sr,method,block,nw,P,D,hist", PAIRS)
def test_contract_any_cut_equals_the_offline_resampler_delayed(backend, orig_sr, new_sr, method, block, nw, P, D, hist):
    from deepfilternet_amd import io as dio

    emu = backend == "emu"
    hop_frames = max(1, (orig_sr // 100) // block)            # a 10 ms hop
    frames = max(12, -(-4 * hist // block), 2 * hop_frames)    # >= 12 frames, >= 4 x the history
    if emu:
        frames = max(12, -(-4 * hist // block))
        hop_frames = min(hop_frames, max(1, frames // 3))
    rng = np.random.default_rng(orig_sr + new_sr)
    x = (0.3 * rng.standard_normal((3, frames * block))).astype(np.float32)
    xt = torch.from_numpy(x)
    ref = IO.resample(np.concatenate([np.zeros((3, P), np.float32), x], axis=1), orig_sr, new_sr, method)[:, : frames * nw]
    outs = []
    for cut in _cuts(frames, block, hist, hop_frames):
        rs = dio.StreamResampler(orig_sr, new_sr, 3, method=method, max_samples=frames * block)
        assert rs.block == block and rs.delay == D and rs.delay_in == P
        y = _run(rs, xt, cut, block)
        assert tuple(y.shape) == (3, frames * nw)
        e = rms(y.cpu().numpy() - ref)
        print(f"{orig_sr}->{new_sr} {method}: {len(cut)} calls, rms err vs oracle {e:.3e}")
        assert e < 1e-6
        outs.append(y)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("orig_sr,new_sr,block,nw", [(16000, 48000, 1, 3), (48000, 44100, 160, 147)])
def test_rows_reset_and_sit_out_on_their_own(backend, orig_sr, new_sr, block, nw):
    from deepfilternet_amd import io as dio

    rows, per, calls = 5, {1: 40, 160: 2}[block], 8
    rng = np.random.default_rng(7)
    x = torch.from_numpy((0.3 * rng.standard_normal((rows, calls * per * block))).astype(np.float32))
    cut = [per] * calls
    plain = _run(dio.StreamResampler(orig_sr, new_sr, rows, max_samples=per * block), x, cut, block)
    # ---- row 1 starts over after three calls
    rs = dio.StreamResampler(orig_sr, new_sr, rows, max_samples=per * block)
    a = _run(rs, x[:, : 3 * per * block], cut[:3], block)
    rs.reset([1])
    b = _run(rs, x[:, 3 * per * block:], cut[3:], block)
    y = torch.cat([a, b], dim=1)
    others = [0, 2, 3, 4]
    assert torch.equal(y[others], plain[others])
    fresh = _run(dio.StreamResampler(orig_sr, new_sr, rows, max_samples=per * block), x[:, 3 * per * block:], cut[3:], block)
    assert torch.equal(b[1], fresh[1])
    assert not torch.equal(b[1], plain[1, 3 * per * nw:])
    rs.reset()   # every row
    assert torch.equal(_run(rs, x, cut, block), plain)
    # ---- masks: inactive rows return exact zeros and do not move
    rs = dio.StreamResampler(orig_sr, new_sr, rows, max_samples=per * block)
    masks = [torch.tensor([(r + c) % 3 != 0 for r in range(rows)]) for c in range(calls)]
    outs = [rs.process(x[:, c * per * block:(c + 1) * per * block], active=masks[c]) for c in range(calls)]
    for r in range(rows):
        on = [c for c in range(calls) if masks[c][r]]
        for c in range(calls):
            if c not in on:
                assert not outs[c][r].any()
        xin = torch.cat([x[r, c * per * block:(c + 1) * per * block] for c in on])[None].repeat(rows, 1)
        ref = _run(dio.StreamResampler(orig_sr, new_sr, rows, max_samples=per * block), xin, [per] * len(on), block)
        assert torch.equal(torch.cat([outs[c][r] for c in on]), ref[r])


@pytest.mark.parametrize("orig_sr,new_sr,block,nw", [(16000, 48000, 1, 3), (48000, 16000, 3, 1), (44100, 48000, 147, 160)])
def test_int16_in_and_out(backend, orig_sr, new_sr, block, nw):
    from deepfilternet_amd import io as dio

    frames = {1: 150, 3: 150, 147: 4}[block]
    rng = np.random.default_rng(11)
    pcm = np.clip(np.round(rng.standard_normal((3, frames * block)) * 9000.0), -32768, 32767).astype(np.int16)
    pcm[0, :: 5] = 32767     # full-scale runs: the filter overshoots +-1 (values that clip, i.e. wrap like save_audio's cast)
    pcm[0, 1:: 5] = -32768
    pcm[1, : 40 * block if block < 100 else block] = 32767
    xt = torch.from_numpy(pcm)
    cut = [frames // 3, frames - frames // 3]
    yf = _run(dio.StreamResampler(orig_sr, new_sr, 3, max_samples=frames * block), xt.to(torch.float32) / 32768, cut, block)
    yi = _run(dio.StreamResampler(orig_sr, new_sr, 3, max_samples=frames * block), xt, cut, block)
    assert yi.dtype == torch.int16 and tuple(yi.shape) == (3, frames * nw)
    want = dio.float_to_pcm16(yf).to(yi.device)
    assert torch.equal(yi, want)
    s = yf.cpu().numpy().astype(np.float64) * 32768.0
    assert (np.abs(s) > 32768.0).any(), "no value that clips"
    assert (s != np.trunc(s)).any(), "no value that truncates"
    # truncation toward zero where the value is in range
    ok = np.abs(s) < 32767.0
    assert np.array_equal(yi.cpu().numpy()[ok], np.trunc(s[ok]).astype(np.int16))


def test_errors(backend):
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    rs = dio.StreamResampler(44100, 48000, 2, max_samples=3 * 147)
    with pytest.raises(_lib.DfxError) as e:
        rs.process(torch.zeros(2, 146))
    assert e.value.code == _lib.DFX_ERR_INVALID_ARG
    with pytest.raises(_lib.DfxError) as e:
        rs.process(torch.zeros(2, 4 * 147))
    assert e.value.code == _lib.DFX_ERR_INVALID_ARG
    with pytest.raises(_lib.DfxError) as e:
        rs.reset([2])
    assert e.value.code == _lib.DFX_ERR_INVALID_ARG
    y = rs.process(torch.zeros(2, 3 * 147))      # the handle still works
    assert tuple(y.shape) == (2, 480) and not y.any()
    L = _lib.lib()
    a, b, h = C.c_int64(), C.c_int64(), C.c_void_p()
    assert L.dfx_stream_resampler_create(None, 2, 147, C.byref(h)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_stream_resampler_create(rs._r.h, 2, 100, C.byref(h)) == _lib.DFX_ERR_INVALID_ARG   # not a multiple of the block
    assert L.dfx_stream_resampler_delay(None, C.byref(a), C.byref(b)) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_stream_resampler_reset(None, None, 0, None) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_stream_resampler_process(None, None, 0, 0, 0, None, 0, 0, None, None) == _lib.DFX_ERR_INVALID_ARG
    L.dfx_stream_resampler_free(None)
    with pytest.raises(ValueError):
        dio.StreamResampler(48000, 48000, 1)
