"""G.711 codes through the step resampler, through ``DfStream`` and through WAVE files.  Everything is held bit for bit to a composition of
parts that exist without G.711: the float path on the decoded codes (tests/golden/g711_tables.npz / 32768), then the encode rule of
include/dfx.h applied in numpy — s = trunc(clamp(x * 32768, -32768, 32767)), NaN -> 0, and the golden encoder table."""
import os
import struct
from functools import lru_cache

import numpy as np
import pytest
import torch

LAWS = ("ulaw", "alaw")
SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}
TOP_CODES = {"ulaw": (0x80, 0x00), "alaw": (0xAA, 0x2A)}    # the codes of the largest and the smallest value
F32, PCM16, ULAW, ALAW = 0, 1, 2, 3                          # DFX_FMT_*
FMT = {"ulaw": ULAW, "alaw": ALAW}
DTYPES = {F32: torch.float32, PCM16: torch.int16, ULAW: torch.uint8, ALAW: torch.uint8}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz")


@lru_cache(maxsize=1)
def _tables():
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


def decode(codes, law):
    """uint8 codes (tensor or array) -> float32 tensor"""
    c = codes.cpu().numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
    return torch.from_numpy(_tables()["dec_" + law][c].astype(np.float32) / np.float32(32768.0))


def encode(x, law):
    """float32 tensor -> uint8 codes by the stated rule"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = x.cpu().numpy().astype(np.float32) * np.float32(32768.0)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(-32768.0), np.float32(32767.0)))
    return torch.from_numpy(_tables()["enc_" + law][np.trunc(v).astype(np.int64) + 32768])


def to_pcm16(x):
    """dfx_f32_to_pcm16's rule (save_audio's cast): truncation toward zero, wrap-around"""
    v = np.trunc(x.cpu().numpy().astype(np.float32) * np.float32(32768.0)).astype(np.int64)
    return torch.from_numpy(v.astype(np.int16))


def convert(x, fmt):
    """a float32 tensor as format fmt"""
    return x if fmt == F32 else (to_pcm16(x) if fmt == PCM16 else encode(x, "ulaw" if fmt == ULAW else "alaw"))


def overshoots(y):
    """does the float signal leave [-32768, 32767] / 32768 on both sides (so that the saturation is exercised)?"""
    v = y.cpu().numpy().astype(np.float64) * 32768.0
    return bool((v > 32767.0).any() and (v < -32768.0).any())


def codes_with_top_runs(rng, law, rows, n, block):
    """random codes; row 0 alternates between the law's two top codes in runs, row 1 starts with a long run of the largest"""
    c = rng.integers(0, 256, (rows, n), dtype=np.uint8)
    hi, lo = TOP_CODES[law]
    run = max(8, 2 * block) if block < 100 else block
    for k in range(0, n, 2 * run):
        c[0, k:k + run] = hi
        c[0, k + run:k + 2 * run] = lo
    c[1, : min(n, 5 * run)] = lo
    c[1, min(n, 5 * run): min(n, 8 * run)] = hi
    return c


# ---- the step resampler ---------------------------------------------------------------------------------------------------------------------
def _rs_process(rs, x, xfmt, yfmt):
    """dfx_stream_resampler_process with a format of its own on either side (StreamResampler.process keeps the input's)"""
    from deepfilternet_amd import _lib

    x = x.to(_lib.device(), DTYPES[xfmt]).contiguous()
    T = x.shape[1]
    out_len = T // rs.block * rs._nw
    y = torch.empty((rs.rows, out_len), dtype=DTYPES[yfmt], device=x.device)
    _lib.check(_lib.lib().dfx_stream_resampler_process(rs._h, _lib.ptr(x), xfmt, T, T, _lib.ptr(y), yfmt, out_len, None, _lib.stream()))
    return y.cpu()


def _rs_run(rs, x, xfmt, yfmt, cut, block):
    out, pos = [], 0
    for c in cut:
        out.append(_rs_process(rs, x[:, pos * block:(pos + c) * block], xfmt, yfmt))
        pos += c
    return torch.cat(out, dim=1)


@pytest.mark.parametrize("orig_sr,new_sr,block,nw", [(8000, 48000, 1, 6), (48000, 8000, 6, 1), (44100, 48000, 147, 160)])
def test_resampler_every_format_pair(backend, orig_sr, new_sr, block, nw):
    from deepfilternet_amd import io as dio

    frames = {1: 150, 6: 150, 147: 4}[block]
    cut = [frames // 3, frames - frames // 3]
    new = lambda: dio.StreamResampler(orig_sr, new_sr, 3, max_samples=frames * block)   # noqa: E731
    rng = np.random.default_rng(orig_sr)
    for law in LAWS:
        codes = torch.from_numpy(codes_with_top_runs(rng, law, 3, frames * block, block))
        xf = decode(codes, law)
        yf = _rs_run(new(), xf, F32, F32, cut, block)             # the float handle on the decoded codes
        assert tuple(yf.shape) == (3, frames * nw)
        assert overshoots(yf), "the filter does not overshoot: no value that saturates"
        for yfmt in (F32, PCM16, ULAW, ALAW):
            y = _rs_run(new(), codes, FMT[law], yfmt, cut, block)
            assert y.dtype == DTYPES[yfmt] and torch.equal(y, convert(yf, yfmt)), (law, yfmt)
        y = _rs_run(new(), xf, F32, FMT[law], cut, block)         # float in, codes out
        assert torch.equal(y, encode(yf, law))
        # the Python wrapper: uint8 in, uint8 out, of the same law
        rs, pos, out = new(), 0, []
        for c in cut:
            out.append(rs.process(codes[:, pos * block:(pos + c) * block], law=law))
            pos += c
        assert out[0].dtype == torch.uint8 and torch.equal(torch.cat(out, dim=1).cpu(), encode(yf, law))
    with pytest.raises(ValueError):
        new().process(codes[:, : block])                          # uint8 needs a law
    with pytest.raises(ValueError):
        new().process(codes[:, : block], law="g711")


@pytest.mark.parametrize("law", LAWS)
def test_resampler_row_sits_out(backend, law):
    from deepfilternet_amd import io as dio

    orig_sr, new_sr, block, nw, per = 8000, 48000, 1, 6, 40
    rng = np.random.default_rng(5)
    codes = torch.from_numpy(rng.integers(0, 256, (3, 3 * per * block), dtype=np.uint8))
    piece = lambda k: codes[:, k * per * block:(k + 1) * per * block]   # noqa: E731
    rs = dio.StreamResampler(orig_sr, new_sr, 3, max_samples=per * block)
    y0 = rs.process(piece(0), law=law)
    y1 = rs.process(piece(1), active=[True, False, True], law=law)
    y2 = rs.process(piece(2), law=law)
    assert (y1[1] == SILENCE[law]).all() and (y1[0] != SILENCE[law]).any()
    # rows 0 and 2 ran all three calls, row 1 only the first and the last: a handle that never saw the middle one
    full = dio.StreamResampler(orig_sr, new_sr, 3, max_samples=per * block)
    f = [full.process(piece(k), law=law) for k in range(3)]
    for r in (0, 2):
        assert torch.equal(torch.cat([y0[r], y1[r], y2[r]]), torch.cat([f[0][r], f[1][r], f[2][r]]))
    two = dio.StreamResampler(orig_sr, new_sr, 3, max_samples=per * block)
    t0, t2 = two.process(piece(0), law=law), two.process(piece(2), law=law)
    assert torch.equal(y0[1], t0[1]) and torch.equal(y2[1], t2[1])
    assert not torch.equal(y2[1], f[2][1])


def test_resampler_refuses_unknown_formats(backend):
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    rs = dio.StreamResampler(8000, 48000, 1, max_samples=8)
    x, y = torch.zeros(1, 8, device=_lib.device()), torch.zeros(1, 48, device=_lib.device())
    L = _lib.lib()
    for xf, yf in ((4, 0), (0, 4), (-1, 0), (0, -1)):
        assert L.dfx_stream_resampler_process(rs._h, _lib.ptr(x), xf, 8, 8, _lib.ptr(y), yf, 48, None, _lib.stream()) == _lib.DFX_ERR_INVALID_ARG
    assert L.dfx_stream_resampler_process(rs._h, _lib.ptr(x), 0, 8, 8, _lib.ptr(y), 0, 48, None, _lib.stream()) == _lib.DFX_OK


# ---- DfStream -------------------------------------------------------------------------------------------------------------------------------
CUTS = [1, 3, 1, 2, 4, 1]
HOPS, STREAMS = 12, 3


@lru_cache(maxsize=2)
def _model(name):
    from deepfilternet_amd.enhance import init_df
    from tests.helpers import shape_params

    model, df_state, _, _ = init_df(params=shape_params(name), epoch="none", seed=9)
    return model, df_state


def _stream(name, sr, **kw):
    from deepfilternet_amd.streaming import DfStream

    model, df_state = _model(name)
    if sr is not None:
        kw["sr"] = sr
    return DfStream(model, df_state, streams=STREAMS, max_frames=max(CUTS), **kw)


def _codes(rt, law, seed, hops=HOPS):
    """a moderately loud signal as codes (every code value occurs), [streams, hops * frame_length]"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((0.1 * rng.standard_normal((STREAMS, hops * rt.frame_length))).astype(np.float32))
    c = encode(x, law)
    c[:, ::97] = torch.from_numpy(rng.integers(0, 256, c[:, ::97].shape, dtype=np.uint8))
    return c


def _cut(x, h, pos, n):
    return x[:, pos * h:(pos + n) * h]


@pytest.mark.gpu
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("sr", [8000, 16000, None])
@pytest.mark.parametrize("name", ["c32_e8_f16", "df3"])
def test_stream_codes_equal_the_float_twin(hip_backend, name, sr, law):
    rt, twin = _stream(name, sr, law=law), _stream(name, sr)
    h = rt.frame_length
    assert h == twin.frame_length == 480 * (sr or 48000) // 48000
    codes = _codes(rt, law, 31)
    xf = decode(codes, law)
    pos = 0
    for n in CUTS:
        y, lsnr = rt.process(_cut(codes, h, pos, n), return_lsnr=True)
        yt, lt = twin.process(_cut(xf, h, pos, n), return_lsnr=True)
        assert y.dtype == torch.uint8 and y.shape == (STREAMS, n * h)
        assert torch.equal(y.cpu(), encode(yt, law)), (pos, n)
        assert torch.equal(lsnr.cpu(), lt.cpu())
        pos += n
    assert pos == HOPS and (y != SILENCE[law]).any()
    with pytest.raises(ValueError):
        twin.process(_cut(codes, h, 0, 1))            # uint8 without a law, on a handle without one
    other = "alaw" if law == "ulaw" else "ulaw"        # the per-call override
    y = rt.process(_cut(codes, h, 0, 1), law=other)
    assert torch.equal(y.cpu(), encode(twin.process(decode(_cut(codes, h, 0, 1), other)), other))
    _model(name)[0].check()


@pytest.mark.gpu
@pytest.mark.parametrize("law", LAWS)
def test_stream_paused_streams_return_silence_codes(hip_backend, law):
    name, sr = "c32_e8_f16", 8000
    rt, twin = _stream(name, sr, law=law, pausable=True), _stream(name, sr, pausable=True)
    h = rt.frame_length
    codes = _codes(rt, law, 32)
    xf = decode(codes, law)
    pos = 0
    for k, n in enumerate(CUTS):
        mask = [True, k not in (2, 3), True]           # stream 1 sits two calls out
        y = rt.process(_cut(codes, h, pos, n), active=mask)
        yt = twin.process(_cut(xf, h, pos, n), active=mask)
        if not mask[1]:
            assert (y[1] == SILENCE[law]).all() and not yt[1].any()
        assert torch.equal(y.cpu(), encode(yt, law)), k
        pos += n
    assert (y[1] != SILENCE[law]).any()
    _model(name)[0].check()


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [8000, None])
def test_stream_pass_through_returns_the_callers_bytes(hip_backend, sr):
    name, law = "c32_e8_f16", "ulaw"
    rt, twin = _stream(name, sr, law=law), _stream(name, sr)
    h = rt.frame_length
    codes = _codes(rt, law, 33)
    codes[:, 5::11] = 0x7F                             # negative zero: a re-encoding would turn it into 0xFF
    xf = decode(codes, law)
    pos = 0
    for k, n in enumerate(CUTS):
        if k == 2:
            rt.set_atten_lim(0.0), twin.set_atten_lim(0.0)
        if k == 4:
            rt.set_atten_lim(100.0), twin.set_atten_lim(100.0)
        x = _cut(codes, h, pos, n)
        y = rt.process(x)
        yt = twin.process(_cut(xf, h, pos, n))
        if k in (2, 3):
            assert (x == 0x7F).any() and torch.equal(y.cpu(), x)
        else:
            assert torch.equal(y.cpu(), encode(yt, law)), k
        pos += n
    _model(name)[0].check()


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [8000, None])
def test_stream_formats_alternate_on_one_handle(hip_backend, sr):
    name, law = "c32_e8_f16", "ulaw"
    rt, twin = _stream(name, sr), _stream(name, sr)
    h = rt.frame_length
    codes = _codes(rt, law, 34)
    pos = 0
    for k, n in enumerate(CUTS):
        c = _cut(codes, h, pos, n)
        if k % 2 == 0:
            y, yt = rt.process(c, law=law), twin.process(decode(c, law))
            assert y.dtype == torch.uint8 and torch.equal(y.cpu(), encode(yt, law)), k
        else:
            pcm = _tables()["dec_" + law][c.numpy()]
            y, yt = rt.process(torch.from_numpy(pcm)), twin.process(torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0)))
            assert y.dtype == torch.int16 and torch.equal(y.cpu(), to_pcm16(yt)), k
        pos += n
    _model(name)[0].check()


@pytest.mark.gpu
def test_stream_moves_from_a_ulaw_fed_handle_into_a_pcm16_fed_one(hip_backend):
    """The sample format is no part of a stream's state: the streams of a handle fed mu-law continue in a handle fed 16-bit PCM, bit-equal to
    a float twin handle that never moved."""
    name, sr, law = "c32_e8_f16", 8000, "ulaw"
    src, dst, twin = _stream(name, sr, law=law), _stream(name, sr), _stream(name, sr)
    assert src.snapshot_bytes == dst.snapshot_bytes
    h = src.frame_length
    codes = _codes(src, law, 35)
    pcm = torch.from_numpy(_tables()["dec_" + law][codes.numpy()])
    xf = decode(codes, law)
    pos = 0
    for k, n in enumerate(CUTS):
        if k == 3:
            dst.import_streams(range(STREAMS), src.export_streams())
        yt = twin.process(_cut(xf, h, pos, n))
        if k < 3:
            assert torch.equal(src.process(_cut(codes, h, pos, n)).cpu(), encode(yt, law)), k
        else:
            assert torch.equal(dst.process(_cut(pcm, h, pos, n)).cpu(), to_pcm16(yt)), k
        pos += n
    _model(name)[0].check()


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
def _wave(path, codes, sr, law, extensible=False):
    """a G.711 WAVE file byte by byte: codes [T, C] uint8"""
    T, nch = codes.shape
    tag = 7 if law == "ulaw" else 6
    if extensible:
        guid = struct.pack("<H", tag) + bytes.fromhex("000000001000800000AA00389B71")
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, nch, sr, sr * nch, nch, 8, 22, 8, 0) + guid
    else:
        fmt = struct.pack("<HHIIHHH", tag, nch, sr, sr * nch, nch, 8, 0)
    payload = codes.tobytes()
    body = (b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<II", 4, T) + b"data" + struct.pack("<I", len(payload))
            + payload + (b"\x00" if len(payload) & 1 else b""))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


@pytest.mark.parametrize("law,nch,extensible", [("ulaw", 1, False), ("alaw", 1, False), ("ulaw", 2, False), ("alaw", 2, True)])
def test_load_g711_wave(backend, tmp_path, law, nch, extensible):
    from deepfilternet_amd import io as dio

    T, sr = 1235, 8000                                   # odd length: mono files carry a pad byte
    rng = np.random.default_rng(nch)
    codes = rng.integers(0, 256, (T, nch), dtype=np.uint8)
    path = str(tmp_path / "call.wav")
    _wave(path, codes, sr, law, extensible)
    audio, meta = dio.load_audio(path)
    want = decode(codes.T.copy(), law)
    assert audio.dtype == torch.float32 and torch.equal(audio.cpu(), want)
    assert (meta.sample_rate, meta.num_frames, meta.num_channels, meta.bits_per_sample, meta.encoding) == (sr, T, nch, 8, law.upper())
    raw, meta2, got_law = dio.load_audio(path, g711=True)
    assert raw.dtype == torch.uint8 and got_law == law and np.array_equal(raw.cpu().numpy(), codes.T) and meta2 == meta
    up, _ = dio.load_audio(path, sr=48000, verbose=False)
    assert torch.equal(up.cpu(), dio.resample(want, sr, 48000).cpu())
    res, _, no_law = dio.load_audio(path, sr=48000, verbose=False, g711=True)     # resampled: floats, no law
    assert no_law is None and torch.equal(res.cpu(), up.cpu())
    part, pm = dio.load_audio(path, frame_offset=100, num_frames=50)
    assert torch.equal(part.cpu(), want[:, 100:150]) and pm.num_frames == T
    # the tag in a 16-byte PCM header (no cbSize: not the chunk a non-PCM format carries) is refused, 16 bits per sample too
    for fmt in (struct.pack("<HHIIHH", 7 if law == "ulaw" else 6, nch, sr, sr * nch, nch, 8),
                struct.pack("<HHIIHHH", 7 if law == "ulaw" else 6, nch, sr, sr * nch * 2, nch * 2, 16, 0)):
        body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", 2 * nch) + bytes(2 * nch)
        bad = tmp_path / "bad.wav"
        bad.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
        with pytest.raises(RuntimeError, match="unsupported WAVE sample format"):
            dio.load_audio(str(bad))


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("kind", ["float", "int16", "codes"])
def test_save_g711_wave(backend, tmp_path, law, kind):
    from deepfilternet_amd import io as dio

    T, nch, sr = 259, 3, 8000
    rng = np.random.default_rng(3)
    x = torch.from_numpy((0.5 * rng.standard_normal((nch, T))).astype(np.float32))     # (some samples beyond +-1: they saturate)
    assert (x.abs() > 1).any()
    if kind == "float":
        audio, codes = x, encode(x, law)
    elif kind == "int16":
        audio = torch.from_numpy(rng.integers(-32768, 32768, (nch, T)).astype(np.int16))
        codes = torch.from_numpy(_tables()["enc_" + law][audio.numpy().astype(np.int64) + 32768])
    else:
        audio = codes = encode(x, law)
    path = dio.save_audio(str(tmp_path / "out.wav"), audio, sr, encoding=law.upper())
    raw = open(path, "rb").read()
    n = nch * T                                          # odd: a pad byte
    assert n & 1 and len(raw) == 12 + 8 + 18 + 8 + 4 + 8 + n + 1
    assert raw[:4] == b"RIFF" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8 and raw[8:12] == b"WAVE"
    assert raw[12:16] == b"fmt " and struct.unpack("<I", raw[16:20])[0] == 18
    tag, ch, rate, byte_rate, align, bits, cb = struct.unpack("<HHIIHHH", raw[20:38])
    assert (tag, ch, rate, byte_rate, align, bits, cb) == (7 if law == "ulaw" else 6, nch, sr, sr * nch, nch, 8, 0)
    assert raw[38:42] == b"fact" and struct.unpack("<II", raw[42:50]) == (4, T)
    assert raw[50:54] == b"data" and struct.unpack("<I", raw[54:58])[0] == n
    assert np.array_equal(np.frombuffer(raw[58:58 + n], np.uint8).reshape(T, nch).T, codes.numpy()) and raw[58 + n] == 0
    back, meta = dio.load_audio(path)
    assert torch.equal(back.cpu(), decode(codes, law)) and meta.encoding == law.upper() and meta.bits_per_sample == 8
    with pytest.raises(ValueError):
        dio.save_audio(str(tmp_path / "bad.wav"), audio, sr, encoding="G711")


def test_pcm16_and_float_files_are_written_and_read_as_before(backend, tmp_path):
    """The default arguments write the bytes they wrote: a 16-bit and a float file, built here byte by byte, come back from save_audio
    identically, and load as before."""
    from deepfilternet_amd import io as dio

    T, nch, sr = 301, 2, 16000
    rng = np.random.default_rng(4)
    pcm = rng.integers(-32768, 32768, (nch, T)).astype(np.int16)
    flt = (0.3 * rng.standard_normal((nch, T))).astype(np.float32)
    head16 = struct.pack("<HHIIHH", 1, nch, sr, sr * nch * 2, nch * 2, 16)
    pay16 = pcm.T.astype("<i2").tobytes()
    body16 = b"WAVE" + b"fmt " + struct.pack("<I", 16) + head16 + b"data" + struct.pack("<I", len(pay16)) + pay16
    head32 = struct.pack("<HHIIHHH", 3, nch, sr, sr * nch * 4, nch * 4, 32, 0)
    pay32 = flt.T.astype("<f4").tobytes()
    body32 = b"WAVE" + b"fmt " + struct.pack("<I", 18) + head32 + b"fact" + struct.pack("<II", 4, T) + b"data" + struct.pack("<I", len(pay32)) + pay32
    p16 = dio.save_audio(str(tmp_path / "a16.wav"), torch.from_numpy(pcm), sr)
    assert open(p16, "rb").read() == b"RIFF" + struct.pack("<I", len(body16)) + body16
    p32 = dio.save_audio(str(tmp_path / "a32.wav"), torch.from_numpy(flt), sr, dtype=torch.float32)
    assert open(p32, "rb").read() == b"RIFF" + struct.pack("<I", len(body32)) + body32
    pq = dio.save_audio(str(tmp_path / "q16.wav"), torch.from_numpy(flt), sr)      # float in, the wrapping 16-bit cast out
    assert open(pq, "rb").read()[44:] == to_pcm16(torch.from_numpy(flt)).numpy().T.astype("<i2").tobytes()
    a, m = dio.load_audio(p16)
    assert torch.equal(a.cpu(), torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0))) and (m.encoding, m.bits_per_sample) == ("PCM_S", 16)
    raw, _ = dio.load_audio(p16, pcm16=True)
    assert raw.dtype == torch.int16 and np.array_equal(raw.cpu().numpy(), pcm)
    b, m = dio.load_audio(p32)
    assert torch.equal(b.cpu(), torch.from_numpy(flt)) and (m.encoding, m.bits_per_sample) == ("PCM_F", 32)
    c, _, law = dio.load_audio(p16, g711=True)
    assert law is None and torch.equal(c.cpu(), a.cpu())
