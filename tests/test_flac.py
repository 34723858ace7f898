"""Native FLAC on the device: ``dfx_flac_probe`` / ``dfx_flac_decode`` and ``io.decode_flac`` / ``io.load_audio`` on top of them, against
tests/flac_ref.py — a reference decoder in Python integers (which has to reproduce the real-encoder fixture's STREAMINFO MD5 first) and an
encoder whose input is the expected output — and against the two real-encoder fixtures of tools/gen_golden_flac.py.  Everything is exact:
integers, and floats that are integers / 2^(bits - 1)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import flac_ref as R

MONO, STEREO = "flac_noise_mono.flac", "flac_noise_stereo24f.flac"
MONO_MD5 = "b9766d53a451a4b6a2b7283163e1bcff"


def _read(golden_dir, name):
    with open(os.path.join(golden_dir, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def mono_ref(golden_dir):
    """(bytes, info, pcm [1, T]) of the mono fixture by the reference decoder, decoded once"""
    data = _read(golden_dir, MONO)
    info, pcm = R.decode(data)
    pcm.setflags(write=False)
    return data, info, pcm


def native(pcm, bps):
    """what the decoder hands back for these samples: int16 filled from the top up to 16 bits, float32 = sample / 2^(bits - 1) above"""
    pcm = np.asarray(pcm, np.int64)
    return (pcm << (16 - bps)).astype(np.int16) if bps <= 16 else (pcm.astype(np.float32) / np.float32(1 << (bps - 1)))


def test_reference_decoder_reproduces_the_fixture_md5(mono_ref):
    data, info, pcm = mono_ref
    assert len(data) == 224035
    assert (info["sample_rate"], info["bps"], info["channels"], info["total"]) == (48000, 16, 1, 236983)
    assert info["md5"].hex() == MONO_MD5 and R.md5_of(pcm, 16).hex() == MONO_MD5
    at, sizes = info["first_frame"], []
    while at < len(data):
        fr = R.decode_frame(data, at, info)
        sizes.append(fr["bs"])
        at = fr["end"]
    assert sizes == [4096] * 57 + [3511]


def test_reference_decoder_inverts_the_encoder():
    for name, (blob, pcm, bps) in R.cases().items():
        info, got = R.decode(blob)
        assert np.array_equal(got, pcm), name
        assert info["bps"] == bps and info["md5"] == R.md5_of(pcm, bps), name


def test_probe(backend, golden_dir):
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    I = dio.flac_probe(_read(golden_dir, MONO))
    assert (I.sample_rate, I.channels, I.bits_per_sample, I.total_samples, I.min_block, I.max_block) == (48000, 1, 16, 236983, 4096, 4096)
    assert bytes(I.md5).hex() == MONO_MD5 and I.first_frame == R.probe(_read(golden_dir, MONO))["first_frame"]
    st = _read(golden_dir, STEREO)
    I = dio.flac_probe(st)
    assert (I.sample_rate, I.channels, I.bits_per_sample, I.total_samples) == (48000, 2, 16, 98304) and not any(I.md5)
    assert I.first_frame == R.probe(st)["first_frame"] == 162                      # the marker and the metadata blocks
    blob, _, _ = R.cases()["id3_and_padding"]
    assert blob[:3] == b"ID3"
    I = dio.flac_probe(blob)
    assert I.first_frame == R.probe(blob)["first_frame"] == 17 + 4 + 38 + 44 and I.total_samples == 192
    # the refusals
    L = _lib.lib()
    info = _lib.FlacInfo()

    def rc(b):
        a = np.frombuffer(b, np.uint8)
        return L.dfx_flac_probe(C.c_void_p(a.ctypes.data), len(b), C.byref(info))

    head = lambda **kw: R.stream_head(**{**dict(bps=16, channels=1, total=16, min_block=16, max_block=16), **kw})   # noqa: E731
    assert rc(head()) == _lib.DFX_OK
    assert rc(b"OggS" + bytes(60)) == _lib.DFX_ERR_INVALID_ARG and b"Ogg" in L.dfx_last_error()
    assert rc(b"RIFF" + bytes(60)) == _lib.DFX_ERR_INVALID_ARG
    assert rc(b"fLaC" + bytes([0x81, 0, 0, 4]) + bytes(4)) == _lib.DFX_ERR_INVALID_ARG and b"STREAMINFO" in L.dfx_last_error()
    assert rc(head(bps=32)) == _lib.DFX_ERR_INVALID_ARG and rc(head(bps=7)) == _lib.DFX_ERR_INVALID_ARG
    assert rc(head(bps=8)) == _lib.DFX_OK and rc(head(bps=24)) == _lib.DFX_OK and rc(head(channels=8)) == _lib.DFX_OK
    assert rc(head()[:30]) == _lib.DFX_ERR_INVALID_ARG            # cut inside STREAMINFO
    assert L.dfx_flac_probe(None, 0, C.byref(info)) == _lib.DFX_ERR_INVALID_ARG
    with pytest.raises(RuntimeError, match="Ogg"):
        dio.flac_probe(b"OggS" + bytes(60), "x.oga")


def test_case_table(backend):
    """Every path of the decoder, each case alone and all of them in one call: bit-exact against the encoder's input."""
    from deepfilternet_amd import io as dio

    cases = R.cases()
    want = {"const16", "verbatim192", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4", "lpc1", "lpc8", "lpc12", "lpc32", "blocks_fixed_strategy",
            "blocks_variable_strategy", "rice5", "escape", "escape_rice5", "long_unary", "left_side", "side_right", "mid_side", "ch3", "ch8",
            "wasted1", "wasted5", "wasted_stereo", "bps8", "bps12", "bps20", "bps24", "wide24", "side17", "adversarial_sync", "id3_and_padding"}
    assert set(cases) == want
    names = list(cases)
    got = dio.decode_flac([cases[k][0] for k in names], pcm16=True, names=names)
    for k, x in zip(names, got):
        _, pcm, bps = cases[k]
        ref = native(pcm, bps)
        assert x.dtype == (torch.int16 if bps <= 16 else torch.float32) and tuple(x.shape) == pcm.shape, k
        assert np.array_equal(x.cpu().numpy(), ref), k
    # alone (another place in the buffer, another grid), and as float32
    for k in ("adversarial_sync", "wide24", "side17", "mid_side", "ch3", "blocks_variable_strategy"):
        blob, pcm, bps = cases[k]
        (x,) = dio.decode_flac([blob], pcm16=False)
        assert x.dtype == torch.float32
        assert np.array_equal(x.cpu().numpy(), np.asarray(pcm, np.float32) / np.float32(1 << (bps - 1))), k


def test_adversarial_sync_is_a_candidate_and_not_a_frame(backend):
    """The look-alike header inside the verbatim payload passes every header check (that is the point of the case): the status still reports
    one frame, all samples."""
    from deepfilternet_amd import io as dio

    blob, pcm, _ = R.cases()["adversarial_sync"]
    info = R.probe(blob)
    fake = R.frame_header(192, 0, 8, 1, False)
    at = blob.index(fake)
    assert at > info["first_frame"] and R.crc8(blob[at:at + len(fake) - 1]) == blob[at + len(fake) - 1]
    st, _ = _raw_decode([blob])
    assert st.tolist() == [[1, 0, 192, 0]]
    (x,) = dio.decode_flac([blob], pcm16=True)
    assert np.array_equal(x.cpu().numpy(), native(pcm, 8))


def _raw_decode(blobs):
    """dfx_flac_decode itself (no exception on lost frames): (status rows, every stream's output bytes)"""
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    arrs = [np.frombuffer(b, np.uint8) for b in blobs]
    infos = [dio.flac_probe(a) for a in arrs]
    n = len(arrs)
    offs, at = [], 0
    for a in arrs:
        offs.append(at)
        at = (at + a.size + 15) // 16 * 16
    host = np.zeros(at, np.uint8)
    for a, o in zip(arrs, offs):
        host[o:o + a.size] = a
    dev = _lib.device()
    blob = torch.from_numpy(host).to(dev)
    oo, oat = [], 0
    for I in infos:
        oo.append(oat)
        oat = (oat + (2 if I.bits_per_sample <= 16 else 4) * I.channels * I.total_samples + 15) // 16 * 16
    out = torch.full((oat + 16,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    i64 = C.c_int64 * n
    lens, arr, need = i64(*[a.size for a in arrs]), (_lib.FlacInfo * n)(*infos), C.c_int64()
    L = _lib.lib()
    _lib.check(L.dfx_flac_workspace_bytes(n, lens, C.cast(arr, C.c_void_p), C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    _lib.check(L.dfx_flac_decode(_lib.ptr(blob), blob.numel(), n, i64(*offs), lens, C.cast(arr, C.c_void_p), i64(*oo), _lib.ptr(out), oat,
                                 _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream()))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert (out[oat:] == 0x5A).all()                      # nothing behind the bytes the call was given
    outs = [out[o:o + (2 if I.bits_per_sample <= 16 else 4) * I.channels * I.total_samples].cpu().numpy() for o, I in zip(oo, infos)]
    return status.cpu().numpy(), outs


def test_corrupt_streams_never_fault(backend, tmp_path):
    from deepfilternet_amd import io as dio

    blob, pcm, _ = R.cases()["blocks_fixed_strategy"]          # 4096 + 4096 + 37 samples
    first = R.probe(blob)["first_frame"]
    ends, at = [], first
    while at < len(blob):
        at = R.decode_frame(blob, at, R.probe(blob))["end"]
        ends.append(at)
    flip = bytearray(blob)
    flip[ends[0] + 2000] ^= 0x04                               # a payload bit of the second frame
    cut = blob[:ends[0] + 1500]                                # ends inside the second frame
    noise = blob[:first] + np.random.default_rng(7).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    st, outs = _raw_decode([bytes(flip), cut, noise, blob])
    assert st[0].tolist() == [2, 1, 4096 + 37, 0]
    assert st[1].tolist() == [1, 1, 4096, 0]
    assert st[2, 0] <= 1 and st[2, 1] >= 1 and st[2, 2] < 8229
    assert st[3].tolist() == [3, 0, 8229, 0]
    got = outs[0].view(np.int16).reshape(1, -1)
    assert np.array_equal(got[:, :4096], pcm[:, :4096]) and (got[:, 4096:8192] == 0).all() and np.array_equal(got[:, 8192:], pcm[:, 8192:])
    got = outs[1].view(np.int16).reshape(1, -1)
    assert np.array_equal(got[:, :4096], pcm[:, :4096]) and (got[:, 4096:] == 0).all()
    for name, b in (("flip", bytes(flip)), ("cut", cut), ("noise", noise)):
        path = tmp_path / f"{name}.flac"
        path.write_bytes(b)
        with pytest.raises(RuntimeError, match=rf"{name}\.flac: \d+ FLAC frame"):
            dio.load_audio(str(path))
    # reserved codes behind a valid header and CRC-8 make no frame: subframe type 2, LPC precision 1111, a negative LPC shift
    for sub_head in (bytes([2 << 1]), bytes([32 << 1, 0x00, 0x01, 0b11110000]), bytes([32 << 1, 0x00, 0x01, 0b00111000, 0x00])):
        hdr = R.frame_header(16, 0, 16, 0, False)
        body = hdr + sub_head + bytes(40)
        bad = R.stream_head(16, 1, 16, 16, 16) + body + R.crc16(body).to_bytes(2, "big")
        assert _raw_decode([bad])[0][0, :3].tolist() == [0, 1, 0]


def test_fixtures(backend, golden_dir, mono_ref):
    from deepfilternet_amd import io as dio

    data, info, pcm = mono_ref
    st = _read(golden_dir, STEREO)
    mono, stereo = dio.decode_flac([data, st], pcm16=True)
    assert mono.dtype == torch.int16 and tuple(mono.shape) == (1, 236983)
    assert dio.flac_md5(mono, 16).hex() == MONO_MD5
    assert np.array_equal(mono.cpu().numpy(), pcm)
    _, ref = R.decode(st)
    assert tuple(stereo.shape) == (2, 98304) and np.array_equal(stereo.cpu().numpy(), ref)


def test_load_audio(backend, golden_dir, mono_ref, tmp_path):
    """FLAC by its marker (not its name), the WAVE file's result, slices, resampling, the MD5 on request."""
    from deepfilternet_amd import io as dio

    _, _, pcm = mono_ref
    src = os.path.join(golden_dir, MONO)
    audio, meta = dio.load_audio(src)
    assert (meta.encoding, meta.bits_per_sample, meta.num_frames, meta.sample_rate, meta.num_channels) == ("FLAC", 16, 236983, 48000, 1)
    assert audio.dtype == torch.float32 and tuple(audio.shape) == (1, 236983)
    assert np.array_equal(audio.cpu().numpy(), pcm.astype(np.float32) / np.float32(32768))
    p16, _ = dio.load_audio(src, pcm16=True, verify_md5=True)
    assert p16.dtype == torch.int16 and np.array_equal(p16.cpu().numpy(), pcm)
    # the same samples from a WAVE file
    wav = str(tmp_path / "same.wav")
    dio.save_audio(wav, p16, 48000)
    w, wm = dio.load_audio(wav)
    assert torch.equal(w, audio) and wm.num_frames == meta.num_frames
    # a name that says nothing, and slices
    odd = tmp_path / "noise.bin"
    odd.write_bytes(_read(golden_dir, MONO))
    for off, n in ((0, 100), (4090, 10), (236000, 5000), (5, -1)):
        a, m = dio.load_audio(str(odd), frame_offset=off, num_frames=n)
        b, _ = dio.load_audio(wav, frame_offset=off, num_frames=n)
        assert m.num_frames == 236983 and torch.equal(a, b) and torch.equal(a, audio[:, off:off + n if n > 0 else None])
    # resampling as for the WAVE file (a short slice: the resampler is not what is tested)
    a, _ = dio.load_audio(src, sr=16000, verbose=False, num_frames=1600)
    b, _ = dio.load_audio(wav, sr=16000, verbose=False, num_frames=1600)
    assert tuple(a.shape) == (1, 1600) and torch.equal(a, b)
    # a wrong MD5 is found on request only
    bad = bytearray(_read(golden_dir, MONO))
    bad[8 + 18] ^= 1
    wrong = tmp_path / "wrong_md5.flac"
    wrong.write_bytes(bytes(bad))
    dio.load_audio(str(wrong))
    with pytest.raises(RuntimeError, match="MD5"):
        dio.load_audio(str(wrong), verify_md5=True)
    # 24 bits: float32 = sample / 2^23, as for a 24-bit WAVE; pcm16 changes nothing there
    blob, pcm24, _ = R.cases()["bps24"]
    f24 = tmp_path / "deep.flac"
    f24.write_bytes(blob)
    a, m = dio.load_audio(str(f24), pcm16=True)
    assert a.dtype == torch.float32 and m.bits_per_sample == 24 and np.array_equal(a.cpu().numpy(), native(pcm24, 24))


def test_argument_errors(backend):
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    L = _lib.lib()
    blob = R.cases()["const16"][0]
    a = np.frombuffer(blob, np.uint8)
    I = dio.flac_probe(a)
    dev = _lib.device()
    buf = torch.zeros(_pad16(a.size) + 16, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.copy())
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    status = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    one = C.c_int64 * 1
    need = C.c_int64()
    assert L.dfx_flac_workspace_bytes(1, one(a.size), C.byref(I), C.byref(need)) == _lib.DFX_OK
    ws = torch.zeros(need.value, dtype=torch.uint8, device=dev)

    def call(off=0, ln=a.size, oo=0, ob=64, wb=None, nbytes=None, blob_ptr=None):
        return L.dfx_flac_decode(blob_ptr or _lib.ptr(buf), buf.numel() if nbytes is None else nbytes, 1, one(off), one(ln), C.byref(I), one(oo),
                                 _lib.ptr(out), ob, _lib.ptr(status), _lib.ptr(ws), ws.numel() if wb is None else wb, _lib.stream())

    bad = _lib.DFX_ERR_INVALID_ARG
    assert call() == _lib.DFX_OK
    assert call(off=8) == bad                       # not a multiple of 16
    assert call(nbytes=a.size - 1) == bad           # the buffer ends before the stream does
    assert call(ob=16) == bad                       # 16 samples of int16 need 32 bytes
    assert call(oo=2) == bad
    assert call(wb=need.value - 1) == bad
    assert call(blob_ptr=C.c_void_p(buf.data_ptr() + 1)) == bad
    assert L.dfx_flac_decode(None, 0, 0, None, None, None, None, None, 0, None, None, 0, None) == _lib.DFX_OK   # nothing to do
    assert L.dfx_flac_decode(None, 0, 1, one(0), one(1), C.byref(I), one(0), _lib.ptr(out), 64, _lib.ptr(status), _lib.ptr(ws), ws.numel(), None) == bad
    assert call() == _lib.DFX_OK and status.cpu().numpy().tolist() == [[1, 0, 16, 0]]
    with pytest.raises(TypeError):
        dio.decode_flac([np.zeros(4, np.int16)])
    assert dio.decode_flac([]) == []


def _pad16(n):
    return (n + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------- GPU only
@pytest.mark.gpu
def test_ragged_batch_of_40_streams(hip_backend, golden_dir, mono_ref):
    """One call over 40 streams in shuffled order: a stream of one 16-sample frame beside the mono fixture."""
    from deepfilternet_amd import io as dio

    data, _, pcm = mono_ref
    cases = R.cases()
    pool = [(k, b, native(p, bps)) for k, (b, p, bps) in cases.items()] + [("mono", data, np.asarray(pcm, np.int16))] * 3
    _, ref = R.decode(_read(golden_dir, STEREO))
    pool += [("stereo", _read(golden_dir, STEREO), ref.astype(np.int16))] * 2
    rng = np.random.default_rng(40)
    pick = [pool[i] for i in rng.permutation(len(pool))[:38]] + [pool[0], ("mono", data, np.asarray(pcm, np.int16))]
    order = rng.permutation(40)
    pick = [pick[i] for i in order]
    assert len(pick) == 40 and {"const16", "mono"} <= {k for k, _, _ in pick}
    got = dio.decode_flac([b for _, b, _ in pick], pcm16=True, names=[k for k, _, _ in pick])
    for (k, _, want), x in zip(pick, got):
        assert np.array_equal(x.cpu().numpy(), want), k


@pytest.mark.gpu
def test_enhance_of_flac_equals_enhance_of_wav(hip_backend, golden_dir, tmp_path):
    from deepfilternet_amd import io as dio
    from deepfilternet_amd.enhance import enhance, enhance_files, init_df
    from tests.helpers import named_params

    p = named_params("df3")
    model, df_state, suffix, _ = init_df(params=p, epoch="none", seed=4)
    src = os.path.join(golden_dir, MONO)
    x, meta = dio.load_audio(src, sr=p.sr, pcm16=True)
    assert x.dtype == torch.int16 and meta.encoding == "FLAC"
    wav = str(tmp_path / "mono.wav")
    dio.save_audio(wav, x, p.sr)
    y, _ = dio.load_audio(wav, sr=p.sr, pcm16=True)
    assert torch.equal(x, y)
    a, b = enhance(model, df_state, x), enhance(model, df_state, y)
    assert a.dtype == torch.int16 and torch.equal(a, b) and int(a.abs().max()) > 100
    # enhance_files on a directory of the two fixtures: the WAVE files of the WAVE-input run, under .wav names
    fdir, wdir = tmp_path / "flac", tmp_path / "wav"
    fdir.mkdir(), wdir.mkdir()
    names = []
    for name in (MONO, STEREO):
        (fdir / name).write_bytes(_read(golden_dir, name))
        s, _ = dio.load_audio(str(fdir / name), pcm16=True)
        names.append(dio.save_audio(str(wdir / name.replace(".flac", ".wav")), s, p.sr))
    (tmp_path / "out_flac").mkdir(), (tmp_path / "out_wav").mkdir()
    got = enhance_files(model, df_state, sorted(str(f) for f in fdir.iterdir()), output_dir=str(tmp_path / "out_flac"), suffix=suffix)
    want = enhance_files(model, df_state, sorted(names), output_dir=str(tmp_path / "out_wav"), suffix=suffix)
    assert [os.path.basename(g) for g in got] == [os.path.basename(w) for w in want] and all(g.endswith(f"_{suffix}.wav") for g in got)
    for g, w in zip(got, want):
        with open(g, "rb") as fg, open(w, "rb") as fw:
            assert fg.read() == fw.read()
