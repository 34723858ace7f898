"""G.711 (mu-law / A-law) <-> float32 / int16: ``dfx_g711_decode`` / ``dfx_g711_encode`` and their ``deepfilternet_amd.io`` wrappers against
tests/golden/g711_tables.npz (tools/gen_golden_g711.py: Python's ``audioop`` for the decoders and for the encoders at s >= 0, G.711's
sign-magnitude rule for s < 0).  Everything here is exact: integers, and floats that are integers / 32768."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

LAWS = ("ulaw", "alaw")
SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}
TOP = {"ulaw": 32124, "alaw": 32256}


@pytest.fixture(scope="module")
def tables(golden_dir):
    with np.load(os.path.join(golden_dir, "g711_tables.npz")) as z:
        t = {k: z[k].copy() for k in z.files}
    for k in t:
        t[k].setflags(write=False)
    return t


def encode_ref(tables, law, s):
    """the golden encoder on int values in [-32768, 32767]"""
    return tables["enc_" + law][np.asarray(s, np.int64) + 32768]


def float_to_s16(x):
    """the float -> 16-bit rule of the contract: trunc(clamp(x * 32768, -32768, 32767)), NaN -> 0 (x float32; the product is exact or inf)"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(x, np.float32) * np.float32(32768.0)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(-32768.0), np.float32(32767.0)))
    return np.trunc(v).astype(np.int64)


def test_golden_tables(tables):
    """The committed tables are audioop's where that module exists; everywhere, they have the properties the contract states."""
    try:
        import audioop  # noqa: F401
        have = True
    except ImportError:
        have = False
    if have:
        from tools.gen_golden_g711 import tables as derive

        fresh = derive()
        assert sorted(fresh) == sorted(tables)
        for k in fresh:
            assert fresh[k].dtype == tables[k].dtype and np.array_equal(fresh[k], tables[k]), k
    for law in LAWS:
        dec, enc = tables["dec_" + law], tables["enc_" + law]
        assert dec.dtype == np.int16 and dec.shape == (256,) and enc.dtype == np.uint8 and enc.shape == (65536,)
        assert int(dec.max()) == TOP[law] and int(dec.min()) == -TOP[law]
        assert enc[32768] == SILENCE[law] and dec[SILENCE[law]] == (0 if law == "ulaw" else 8)   # (A-law has no zero: its smallest step)
        # sign symmetry: the codes of s and -s differ in the sign bit only, s = 1 .. 32767; -32768 clips like -32767
        s = np.arange(1, 32768)
        assert np.array_equal(enc[32768 + s] ^ 0x80, enc[32768 - s])
        assert enc[0] == enc[1]
        # idempotence: encode(decode(c)) == c, but for mu-law's negative zero
        back = enc[dec.astype(np.int64) + 32768]
        odd = np.flatnonzero(back != np.arange(256))
        assert odd.tolist() == ([0x7F] if law == "ulaw" else [])
        if law == "ulaw":
            assert back[0x7F] == 0xFF and dec[0x7F] == 0
        # monotone: a larger sample never decodes to a smaller value
        assert (np.diff(dec[enc].astype(np.int64)) >= 0).all()
        assert np.abs(dec[enc].astype(np.int64) - np.clip(np.arange(-32768, 32768), -TOP[law], TOP[law])).max() <= 1024


@pytest.mark.parametrize("law", LAWS)
def test_decode_all_codes(backend, tables, law):
    from deepfilternet_amd import io as dio

    codes = torch.arange(256, dtype=torch.uint8)
    f = dio.g711_to_float(codes, law)
    i = dio.g711_to_pcm16(codes, law)
    assert f.dtype == torch.float32 and i.dtype == torch.int16 and tuple(f.shape) == tuple(i.shape) == (256,)
    assert np.array_equal(i.cpu().numpy(), tables["dec_" + law])
    assert np.array_equal(f.cpu().numpy(), tables["dec_" + law].astype(np.float32) / np.float32(32768.0))
    assert tuple(dio.g711_to_float(codes.reshape(2, 4, 32), law).shape) == (2, 4, 32)


@pytest.mark.parametrize("law", LAWS)
def test_encode_all_int16(backend, tables, law):
    from deepfilternet_amd import io as dio

    s = np.arange(-32768, 32768).astype(np.int16)
    got = dio.pcm16_to_g711(torch.from_numpy(s), law)
    assert got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), tables["enc_" + law])


@pytest.mark.parametrize("law", LAWS)
def test_encode_floats_truncates_and_saturates(backend, tables, law):
    from deepfilternet_amd import io as dio

    s = np.arange(-32768, 32768)
    # (s + 0.5) / 32768: halfway between two 16-bit values (exact in float32) — truncation toward zero, not rounding, not flooring
    x = ((s + 0.5) / 32768.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 32768.0, s + 0.5)
    want = encode_ref(tables, law, np.where(s >= 0, s, s + 1))
    assert np.array_equal(float_to_s16(x), np.where(s >= 0, s, s + 1))
    assert np.array_equal(dio.float_to_g711(torch.from_numpy(x), law).cpu().numpy(), want)
    # saturation: out of range on either side, up to the infinities (float_to_pcm16 would wrap these)
    big = np.array([1.0, -1.0, 1.5, -1.5, 1e30, -1e30, np.inf, -np.inf, 32767.5 / 32768, -32768.5 / 32768, 3.0, -3.0], np.float32)
    v = big.astype(np.float64) * 32768.0
    assert (v > 32767).any() and (v < -32768).any() and np.isinf(big).any()
    sat = np.where(big > 0, 32767, -32768)
    assert np.array_equal(float_to_s16(big), sat)
    got = dio.float_to_g711(torch.from_numpy(big), law).cpu().numpy()
    assert np.array_equal(got, encode_ref(tables, law, sat))
    top_pos, top_neg = encode_ref(tables, law, 32767), encode_ref(tables, law, -32768)
    assert set(got[big > 0].tolist()) == {int(top_pos)} and set(got[big < 0].tolist()) == {int(top_neg)} and top_pos ^ 0x80 == top_neg
    # NaN is silence; so are both zeros
    quiet = dio.float_to_g711(torch.tensor([float("nan"), 0.0, -0.0, -float("nan")]), law).cpu().numpy()
    assert quiet.tolist() == [SILENCE[law]] * 4


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 65536 + 37])
def test_lengths_and_byte_offsets(backend, tables, law, n):
    """The byte side is read / written 16 codes at a time between a head and a tail of single codes: every length around one vector, and
    arrays that start 0, 1 and 3 bytes into their tensor."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    rng = np.random.default_rng(n + len(law))
    dev = _lib.device()
    for off in (0, 1, 3):
        codes = rng.integers(0, 256, n + off, dtype=np.uint8)
        buf = torch.from_numpy(codes).to(dev)
        view = buf[off:]
        assert n == 0 or view.data_ptr() == buf.data_ptr() + off
        dec = tables["dec_" + law][codes[off:]]
        assert np.array_equal(dio.g711_to_pcm16(view, law).cpu().numpy(), dec)
        assert np.array_equal(dio.g711_to_float(view, law).cpu().numpy(), dec.astype(np.float32) / np.float32(32768.0))
        # encode into a view at the same offset; the bytes in front of it and one guard byte behind it stay
        pcm = rng.integers(-32768, 32768, n).astype(np.int16)
        x = (rng.standard_normal(n) * 0.6).astype(np.float32)
        for src, want in ((torch.from_numpy(pcm), encode_ref(tables, law, pcm)), (torch.from_numpy(x), encode_ref(tables, law, float_to_s16(x)))):
            out = torch.full((off + n + 1,), 0x5A, dtype=torch.uint8, device=dev)
            fn = dio.pcm16_to_g711 if src.dtype == torch.int16 else dio.float_to_g711
            ret = fn(src, law, out=out[off:off + n])
            assert n == 0 or ret.data_ptr() == out.data_ptr() + off
            o = out.cpu().numpy()
            assert np.array_equal(o[off:off + n], want)
            assert (o[:off] == 0x5A).all() and o[off + n] == 0x5A


def test_errors(backend):
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio

    L = _lib.lib()
    dev = _lib.device()
    c = torch.zeros(32, dtype=torch.uint8, device=dev)
    f = torch.zeros(32, dtype=torch.float32, device=dev)
    bad = _lib.DFX_ERR_INVALID_ARG
    for law in (0, 3, -1):
        assert L.dfx_g711_decode(_lib.ptr(c), law, 32, _lib.ptr(f), 0, None) == bad
        assert L.dfx_g711_encode(_lib.ptr(f), 0, law, 32, _lib.ptr(c), None) == bad
    assert L.dfx_g711_decode(None, 1, 32, _lib.ptr(f), 0, None) == bad
    assert L.dfx_g711_decode(_lib.ptr(c), 1, 32, None, 0, None) == bad
    assert L.dfx_g711_encode(None, 0, 2, 32, _lib.ptr(c), None) == bad
    assert L.dfx_g711_encode(_lib.ptr(f), 0, 2, 32, None, None) == bad
    assert L.dfx_g711_decode(_lib.ptr(c), 1, -1, _lib.ptr(f), 0, None) == bad
    assert L.dfx_g711_encode(_lib.ptr(f), 0, 1, -1, _lib.ptr(c), None) == bad
    assert L.dfx_g711_decode(None, 1, 0, None, 0, None) == _lib.DFX_OK       # nothing to do
    assert L.dfx_g711_encode(None, 0, 2, 0, None, None) == _lib.DFX_OK
    assert L.dfx_stream_process_g711(None, None, 1, 1, None, None, None, None) == bad
    for fn in (dio.g711_to_float, dio.g711_to_pcm16):
        with pytest.raises(ValueError):
            fn(torch.zeros(4, dtype=torch.uint8), "mulaw")
        with pytest.raises(TypeError):
            fn(torch.zeros(4, dtype=torch.int16), "ulaw")
    with pytest.raises(ValueError):
        dio.float_to_g711(torch.zeros(4), None)
    with pytest.raises(TypeError):
        dio.pcm16_to_g711(torch.zeros(4), "alaw")
    with pytest.raises(ValueError):
        dio.float_to_g711(torch.zeros(4), "alaw", out=torch.zeros(3, dtype=torch.uint8, device=dev))
    assert L.dfx_g711_decode(_lib.ptr(c), 1, 32, _lib.ptr(f), 0, _lib.stream()) == _lib.DFX_OK   # the library still works
    assert C.c_int(L.dfx_g711_encode(_lib.ptr(f), 0, 1, 32, _lib.ptr(c), _lib.stream())).value == _lib.DFX_OK
