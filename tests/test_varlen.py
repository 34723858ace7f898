"""Clips of different lengths in one batched pass (dfx_enhance_varlen[_pcm16], enhance_batch): every row gets exactly the samples that enhance()
gives that clip alone — bit for bit — and zeros behind its own output; enhance_files and the command line on top of it write the files of the
one-file-at-a-time loop, byte for byte."""
import ctypes as C
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from tests.helpers import emu_subset, named_params, rms, torch_sd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# nothing, one sample, less than a hop, a hop -1 / +0 / +1, two hops +0 / +1, a ragged eighth hop
EDGE_LENGTHS = [0, 1, 100, 479, 480, 481, 960, 961, 480 * 7 + 91]
LONGER = [480 * 40 + 17, 480 * 97 + 300, 48000 + 1]   # (on the GPU)
JUNK_F, JUNK_I = -7.0, -77


def _init(name, seed, **kw):
    from deepfilternet_amd.enhance import init_df

    p = named_params(name)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=seed, **kw)
    return p, model, df_state


def _clips(lengths, seed, channels=1, pcm16=False):
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        a = 0.1 * rng.standard_normal((channels, n))
        out.append(torch.from_numpy((a * 32768).clip(-32768, 32767).astype(np.int16) if pcm16 else a.astype(np.float32)))
    return out


def _ws(model, df_state, lens, pad):
    from deepfilternet_amd import _lib

    arr = (C.c_int64 * len(lens))(*lens)
    n = C.c_int64()
    _lib.check(_lib.lib().dfx_enhance_varlen_workspace_bytes(model.handle, df_state.handle, len(lens), arr, int(pad), C.byref(n)))
    return n.value


def _varlen(model, df_state, rows, pad=True, atten_lim_db=None, after_call=None):
    """dfx_enhance_varlen[_pcm16] on 1-D rows packed into [B, longest + 3] with junk behind every row, into a y pre-filled with junk.
    -> (y [B, y_stride] on the host, out_len per row, the pass's widest output)"""
    from deepfilternet_amd import _lib

    L = _lib.lib()
    dev = _lib.device()
    pcm16 = rows[0].dtype == torch.int16
    dt = torch.int16 if pcm16 else torch.float32
    lens = [int(r.shape[-1]) for r in rows]
    B, hop = len(rows), df_state.hop_size()
    outs = [n if pad else n // hop * hop for n in lens]
    x = torch.full((B, max(lens) + 3), 1234 if pcm16 else 0.75, dtype=dt)
    for b, r in enumerate(rows):
        x[b, : lens[b]] = r
    wide = max(outs)
    y = torch.full((B, wide + 5), JUNK_I if pcm16 else JUNK_F, dtype=dt)
    x, y = x.to(dev), y.to(dev)
    arr = (C.c_int64 * B)(*lens)
    nbytes = _ws(model, df_state, lens, pad)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fn = L.dfx_enhance_varlen_pcm16 if pcm16 else L.dfx_enhance_varlen
    _lib.check(fn(model.handle, df_state.handle, _lib.ptr(x), B, x.shape[1], arr, int(pad), float(atten_lim_db or 0.0), _lib.ptr(y), y.shape[1],
                  _lib.ptr(ws), nbytes, _lib.stream()))
    if after_call is not None:
        after_call(arr)
    model.check()
    return y.cpu(), outs, wide


def _check_rows(model, df_state, rows, y, outs, wide, **kw):
    from deepfilternet_amd.enhance import enhance

    junk = JUNK_I if y.dtype == torch.int16 else JUNK_F
    for b, r in enumerate(rows):
        alone = enhance(model, df_state, r.unsqueeze(0), **kw)[0].cpu()
        assert alone.shape == (outs[b],)
        assert torch.equal(y[b, : outs[b]], alone), (b, r.shape[-1])
        assert not y[b, outs[b]: wide].any(), (b, r.shape[-1])        # zeros up to the pass's widest output
        assert bool((y[b, wide:] == junk).all()), b                     # and nothing stored behind it


# case: (model on the interpreter, model on the GPU, init_df keywords, enhance keywords, 16-bit PCM)
CASES = {
    "pad": ("pf32_nopf", "df3", {}, {"pad": True}, False),
    "nopad": ("pf32_nopf", "df3", {}, {"pad": False}, False),
    "lim12": ("pf32_nopf", "df3", {}, {"pad": True, "atten_lim_db": 12.0}, False),
    "post_filter": ("pf32", "pf32", {}, {"pad": True}, False),
    "mask_only": ("pf32_nopf", "df3", {"mask_only": True}, {"pad": True}, False),
    "two_kernel_finish": ("df3_o10", "df3_o10", {}, {"pad": True}, False),   # df_order 10: dfx_synthesis_rows_ok is false
    "pcm16": ("pf32_nopf", "df3", {}, {"pad": True}, True),
    "pcm16_nopad": ("pf32_nopf", "df3", {}, {"pad": False}, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_varlen_rows_are_enhance_of_each_clip_alone(backend, case):
    from deepfilternet_amd.enhance import enhance_batch

    emu_name, gpu_name, init_kw, kw, pcm16 = CASES[case]
    if emu_subset(backend) and case in ("lim12", "two_kernel_finish", "pcm16_nopad"):
        pytest.skip("interpreter subset: this option runs on the GPU (DFX_EMU_ALL=1 runs it here)")
    _, model, df_state = _init(emu_name if backend == "emu" else gpu_name, 3, **init_kw)
    lengths = EDGE_LENGTHS + ([] if backend == "emu" else LONGER)
    rows = [c[0] for c in _clips(lengths, 1, pcm16=pcm16)]
    rows = rows[3:] + rows[:3]   # (any order: the C call does not want the rows sorted)
    y, outs, wide = _varlen(model, df_state, rows, **kw)
    _check_rows(model, df_state, rows, y, outs, wide, **kw)
    got = enhance_batch(model, df_state, rows, **kw)   # the Python layer: the same bits, 1-D clips give 1-D results
    assert len(got) == len(rows)
    for b, g in enumerate(got):
        assert g.shape == (outs[b],) and g.dtype == y.dtype and torch.equal(g.cpu(), y[b, : outs[b]]), b


def test_varlen_rows_match_the_oracle(backend):
    p, model, df_state = _init("pf32", 5)
    rows = [c[0] for c in _clips([480 * 5 + 33, 1500, 480 * 9 + 7], 9)]
    y, outs, _ = _varlen(model, df_state, rows)
    for b, r in enumerate(rows):
        ref = O.enhance(p, torch_sd(p, 5), r.numpy()[None])[0]
        assert rms(y[b, : outs[b]].numpy() - ref) < 2e-6, b


def test_zero_padding_changes_a_short_clip_varlen_does_not(backend):
    """Padding a short clip with zeros to the length of the others and slicing its output is not enhance() of the clip: the normalised features of
    the padded silence are not the reference's zero padding (pad_feat), and they reach the clip's last frames through the lookahead."""
    from deepfilternet_amd.enhance import enhance

    _, model, df_state = _init("pf32_nopf", 6)
    long_, short = _clips([480 * 34 + 11, 480 * 30 + 200], 4)
    n = short.shape[1]
    alone = enhance(model, df_state, short)[0]
    padded = torch.zeros((2, long_.shape[1]))
    padded[0], padded[1, :n] = long_[0], short[0]
    naive = enhance(model, df_state, padded)[1, :n]
    diff = torch.nonzero(naive != alone)
    assert diff.numel() > 0 and int(diff[0]) >= n - 4800          # the clip's last 100 ms differ, its head does not
    y, outs, _ = _varlen(model, df_state, [long_[0], short[0]])
    assert torch.equal(y[1, :n], alone) and torch.equal(y[0, : outs[0]], enhance(model, df_state, long_)[0])


def test_varlen_invalid_arguments(backend):
    from deepfilternet_amd import _lib

    L, dev = _lib.lib(), _lib.device()
    _, model, df_state = _init("pf32_nopf", 2)
    lens = (C.c_int64 * 3)(961, 480, 100)
    nbytes = _ws(model, df_state, list(lens), True)
    x = torch.zeros((3, 961), device=dev)
    y = torch.zeros((3, 961), device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    bad = (C.c_int64 * 3)(961, -1, 100)
    INVALID = _lib.DFX_ERR_INVALID_ARG

    def p(t):
        return _lib.ptr(t) if t is not None else None

    def call(x_=x, xs=961, lens_=lens, pad=1, y_=y, ys=961, ws_=ws, wsb=nbytes, B=3):
        return L.dfx_enhance_varlen(model.handle, df_state.handle, p(x_), B, xs, lens_, pad, 0.0, p(y_), ys, p(ws_), wsb, _lib.stream())

    n = C.c_int64()
    assert L.dfx_enhance_varlen_workspace_bytes(model.handle, df_state.handle, 3, bad, 1, C.byref(n)) == INVALID
    assert L.dfx_enhance_varlen_workspace_bytes(model.handle, df_state.handle, 3, None, 1, C.byref(n)) == INVALID
    assert call(lens_=bad) == INVALID                    # a negative length
    assert call(xs=960) == INVALID                       # x_stride below the longest clip
    assert call(ys=960) == INVALID                       # y_stride below its output (pad: 961)
    assert call(pad=0, ys=959) == INVALID                # (no pad: 960)
    assert call(wsb=nbytes - 1) == INVALID               # workspace too small
    for kw in ({"x_": None}, {"y_": None}, {"ws_": None}, {"lens_": None}):
        assert call(**kw) == INVALID, kw                 # null buffers with B > 0
    assert L.dfx_enhance_varlen_pcm16(model.handle, df_state.handle, p(x), 3, 961, bad, 1, 0.0, p(y), 961, p(ws), nbytes, _lib.stream()) == INVALID
    assert call(B=0, x_=None, y_=None, ws_=None, lens_=None) == 0
    assert call(pad=0, ys=960) == 0 and call() == 0
    model.check()


def test_varlen_lengths_array_is_free_when_the_call_returns(backend):
    """The caller may overwrite `lengths` as soon as the call returns, before the stream has caught up."""
    _, model, df_state = _init("pf32_nopf", 3)
    rows = [c[0] for c in _clips([480 * 9 + 5, 480 * 3 + 1, 700], 12)]
    y0, _, _ = _varlen(model, df_state, rows)

    def scribble(arr):
        for i in range(len(arr)):
            arr[i] = 5

    y1, _, _ = _varlen(model, df_state, rows, after_call=scribble)
    assert torch.equal(y0, y1)


def test_enhance_batch_passes_under_a_workspace_cap(backend, monkeypatch):
    """A workspace cap (DFX_WORKSPACE_CAP_GB) that holds two rows of the longest clip: several passes, the same samples."""
    from deepfilternet_amd import enhance as E

    _, model, df_state = _init("pf32_nopf", 2)
    clips = _clips([480 * 6 + 5, 480 * 2, 961, 77, 480 * 4 + 3], 8, channels=2)
    y0 = E.enhance_batch(model, df_state, clips)
    for c, y in zip(clips, y0):
        assert torch.equal(y, E.enhance(model, df_state, c))
    lens = sorted((c.shape[1] for c in clips for _ in range(2)), reverse=True)
    need = _ws(model, df_state, lens[:2], True)
    monkeypatch.setenv("DFX_WORKSPACE_CAP_GB", repr((need + 64) / (1 << 30)))
    assert len(E._plan_passes(model, df_state, lens, True)) >= 4
    model._ws = None
    y1 = E.enhance_batch(model, df_state, clips)
    assert model._ws.numel() <= need + 64
    for a, b in zip(y0, y1):
        assert torch.equal(a, b)
    monkeypatch.setenv("DFX_WORKSPACE_CAP_GB", "1e-9")
    with pytest.raises(MemoryError):
        E.enhance_batch(model, df_state, clips)


def test_enhance_batch_keeps_order_shapes_dtypes_devices(backend):
    from deepfilternet_amd.enhance import enhance, enhance_batch

    _, model, df_state = _init("pf32_nopf", 4)
    f = _clips([480 * 3 + 7, 480 * 5, 333], 2, channels=2)       # stereo float
    s = _clips([480 * 4 + 9, 10], 3, pcm16=True)                  # mono 16-bit PCM
    one_d = _clips([480 * 2 + 1], 4)[0][0]                        # a 1-D clip
    clips = [f[0], s[0], one_d, f[1], s[1], f[2], _clips([0], 5)[0]]
    variants = [clips]
    if backend == "hip":
        variants += [[c.pin_memory() for c in clips], [c.cuda() for c in clips], [c.cuda() if i % 2 else c.pin_memory() for i, c in enumerate(clips)]]
    assert enhance_batch(model, df_state, []) == []
    for pad in (True, False):
        for cs in variants:
            got = enhance_batch(model, df_state, cs, pad=pad)
            assert len(got) == len(cs)
            for c, g in zip(cs, got):
                want = enhance(model, df_state, c if c.dim() == 2 else c.unsqueeze(0), pad=pad)
                want = want if c.dim() == 2 else want[0]
                assert g.shape == want.shape and g.dtype == want.dtype and g.device == want.device
                if backend == "hip":
                    assert g.is_pinned() == want.is_pinned()
                assert torch.equal(g.cpu(), want.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["rows40", "rows70_batch_chunks", "time_chunks", "DFX_EXACT_FP32=1", "DFX_STREAMS=0", "DFX_GRU_SEQ=0",
                                     "DFX_GRU_PAIR=0"])
def test_varlen_across_groups_chunks_and_engine_paths(hip_backend, variant, monkeypatch):
    """40 rows cross the 16-clip groups and the pair form's 32; 70 rows are cut into pipelined batch chunks (from 64 clips), each with its slice
    of the row metadata; the layer-pipelined GRU phase; and the engine variants of test_enhance_engine_variants_agree: every row equals
    enhance() of its clip alone."""
    for k in ("DFX_GRU_SEQ", "DFX_EXACT_FP32", "DFX_GRU_PAIR", "DFX_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    if variant.startswith("DFX_"):
        k, v = variant.split("=")
        monkeypatch.setenv(k, v)
    _, model, df_state = _init("df3", 4)
    B = 70 if variant == "rows70_batch_chunks" else 40
    if variant == "rows70_batch_chunks":
        model.set_pipeline(batch_chunks=4)
    if variant == "time_chunks":
        model.set_pipeline(time_chunks=3, min_chunk_frames=2)
    lengths = np.random.default_rng(B).integers(1, 480 * 120, B).tolist()
    rows = [c[0] for c in _clips(lengths, 5)]
    y, outs, wide = _varlen(model, df_state, rows)
    if variant != "DFX_EXACT_FP32=1":
        _check_rows(model, df_state, rows, y, outs, wide)
    else:
        # the exact fp32 kernels' bits for a frame depend on the frame count of the pass (a batch of equal lengths gives every clip the bits of a
        # pass of its own; a row shorter than its pass does not): rows are held to that mode's bound against enhance() alone
        # (test_enhance_engine_variants_agree), their tails to zeros
        from deepfilternet_amd.enhance import enhance

        for b, r in enumerate(rows):
            alone = enhance(model, df_state, r.unsqueeze(0))[0].cpu()
            assert rms((y[b, : outs[b]] - alone).numpy()) < 1e-6 and not y[b, outs[b]: wide].any(), b
    model.check()


@pytest.mark.gpu
def test_varlen_full_size_mixed_lengths(hip_backend):
    """256 clips of 1-12 s in one pass (its GRU phase runs the frames of the longest): the longest, the shortest and two middle rows are
    enhance() of their clip alone; two rows against the oracle; no flag wait timed out."""
    from deepfilternet_amd.enhance import enhance, enhance_batch

    p, model, df_state = _init("df3", 7)
    lengths = np.random.default_rng(256).integers(48000, 12 * 48000 + 1, 256).tolist()
    clips = [c.cuda() for c in _clips(lengths, 11)]
    got = enhance_batch(model, df_state, clips)
    model.check()
    order = np.argsort(lengths)
    for i in (order[-1], order[0], order[100], order[180]):
        assert torch.equal(got[i], enhance(model, df_state, clips[i])), int(i)
    for i in (order[0], order[40]):
        ref = O.enhance(p, torch_sd(p, 7), clips[i].cpu().numpy())
        assert rms(got[i].cpu().numpy() - ref) < 2e-6, int(i)
    model.check()


def _write_wav(path, pcm, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1]), w.setsampwidth(2), w.setframerate(sr)
        w.writeframes(pcm.astype("<i2").tobytes())


def _noisy_files(tmp_path, specs, seed):
    rng = np.random.default_rng(seed)
    (tmp_path / "in").mkdir()
    files = []
    for name, sr, ch, n in specs:
        path = str(tmp_path / "in" / name)
        _write_wav(path, (0.2 * rng.standard_normal((n, ch)) * 32768).clip(-32768, 32767).astype("<i2"), sr)
        files.append(path)
    return files


def _per_file_loop(model, df_state, files, out_dir, suffix):
    """The loop enhance_files ran before it batched: one enhance() per file (df/enhance.py:73-89, 16-bit PCM at the model's rate)."""
    from deepfilternet_amd.enhance import enhance
    from deepfilternet_amd.io import load_audio, resample, save_audio

    sr, out = df_state.sr(), []
    for f in files:
        audio, meta = load_audio(f, sr=sr, verbose=False, pcm16=True)
        e = enhance(model, df_state, audio)
        if e.dtype != torch.int16:
            e = resample(e, sr, meta.sample_rate)
        out.append(save_audio(f, e, sr=meta.sample_rate, output_dir=out_dir, suffix=suffix))
    return out


def _same_bytes(got, want):
    assert [os.path.basename(g) for g in got] == [os.path.basename(w) for w in want]
    for g, w in zip(got, want):
        with open(g, "rb") as a, open(w, "rb") as b:
            assert a.read() == b.read(), g


def test_enhance_files_writes_the_per_file_bytes(backend, tmp_path):
    """Mono and stereo, 48 kHz 16-bit (the PCM16 path) and 16 kHz (resampled: the float path), different lengths, in one window."""
    from deepfilternet_amd.enhance import enhance_files

    _, model, df_state = _init("pf32_nopf", 5)
    k = 1 if backend == "emu" else 25
    files = _noisy_files(tmp_path, [("a.wav", 48000, 1, 480 * 3 * k + 17), ("b.wav", 16000, 2, 160 * 5 * k + 3), ("c.wav", 48000, 2, 480 * 5 * k),
                                    ("d.wav", 16000, 1, 160 * 2 * k + 1), ("e.wav", 48000, 1, 200)], 7)
    (tmp_path / "loop").mkdir()
    (tmp_path / "batch").mkdir()
    want = _per_file_loop(model, df_state, files, str(tmp_path / "loop"), "x")
    got = enhance_files(model, df_state, files, output_dir=str(tmp_path / "batch"), suffix="x")
    _same_bytes(got, want)


def test_cli_writes_what_enhance_files_writes(backend, tmp_path):
    """python -m deepfilternet_amd.enhance (df/enhance.py:299-379's deepFilter) with the reference's exported archive, and with a .dfx file."""
    from deepfilternet_amd import enhance as E
    from deepfilternet_amd.model import export_dfx, read_onnx_targz

    tar = os.path.join(REPO, "tests", "golden", "df3s_onnx.tar.gz")
    model, df_state, suffix, _ = E.init_df(tar)
    k = 1 if backend == "emu" else 20
    files = _noisy_files(tmp_path, [("one.wav", 48000, 1, 480 * 2 * k + 9), ("two.wav", 16000, 2, 160 * 3 * k + 1)], 3)
    (tmp_path / "api").mkdir()
    want = E.enhance_files(model, df_state, files, output_dir=str(tmp_path / "api"), suffix=suffix)
    p, sd = read_onnx_targz(tar)
    dfx = export_dfx(str(tmp_path / "m.dfx"), params=p, state_dict=sd)
    for m in (tar, dfx):
        cli = str(tmp_path / ("cli_" + os.path.basename(m)))
        args = ["-m", m, "-o", cli, "--no-suffix", *files]
        if backend == "emu":   # in this process: the interpreter build is the library it has loaded
            got = E.main(args)
        else:
            r = subprocess.run([sys.executable, "-m", "deepfilternet_amd.enhance", *args], cwd=REPO, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            got = [os.path.join(cli, os.path.basename(f)) for f in files]
        assert [os.path.basename(g) for g in got] == ["one.wav", "two.wav"]
        for g, w in zip(got, want):
            with open(g, "rb") as a, open(w, "rb") as b:
                assert a.read() == b.read(), (m, g)
    if backend == "emu":
        got = E.main(["-m", tar, "-o", str(tmp_path / "cli_dir"), "-i", str(tmp_path / "in")])
        _same_bytes(got, want)
