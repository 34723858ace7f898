"""No pass depends on what its scratch memory held before.

Every network pass keeps its intermediates in a workspace the caller supplies (csrc/dfx_model.hip plan_ws, csrc/dfx_model_enhance.h plan_enh,
a stream handle's model_ws), and the Python package hands it ``torch.empty`` memory, as it does for every output.  The rest of the suite runs
the same shape several times in one process, so a pass there starts on the correct values of the computation under test, at the same offsets:
a consumer that reads a hand-over too early, a kernel that leaves a halo row or a ragged tail unwritten, or a chunk that reads past what its
producer has published would still give bit-equal, oracle-accurate output.

Here every case runs four times, each on a FRESH handle: once as the rest of the suite runs it, and once per pattern of
tests/scratch_fill.py FILLS with the workspace filled by the engine (``DFX_WS_FILL``, read by dfx_model_create) and every tensor the package
allocates filled by ``fresh_memory``.  Required of every case:
  * all outputs are bit-identical across the four runs;
  * ``model.check()`` reports nothing (no fp16-split range fault from a padding lane that loaded the pattern, no flag-wait timeout);
  * ``last_plan()`` is the same in the four runs: the same kernels ran;
  * under 0xFF the outputs meet the oracle at the tolerance of the existing test of that entry point (restated with its source line).

Shapes are the smallest at which each path can still go wrong (ragged batch and frame counts, more than one 16-clip group, one frame);
the workspace-free kernels run at the ragged shapes of their own tests with filled outputs only: equal across fills = every element written."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepfilternet_amd.state_dict import random_state_dict
from oracle import dfnet_oracle as O
from oracle import libdf_oracle as L
from tests.helpers import NAMED, emu_subset, named_params, rms, shape_params, torch_sd, widths_for
from tests.scratch_fill import FILLS, assert_same_bits, bits, fresh_memory, set_fill

HOP = 480
RUNS = (None,) + FILLS   # None: the switch unset and torch.empty as it is
GRU_SWITCHES = ("DFX_GRU_SEQ", "DFX_EXACT_FP32", "DFX_GRU_PAIR", "DFX_GRU_PAIR_FAR", "DFX_STREAMS")


def _noise(shape, seed, scale=0.1):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32))


def _cpu(out):
    return tuple(o.cpu() for o in out) if isinstance(out, (tuple, list)) else (out.cpu(),)


def _sweep(monkeypatch, run, what, same_plan=True):
    """run(fill) -> (outputs, model) on a handle created inside it.  The four runs give the same bits, no fault and the same plan.
    -> {fill: outputs}"""
    outs, plans = {}, {}
    for fill in RUNS:
        set_fill(monkeypatch, fill)
        out, model = run(fill)
        model.check()
        outs[fill], plans[fill] = _cpu(out), model.last_plan()
    set_fill(monkeypatch, None)
    assert_same_bits(outs, what)
    if same_plan:
        for fill in FILLS:
            assert plans[fill] == plans[None], (what, fill, plans[fill], plans[None])
    return outs


# ------------------------------------------------------------------------------------------------------------------ the switch itself
def test_the_switch_fills_the_layout_and_nothing_else(backend, monkeypatch):
    """DFX_WS_FILL=75 on a zeroed workspace that is larger than the pass needs: the last byte of the `need` bytes — alignment slack no kernel
    writes — holds the pattern after dfx_model_forward and after dfx_enhance, the bytes behind `need` are untouched, and without the switch that
    byte stays zero: the other cases of this file do run on filled memory, and the fill stays inside what the pass was given."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import enhance, init_df

    p = named_params("pf32")
    B, T = 2, 3
    spec, fe, fs = _noise((B, 1, T, p.freq_bins, 2), 1), _noise((B, 1, T, p.nb_erb), 2), _noise((B, 1, T, p.nb_df, 2), 3)
    x = _noise((B, HOP * T), 4)
    for fill in (0x4B, None):
        set_fill(monkeypatch, fill)
        model, df_state, _, _ = init_df(params=named_params("pf32"), epoch="none", seed=1)
        n = C.c_int64()
        for entry in ("forward", "enhance"):
            if entry == "forward":
                _lib.check(_lib.lib().dfx_model_workspace_bytes(model.handle, B, T, C.byref(n)))
            else:
                _lib.check(_lib.lib().dfx_enhance_workspace_bytes(model.handle, df_state.handle, B, x.shape[1], 0, C.byref(n)))
            need = int(n.value)
            model._ws = torch.zeros(need + 512, dtype=torch.uint8, device=_lib.device())
            if entry == "forward":
                model(spec, fe, fs)
            else:
                enhance(model, df_state, x, pad=False)
            model.check()
            ws = model._ws.cpu()
            assert ws.numel() == need + 512                       # (the pass ran in the workspace it was handed)
            assert int(ws[need - 1]) == (fill or 0), (entry, fill)
            assert not bool(ws[need:].any()), (entry, fill)
    set_fill(monkeypatch, None)


# ------------------------------------------------------------------------------------------------------------------ DfNet.forward
# the SHAPES entries that flip a plan decision away from df3 (tests/helpers.py), and which of them the interpreter keeps
FORWARD_SHAPES = ("kt7", "lg8", "lg4_elg16", "c16_e16_f32_o6", "e64", "l5_d3", "o1", "fft512", "c32_e8_f16")
FORWARD_CASES = [(n, B, T) for n in NAMED for B, T in ((3, 21), (17, 5))] + [(n, 3, 9) for n in FORWARD_SHAPES]
EMU_FORWARD = {("pf32", 3, 21), ("df3", 17, 5), ("kt7", 3, 9), ("c32_e8_f16", 3, 9), ("lg4_elg16", 3, 9)}


def _rel(a, b):
    """tests/test_dfnet_kernels.py _cmp: the largest error relative to max(1, largest reference value)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("shape,B,T", FORWARD_CASES, ids=[f"{n}-{B}x{T}" for n, B, T in FORWARD_CASES])
def test_forward_ignores_scratch_contents(backend, monkeypatch, shape, B, T):
    from deepfilternet_amd.model import DfNet

    if emu_subset(backend) and (shape, B, T) not in EMU_FORWARD:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it); every case runs on the GPU")
    p = shape_params(shape)
    sd = random_state_dict(p, 11, widths=widths_for(p))
    rng = np.random.default_rng(B + T)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy(rng.standard_normal((B, 1, T, p.nb_df, 2)).astype(np.float32))

    def run(fill):
        model = DfNet(p, sd)
        with fresh_memory(fill):
            return model(spec, fe, fs), model

    outs = _sweep(monkeypatch, run, f"forward {shape} {B}x{T}")
    spec_e, m, lsnr, coefs = outs[0xFF]
    ref = O.dfnet_forward(p, {k: torch.as_tensor(v) for k, v in sd.items()}, widths_for(p), spec, fe, fs)
    # tolerances: tests/test_dfnet_kernels.py:68-71 == tests/test_model_shapes.py:78-81
    errs = {"mask": (_rel(m, ref["m"]), 3e-5), "lsnr": (_rel(lsnr, ref["lsnr"]), 3e-5), "df_coefs": (_rel(coefs, ref["df_coefs"]), 5e-5),
            "spec_e": (_rel(spec_e, ref["spec_e"]), 5e-5)}
    print(f"  forward {shape} {B}x{T} [{backend}] under 0xFF, error / max(1, |ref|max): " + ", ".join(f"{k} {e:.3e}" for k, (e, _) in errs.items()))
    for k, (e, tol) in errs.items():
        assert e <= tol, (k, e)


# ------------------------------------------------------------------------------------------------------------------ enhance()
def _enh_model(backend):
    return "pf32" if backend == "emu" else "df3"   # (the interpreter is slow: the conv_ch=32 model there, as in tests/test_streaming.py)


@pytest.mark.parametrize("pad", [True, False], ids=["pad", "nopad"])
@pytest.mark.parametrize("form", ["serial", "chunked", "one_frame"])
def test_enhance_ignores_scratch_contents(backend, monkeypatch, form, pad):
    """3 clips x 21 frames with the GRU phase as one chunk and cut into time chunks (h carried between chunks: on the GPU the persistent phase
    with its followers, on the interpreter one launch per layer and chunk), and a clip of one hop: ONE frame without the padding, three with it."""
    from deepfilternet_amd.enhance import enhance, init_df

    if emu_subset(backend) and form == "chunked" and not pad:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it): the chunked form runs padded there, both on the GPU")
    # (one frame: the oracle's pad_feat, like the reference's, needs more frames than the lookahead — pf32 looks one frame ahead, df3 two)
    name = "pf32" if form == "one_frame" else _enh_model(backend)
    p = named_params(name)
    x = _noise((2, HOP), 6) if form == "one_frame" else _noise((3, HOP * (19 if pad else 21) + 7), 5)   # (the padding adds fft_size / hop = 2 frames)
    frames = (x.shape[1] + (p.fft_size if pad else 0)) // HOP
    assert frames == (21 if form != "one_frame" else (3 if pad else 1))

    def run(fill):
        model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=4)
        if form == "chunked":
            model.set_pipeline(time_chunks=3, min_chunk_frames=2)
        with fresh_memory(fill):
            y = enhance(model, df_state, x, pad=pad)
        assert model.last_plan()["pipe"] == (form == "chunked"), model.last_plan()
        return y, model

    y = _sweep(monkeypatch, run, f"enhance {form} pad={pad}")[0xFF][0]
    err = rms(y.numpy() - O.enhance(p, torch_sd(p, 4), x.numpy(), pad=pad))
    print(f"  enhance {name} {form} pad={pad} [{backend}] under 0xFF: rms error {err:.3e}")
    assert err < 2e-6, err   # tests/test_enhance.py:95


def test_sub_batches_in_a_capped_workspace_ignore_its_contents(backend, monkeypatch):
    """5 clips in a workspace with room for two (tests/test_enhance.py test_enhance_sub_batches_when_the_workspace_is_capped): 2 + 2 + 1, the last
    sub-batch runs in a workspace whose tail still holds the second clip of the one before it (or, here, the pattern)."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import enhance, init_df

    p = named_params("defaults")
    x = _noise((5, HOP * 5 + 17), 8)

    def run(fill):
        model, df_state, _, _ = init_df(params=named_params("defaults"), epoch="none", seed=2)
        n = C.c_int64()
        _lib.check(_lib.lib().dfx_enhance_workspace_bytes(model.handle, df_state.handle, 2, x.shape[1], 1, C.byref(n)))
        monkeypatch.setenv("DFX_WORKSPACE_CAP_GB", repr((n.value + 64) / (1 << 30)))
        with fresh_memory(fill):
            y = enhance(model, df_state, x)
        monkeypatch.delenv("DFX_WORKSPACE_CAP_GB")
        assert model._ws.numel() <= n.value + 64    # three passes in one small workspace
        return y, model

    y = _sweep(monkeypatch, run, "capped enhance")[0xFF][0]
    err = rms(y.numpy() - O.enhance(p, torch_sd(p, 2), x.numpy()))
    print(f"  enhance defaults 2+2+1 [{backend}] under 0xFF: rms error {err:.3e}")
    assert err < 2e-6, err   # tests/test_enhance.py:50


# ------------------------------------------------------------------------------------------------------------------ varlen
VARLEN_LENGTHS = [HOP * 17 + 91, HOP * 7, HOP * 5 + 1, 100]   # 17, 7, 5 and 0 whole hops: the last clip is shorter than a hop


@pytest.mark.parametrize("pad", [True, False], ids=["pad", "nopad"])
def test_varlen_ignores_scratch_contents(backend, monkeypatch, pad):
    """dfx_enhance_varlen: the row metadata in front of the workspace, the zeroed tails of spectrum and features, the zeros behind a shorter
    row's output (include/dfx.h, dfx_enhance_varlen: row b = dfx_enhance of clip b alone, then zeros up to the widest output, nothing behind)
    — and enhance_batch on top, whose packing buffer holds the pattern behind every row's own samples."""
    from deepfilternet_amd.enhance import enhance_batch, init_df
    from tests.test_varlen import _check_rows, _clips, _varlen

    name = "pf32" if backend == "emu" else "df3"
    p = named_params(name)
    rows = [c[0] for c in _clips(VARLEN_LENGTHS, 1)]
    rows = rows[1:] + rows[:1]   # (the longest row is not the first)

    def run(fill):
        model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=3)
        with fresh_memory(fill):
            y, outs, wide = _varlen(model, df_state, rows, pad=pad)          # (its workspace is a torch.empty of its own)
            # tests/test_varlen.py: every row is enhance() of the clip alone, bit for bit, then zeros, then nothing stored.  (The interpreter
            # runs the four passes of single clips once: the other runs have to equal this one anyway.)
            if fill is None or backend == "hip":
                _check_rows(model, df_state, rows, y, outs, wide, pad=pad)
            got = enhance_batch(model, df_state, rows, pad=pad)
        for b, g in enumerate(got):
            assert g.shape == (outs[b],) and torch.equal(g.cpu(), y[b, : outs[b]]), b
        return (y,) + tuple(got), model

    y = _sweep(monkeypatch, run, f"varlen pad={pad}", same_plan=False)[0xFF][0]   # (the last pass of a run is enhance_batch's)
    hop = p.hop_size
    sd = torch_sd(p, 3)
    worst = 0.0
    for b, r in enumerate(rows):
        n = r.shape[0] if pad else r.shape[0] // hop * hop
        if n:
            worst = max(worst, rms(y[b, :n].numpy() - O.enhance(p, sd, r.numpy()[None], pad=pad)[0]))
    print(f"  varlen {name} pad={pad} [{backend}] under 0xFF: largest row rms error {worst:.3e}")
    assert worst < 2e-6, worst   # tests/test_varlen.py:130


# ------------------------------------------------------------------------------------------------------------------ GRU phase forms (GPU)
# form -> (environment, plan["pipe"], plan["use_seq"] == the persistent phase ran, its recurrences ran on pairs of CUs)
GRU_FORMS = {
    "pair": ({}, True, True, True),
    "pair0": ({"DFX_GRU_PAIR": "0"}, True, True, False),
    "pair_far": ({"DFX_GRU_PAIR_FAR": "1"}, True, True, True),
    "seq0": ({"DFX_GRU_SEQ": "0"}, True, False, False),
    "exact": ({"DFX_EXACT_FP32": "1"}, True, True, False),
    "streams0": ({"DFX_STREAMS": "0"}, False, False, False),   # no internal streams: the serial GRU phase
}
GRU_SIZES = [(17, 5), (20, 17), (48, 40)]   # tests/test_gru_pair_step.py: a second tile with one live clip / partly live / an empty last half; frames below, at and above the followers' blocks


def _gru_env(monkeypatch, env):
    for k in GRU_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _gru_run(monkeypatch, form, xs, fill):
    """A fresh df3 handle in the given form; enhance() of every input in xs, one after the other, in one workspace.  The assertions on which
    form ran are those of tests/test_gru_pair_step.py _run."""
    from deepfilternet_amd.enhance import enhance, init_df

    env, pipe, persistent, pair = GRU_FORMS[form]
    _gru_env(monkeypatch, env)
    model, df_state, _, _ = init_df(params=named_params("df3"), epoch="none", seed=4)
    model.set_pipeline(time_chunks=12, min_chunk_frames=2)
    before, before_pair = model.query(model.Q_PASSES_PERSISTENT), model.query(model.Q_PASSES_PAIR)
    with fresh_memory(fill):
        ys = [enhance(model, df_state, x, pad=False).cpu() for x in xs]
    model.check()
    plan = model.last_plan()
    assert plan["pipe"] == pipe and plan["use_seq"] == persistent, plan
    assert model.query(model.Q_GRU_PERSISTENT) == int(form not in ("seq0", "streams0"))   # (a handle without internal streams has no multi-stream passes)
    assert model.query(model.Q_PASSES_PERSISTENT) - before == (len(xs) if persistent else 0)
    assert model.query(model.Q_PASSES_PAIR) - before_pair == (len(xs) if pair else 0)
    _gru_env(monkeypatch, {})
    return ys, model


_GRU_REFS = {}


def _gru_ref(x, key):
    """O.enhance(pad=False) of a df3 input, computed once per input and shared by the forms (left unchanged)."""
    if key not in _GRU_REFS:
        p = named_params("df3")
        _GRU_REFS[key] = O.enhance(p, torch_sd(p, 4), x.cpu().numpy(), pad=False)
    return _GRU_REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("clips,frames", GRU_SIZES, ids=[f"{c}x{f}" for c, f in GRU_SIZES])
@pytest.mark.parametrize("form", list(GRU_FORMS))
def test_gru_phase_forms_ignore_scratch_contents(hip_backend, monkeypatch, form, clips, frames):
    """df3, clips x frames, every form of the GRU phase.  In the persistent forms the follower workgroups run at all three sizes.  That is
    DERIVED, not observed (no counter or plan bit reports followers): their condition in dfx_model_forward.h gru_persistent is the fan-out
    kernel (plan["fan"]) and (layers + followers + 1) * groups <= 3/4 of the CUs — 10 * groups <= 192 on the 256 CUs of an MI355X — which
    holds for the 2 and 3 groups of 16 clips here; the two premises are asserted below.  So 5, 17 and 40 frames are less than a block of the
    emb follower (8 steps), a block of the projection followers (16) plus one step, and two blocks plus a partial one."""
    x = _noise((clips, frames * HOP), 100 * clips + frames).cuda()

    def run(fill):
        ys, model = _gru_run(monkeypatch, form, [x], fill)
        groups = -(-clips // 16)
        assert model.last_plan()["fan"] and groups in (2, 3) and 10 * groups <= torch.cuda.get_device_properties(0).multi_processor_count * 3 // 4
        return ys[0], model

    outs = _sweep(monkeypatch, run, f"{form} {clips}x{frames}")
    y = outs[0xFF][0]
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    err = rms(y.numpy() - _gru_ref(x, (clips, frames)))
    print(f"  {form} {clips}x{frames} under 0xFF: rms error {err:.3e}")
    assert err < 2e-6, err   # tests/test_enhance.py:127


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(GRU_FORMS))
def test_second_input_on_a_handle_equals_a_fresh_handle(hip_backend, monkeypatch, form):
    """Two different inputs back to back on one handle: the second pass starts on the first one's intermediates — plausible values of another
    signal at the same offsets — and gives what a fresh handle gives, which is the oracle's answer to the second input."""
    a, b = _noise((20, 17 * HOP), 31).cuda(), _noise((20, 17 * HOP), 32).cuda()
    for fill in (None, 0x4B):
        set_fill(monkeypatch, fill)
        (ya, yb), _ = _gru_run(monkeypatch, form, [a, b], fill)
        (yb_fresh,), _ = _gru_run(monkeypatch, form, [b], fill)
        assert not torch.equal(ya, yb)
        assert_same_bits({"fresh handle": (yb_fresh,), "second pass": (yb,)}, f"{form}, fill {fill}")
    set_fill(monkeypatch, None)
    err = rms(yb.numpy() - _gru_ref(b, "second input"))
    print(f"  {form} second input on a handle, fill 0x4B: rms error {err:.3e}")
    assert err < 2e-6, err   # tests/test_enhance.py:127


# ------------------------------------------------------------------------------------------------------------------ DfStream
STREAM_CUTS = (1, 3, 1, 2)
STREAM_VARIANTS = {
    # variant: (DfStream keywords, environment of the model, rows per stream)
    "plain": ({}, {}, 1),
    "gated": ({"gating": True}, {}, 1),
    "pausable": ({"pausable": True}, {}, 1),
    "sr16000": ({"sr": 16000}, {}, 1),
    "two_channels": ({"channels": 2}, {}, 2),
    "exact_fp32": ({}, {"DFX_EXACT_FP32": "1"}, 1),
}
EMU_STREAM = ("plain", "pausable", "sr16000")   # (gated handles: test_process_raw_ignores_scratch_contents runs there)
OPEN = (-1e9, 1e9, 1e9)   # thresholds with which no stage is ever skipped (tests/test_stream_slots.py)


@pytest.mark.parametrize("variant", list(STREAM_VARIANTS))
def test_streams_ignore_scratch_contents(backend, monkeypatch, variant):
    """Three streams, max_frames=4, calls of 1, 3, 1 and 2 hops: a handle's model workspace sits behind its state in ONE allocation, and
    dfx_stream_reset zeroes everything but it.  The pausable variant pauses stream 1 in the call of 3 hops: its rows of y are exact zeros and its
    lsnr NaN, every other sample and estimate is finite.  Under 0xFF every variant meets its oracle at the bar of its own existing test."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream
    from oracle import stream_oracle as S
    from tests.test_stream_slots import _fresh_stream_oracle

    if emu_subset(backend) and variant not in EMU_STREAM:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it); every variant runs on the GPU")
    kw, env, ch = STREAM_VARIANTS[variant]
    kw = dict(kw)
    name = "pf32" if backend == "emu" else "df3"
    p = named_params(name)
    sd = torch_sd(p, 9)
    T = sum(STREAM_CUTS)
    hop = 160 if variant == "sr16000" else HOP
    x = _noise((3 * ch, hop * T), 2)
    if variant == "gated":   # thresholds inside the observed lsnr values, so that stages are skipped (tests/test_streaming_gated.py _thresholds)
        from tests.test_streaming_gated import _thresholds

        kw["thresholds"] = _thresholds(p, sd, x.numpy(), (0.15, 0.85, 0.5))

    def model_for():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=9)
        for k in env:
            monkeypatch.delenv(k)
        return model, df_state

    def run(fill):
        model, df_state = model_for()
        rt = DfStream(model, df_state, streams=3 * ch, max_frames=4, **kw)
        assert rt.frame_length == hop
        out, pos = [], 0
        for call, n in enumerate(STREAM_CUTS):
            active = [True, call != 1, True] if variant == "pausable" else None
            with fresh_memory(fill):
                y, lsnr = rt.process(x[:, pos * hop:(pos + n) * hop], return_lsnr=True, active=active)
            pos += n
            if active is not None and not all(active):
                assert float(y[1].abs().max()) == 0.0 and bool(torch.isnan(lsnr[1]).all()), (fill, call)
                assert bool(torch.isfinite(y[[0, 2]]).all()) and bool(torch.isfinite(lsnr[[0, 2]]).all()), (fill, call)
            else:
                assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lsnr).all()), (fill, call)
            out += [y, lsnr]
        return out, model

    outs = _sweep(monkeypatch, run, f"stream {variant}")[0xFF]
    y, lsnr = torch.cat(outs[0::2], 1).numpy(), torch.cat(outs[1::2], 1).numpy()
    assert float(np.abs(y).max()) > 0
    xn = x.numpy()
    if variant in ("plain", "exact_fp32"):
        refs = np.stack([S.process_stream(p, sd, xi, thresholds=OPEN)[0] for xi in xn])
        err = rms(y - refs)
        assert err < 1e-6, err   # tests/test_streaming.py:56; tests/test_stream_modes.py holds exact handles to the same oracle at 1e-6
    elif variant == "gated":
        thr, d, err = kw["thresholds"], p.df_lookahead, 0.0
        for i, (yr, lr, info) in enumerate(S.process_stream(p, sd, xi, thresholds=thr) for xi in xn):
            assert min(np.abs(np.asarray(info["lsnr_pass1"]) - t).min() for t in thr) > 1e-4   # robust decisions only (tests/test_streaming_gated.py:88-90)
            err = max(err, rms(y[i] - yr))
            assert rms(y[i] - yr) < 1e-6, (i, rms(y[i] - yr))                                      # tests/test_streaming_gated.py:95
            acc = info["accepted"]
            live, frozen = np.zeros(T, bool), np.ones(T, bool)
            live[acc[d:]] = True
            frozen[acc] = False
            assert not live.any() or np.abs(lsnr[i] - lr)[live].max() < 1e-3                       # :99
            assert np.all(lsnr[i][frozen] == -15.0) and np.all(y[i].reshape(T, HOP)[frozen] == 0.0)   # :102-103
    elif variant == "two_channels":
        err = 0.0
        for k in range(3):
            ref = S.process_stream(p, sd, xn[2 * k: 2 * k + 2], thresholds=OPEN, reduce_mask="mean")[0]
            err = max(err, rms(y[2 * k: 2 * k + 2] - ref))
            assert rms(y[2 * k: 2 * k + 2] - ref) < 1e-6, k   # tests/test_streaming_gated.py:181-191
    elif variant == "pausable":
        # a stream's oracle is the oracle of the hops it DELIVERED, against its outputs over the calls it took part in (tests/test_stream_pause.py)
        keep = np.ones(T, bool)
        keep[1:4] = False   # stream 1 sat the call of 3 hops out
        err = 0.0
        for i in range(3):
            hops = keep if i == 1 else np.ones(T, bool)
            sig, got = xn[i].reshape(T, HOP)[hops].reshape(-1), y[i].reshape(T, HOP)[hops].reshape(-1)
            err = max(err, rms(got - _fresh_stream_oracle(p, sd, sig)))
            assert rms(got - _fresh_stream_oracle(p, sd, sig)) < 1e-6, i   # tests/test_stream_pause.py:105
    else:   # sr16000: tests/test_stream_rates.py _check_composition — the composition of existing parts at 1e-6, and no further from the CPU oracle chain than it
        from oracle import io_oracle as IO
        from tests.test_stream_rates import MSR, _composition, _P

        Pu, Pd = _P(16000, MSR), _P(MSR, 16000)
        up_o = IO.resample(np.concatenate([np.zeros((3, Pu), np.float32), xn], axis=1), 16000, MSR)[:, : T * HOP]
        z_o = np.stack([_fresh_stream_oracle(p, sd, np.ascontiguousarray(u, dtype=np.float32)) for u in up_o])
        chain = IO.resample(np.concatenate([np.zeros((3, Pd), np.float32), z_o], axis=1), MSR, 16000)[:, : T * hop]
        model, df_state = model_for()
        ref, _, _ = _composition(model, df_state, x, 16000, [("proc", c) for c in STREAM_CUTS])
        err, d0, d1 = rms(y - ref.numpy()), rms(ref.numpy() - chain), rms(y - chain)
        print(f"  stream {name} sr16000: composition vs oracle chain {d0:.3e}, this handle vs oracle chain {d1:.3e}")
        assert err < 1e-6, err          # tests/test_stream_rates.py:85
        assert d1 < d0 + 1e-6, (d0, d1)   # tests/test_stream_rates.py:86
    print(f"  stream {name} {variant} [{backend}] under 0xFF: rms error {err:.3e}")


def test_process_raw_ignores_scratch_contents(backend, monkeypatch):
    """dfx_stream_process_raw: seven spectral frames (the interpreter: four) for three streams of a gated handle; the pass's mask and coefficients leave through g_mask /
    g_coefs, the model workspace is the handle's own.  Compared: lsnr and stages of every call, and the gains / coefficients that stages reports.
    Thresholds as in tests/test_stream_modes.py test_exact_process_raw_matches_oracle: stage 1 always, stage 2 for the lower half of the
    observed lsnr values; under 0xFF every call meets oracle.stream_oracle.process_raw_frames at that test's bars."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream
    from oracle import stream_oracle as S

    name = "pf32" if backend == "emu" else "df3"
    p = named_params(name)
    sd = torch_sd(p, 9)
    d = L.DF(p.sr, p.fft_size, p.hop_size, p.nb_erb, p.min_nb_freqs)
    spec = torch.from_numpy(d.analysis(_noise((3, HOP * (4 if backend == "emu" else 7)), 3).numpy()))   # [3, frames, F] complex64
    K = spec.shape[1]
    free = [S.process_raw_frames(p, sd, spec[i].numpy(), thresholds=OPEN) for i in range(3)]
    vals = np.sort([r[0] for f in free for r in f if r[0] is not None])
    j = max(range(max(len(vals) // 2 - 2, 0), min(len(vals) // 2 + 2, len(vals) - 1)), key=lambda i: vals[i + 1] - vals[i])
    thr = (-1e9, 1e9, float(vals[j] + vals[j + 1]) / 2)
    assert min(abs(v - thr[2]) for v in vals) > 1e-4
    ref = [S.process_raw_frames(p, sd, spec[i].numpy(), thresholds=thr) for i in range(3)]
    assert any(r[2] is None and r[1] is not None for f in ref for r in f) and any(r[2] is not None for f in ref for r in f)

    def run(fill):
        model, df_state, _, _ = init_df(params=named_params(name), epoch="none", seed=9)
        rt = DfStream(model, df_state, streams=3, gating=True, thresholds=thr)
        out = []
        for t in range(K):
            with fresh_memory(fill):
                lsnr, gains, coefs, stages = rt.process_raw(spec[:, t].contiguous())
            # what stages calls absent does not exist (the reference hands back NULL there, include/dfx.h): those rows are not compared
            assert not bool((stages & ~torch.tensor(10, dtype=torch.uint8)).any()), stages
            have_g, have_c = (stages.cpu() & 2).bool(), (stages.cpu() & 8).bool()
            gains = torch.where(have_g[:, None], gains.cpu(), torch.zeros(()))
            coefs = torch.where(have_c[:, None, None, None], torch.view_as_real(coefs.cpu()), torch.zeros(()))
            out += [lsnr, gains, coefs, stages]
        return out, model

    outs = _sweep(monkeypatch, run, "process_raw")[0xFF]
    assert all(bool(torch.isfinite(o).all()) for o in outs if o.is_floating_point())
    worst = [0.0, 0.0, 0.0]
    for k in range(K):   # tests/test_stream_modes.py:249-259
        lsnr, gains, coefs, stages = outs[4 * k: 4 * k + 4]
        coefs = torch.view_as_complex(coefs.contiguous())
        for i in range(3):
            rl, rg, rc = ref[i][k]
            if rl is None:
                assert int(stages[i]) == 0 and float(lsnr[i]) == -15.0
                continue
            worst[0] = max(worst[0], abs(float(lsnr[i]) - rl))
            assert abs(float(lsnr[i]) - rl) < 1e-3
            assert bool(int(stages[i]) & 2) == (rg is not None) and bool(int(stages[i]) & 8) == (rc is not None)
            if rg is not None:
                worst[1] = max(worst[1], float(np.abs(gains[i].numpy() - rg).max()))
                assert np.abs(gains[i].numpy() - rg).max() < 1e-5
            if rc is not None:
                worst[2] = max(worst[2], float(np.abs(coefs[i].numpy() - rc).max()))
                assert np.abs(coefs[i].numpy() - rc).max() < 1e-5
    print(f"  process_raw {name} [{backend}] under 0xFF: largest error lsnr {worst[0]:.3e}, gains {worst[1]:.3e}, coefs {worst[2]:.3e}")


# ------------------------------------------------------------------------------------------------------------------ workspace-free kernels
def _fills(run, what):
    """run() under every pattern of FILLS (outputs only: these kernels take no workspace): the same bits = every element is written."""
    outs = {}
    for fill in FILLS:
        with fresh_memory(fill):
            outs[fill] = tuple(torch.as_tensor(np.ascontiguousarray(o) if isinstance(o, np.ndarray) else o) for o in run())
    assert_same_bits(outs, what)
    return outs[0xFF]


@pytest.mark.parametrize("N,H,nb", [(960, 480, 32), (96, 24, 8), (320, 160, 24)])
def test_stft_kernels_write_every_element(backend, N, H, nb):
    """analysis / synthesis at the ragged sizes of tests/test_dsp_kernels.py, also continued (reset=False: mem_out of one call is mem_in of the next)."""
    from deepfilternet_amd import libdf as D

    x = (0.3 * np.random.default_rng(N).standard_normal((3, H * 11 + 7))).astype(np.float32)

    def run():
        d = D.DF(48000, N, H, nb, 1)
        S = d.analysis(x)
        y = d.synthesis(S)
        d.reset()
        parts = [d.analysis(x[:1, a * H:b * H].copy(), reset=False) for a, b in ((0, 3), (3, 4), (4, 11))]
        d.reset()
        back = [d.synthesis(S[:1, a:b].copy(), reset=False) for a, b in ((0, 3), (3, 4), (4, 11))]
        return [S, y] + parts + back

    S, y = _fills(run, f"stft {N}/{H}")[:2]
    o = L.DF(48000, N, H, nb, 1)
    R = o.analysis(x)
    assert np.abs(S.numpy() - R).max() < 3e-7 * max(1.0, np.abs(R).max() / 0.02)   # tests/test_dsp_kernels.py:30
    r = o.synthesis(R.copy())
    assert np.abs(y.numpy() - r).max() < 2e-5 * np.abs(r).max()                     # tests/test_dsp_kernels.py:51 (on the oracle's own spectrum: 1e-6 apart)


def test_feature_kernels_write_every_element(backend):
    from deepfilternet_amd import libdf as D
    from deepfilternet_amd.enhance import df_features

    rng = np.random.default_rng(5)
    w = L.DF(48000, 960, 480, 32, 2).erb_widths()
    X = ((rng.standard_normal((2, 3, 9, 481)) + 1j * rng.standard_normal((2, 3, 9, 481))) * 0.1).astype(np.complex64)
    g = rng.uniform(0, 1, (2, 7, 32)).astype(np.float32)
    e = (rng.standard_normal((3, 37, 32)) * 8 - 50).astype(np.float32)
    U = (rng.standard_normal((2, 29, 96)) + 1j * rng.standard_normal((2, 29, 96))).astype(np.complex64)
    x = (0.1 * rng.standard_normal((3, 480 * 13 + 5))).astype(np.float32)

    def run():
        d = D.DF(48000, 960, 480, 32, 2)
        feats = [torch.view_as_real(t) if t.is_complex() else t for t in df_features(torch.from_numpy(x), d, 96)]
        return [D.erb(X, w, True), D.erb(X, w, False), D.erb_inv(g, w), D.erb_norm(e.copy(), 0.99), D.unit_norm(U, 0.99)] + feats

    out = _fills(run, "features")
    assert np.allclose(out[0].numpy(), L.erb(X, w, True), rtol=2e-6, atol=2e-5)   # tests/test_dsp_kernels.py:96
    assert np.array_equal(out[2].numpy(), L.erb_inv(g, w))                        # :99
    assert np.allclose(out[3].numpy(), L.erb_norm(e.copy(), 0.99), rtol=1e-6, atol=1e-6)   # :113


@pytest.mark.parametrize("B,T,F,nd,O_,la,layout", [(2, 19, 481, 96, 5, 2, 0), (3, 21, 33, 8, 1, 0, 2), (2, 5, 64, 64, 3, 1, 0)])
def test_df_apply_writes_every_element(backend, B, T, F, nd, O_, la, layout):
    """dfx_df_apply on dense rows (the flat-stream kernel; its output is a torch.empty_like) and on padded rows (dfx_k_df_apply_rows)."""
    from tests.test_df_apply import run_df_apply, run_df_apply_strided

    rng = np.random.default_rng(B * 1000 + T + O_)
    spec = (rng.standard_normal((B, T, F)) + 1j * rng.standard_normal((B, T, F))).astype(np.complex64)
    cbotf = ((rng.standard_normal((B, O_, T, nd)) + 1j * rng.standard_normal((B, O_, T, nd))) * 0.3).astype(np.complex64)
    coefs = cbotf if layout == 0 else np.ascontiguousarray(cbotf.transpose(0, 2, 1, 3))
    widths = np.full(8, F // 8, np.uint64)
    widths[-1] += F - int(widths.sum())
    gains = rng.uniform(0, 1, (B, T, 8)).astype(np.float32)

    def run():
        return [run_df_apply(spec, coefs, layout, gains, widths, nd, O_, la), run_df_apply(spec, coefs, layout, None, None, nd, O_, la),
                run_df_apply_strided(spec, coefs, layout, gains, widths, nd, O_, la)]

    flat = _fills(run, f"df_apply {B}x{T}x{F}")[0]
    st = torch.from_numpy(spec)
    ref = st * O.band_gain(torch.from_numpy(gains), widths)
    ref[..., :nd] = O.df_apply(st, torch.from_numpy(cbotf), O_, la, nd)
    assert np.abs(flat.numpy() - ref.numpy()).max() < 2e-5 * max(1.0, float(ref.abs().max()))   # tests/test_df_apply.py:83


def test_io_kernels_write_every_element(backend):
    """resample (ragged lengths, both directions), StreamResampler call by call (one row paused in one call), the PCM16 converters."""
    from deepfilternet_amd import io as IO

    rng = np.random.default_rng(9)
    x = torch.from_numpy((0.3 * rng.standard_normal((3, 4801))).astype(np.float32))
    pcm = torch.from_numpy(rng.integers(-32768, 32767, (2, 1237), dtype=np.int16))

    def run():
        out = [IO.resample(x, 48000, 16000), IO.resample(x[:, :1603], 16000, 48000), IO.resample(x, 44100, 48000),
               IO.pcm16_to_float(pcm), IO.float_to_pcm16(x)]
        rs = IO.StreamResampler(48000, 16000, rows=3)
        for k, (a, b) in enumerate(((0, 480), (480, 1920), (1920, 2400))):
            out.append(rs.process(x[:, a:b], active=[True, k != 1, True] if k == 1 else None))
        out.append(rs.process((x[:, 2400:3360] * 32768).clamp(-32768, 32767).to(torch.int16)))
        return out

    out = _fills(run, "io")
    assert torch.equal(out[3].cpu(), pcm.to(torch.float32) / 32768)
    assert float(out[6][1].abs().max()) == 0.0 and float(out[6][0].abs().max()) > 0   # the paused row: zeros


def test_mf_filters_write_every_element(backend):
    """MfWf / MfMvdr at the ragged shapes of tests/test_mf.py (T shorter than the filter, bins that do not fill a wave)."""
    from deepfilternet_amd import multiframe as MF
    from oracle import mf_oracle as M

    for mvdr, N, la, chol, inv in ((False, 5, 2, False, True), (True, 6, 1, True, True)):
        rng = np.random.default_rng(N * 7 + la)
        for B, T, F, nb in ((1, 3, 33, 33), (2, 5, 40, 17), (2, 1, 9, 4)):
            spec = rng.standard_normal((B, 1, T, F, 2)).astype(np.float32)
            ifc = rng.standard_normal((B, T, nb, 2 * N)).astype(np.float32)
            a = rng.standard_normal((B, T, nb, N, N)) + 1j * rng.standard_normal((B, T, nb, N, N))
            m = 0.3 * np.tril(a, -1) + 2 * np.eye(N) if chol else a @ a.conj().swapaxes(-1, -2) / N + np.eye(N)
            mat = np.stack([m.real, m.imag], -1).reshape(B, T, nb, 2 * N * N).astype(np.float32)
            op = (MF.MfMvdr if mvdr else MF.MfWf)(nb, N, lookahead=la, cholesky_decomp=chol, inverse=inv)
            y = _fills(lambda: [op(torch.from_numpy(spec), torch.from_numpy(ifc), torch.from_numpy(mat))], f"mf {mvdr} {B}x{T}x{F}")[0]
            ref = M.mf_filter(torch.from_numpy(spec), torch.from_numpy(ifc), torch.from_numpy(mat), mvdr=mvdr, num_freqs=nb, frame_size=N,
                              lookahead=la, cholesky_decomp=chol, inverse=inv).numpy()
            assert np.abs(y.numpy() - ref).max() < 5 * 2e-5 * max(1.0, float(np.abs(ref).max()))   # tests/test_mf.py:69


def test_the_patterns_are_what_they_claim():
    """0xFF is NaN in both float formats; 0x4B is finite, beyond the fp16-split range as float32 and far outside every tolerance as float16."""
    ff, kb = np.full(4, 0xFF, np.uint8), np.full(4, 0x4B, np.uint8)
    assert np.isnan(ff.view(np.float32)[0]) and np.isnan(ff.view(np.float16)).all() and ff.view(np.int32)[0] == -1
    assert 1.3e7 < kb.view(np.float32)[0] < 1.4e7 and kb.view(np.float32)[0] > 6e4 and 14.5 < float(kb.view(np.float16)[0]) < 14.7
    with fresh_memory(0x4B):
        t, u = torch.empty((3, 5)), torch.empty_like(torch.zeros(2, dtype=torch.complex64))
    assert bits(t).tolist() == [0x4B] * 60 and bits(u).tolist() == [0x4B] * 16
    assert torch.empty is not None and torch.empty.__name__ == "empty"   # restored
