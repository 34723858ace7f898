"""Every kind of model shape check_cfg accepts against the oracle, not just the four named configurations: tests/helpers.py SHAPES moves one or
two dimensions at a time off DeepFilterNet3 (band / bin counts, filter order, pathway kernel, GRU stack depths, group counts, lookaheads, FFT and
hop size) and says which decisions of a pass each entry flips; DfNet.last_plan() (dfx_model_query DFX_Q_LAST_PLAN) reports what a pass decided,
so that the suite itself shows that its shapes reach both sides of every decision.  Configurations just outside the accepted space are refused
with the library's message, and what the frame-by-frame runtime cannot run is refused when the runtime is created.

The interpreter runs about six shapes per test (DFX_EMU_ALL=1: all of them); every shape runs on the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepfilternet_amd.config import ModelParams
from deepfilternet_amd.state_dict import random_state_dict
from oracle import dfnet_oracle as O
from tests.helpers import NAMED, SHAPES, emu_subset, rms, shape_params, widths_for

# what the interpreter runs by default: between them the three lists hold every entry of SHAPES but l4_d3 / l5_d3 / look31 / f32 (whose
# differences from their neighbours only show in the GPU-only forms or in nothing the interpreter decides differently)
EMU_FORWARD = ("e24_f64", "e64", "kt7", "lg8", "l2_d1", "c32_e8_f16")
EMU_ENHANCE = ("f128", "kt4_o8", "o1", "c32_e64", "fft512", "hop240")
EMU_STREAM = ("e16", "kt2_o3", "l4_d1", "lg4_elg16", "c32_e8_f16", "c16_e16_f32_o6")
# shapes the frame-by-frame runtime refuses at creation, with the reason the message gives
STREAM_REFUSED = {"e64": "fused ERB encoder head", "c32_e64": "fused ERB encoder head", "look31": "conv_lookahead != df_lookahead",
                  "kt7": "fused DF encoder", "df3_o10": "fused DF encoder"}
STREAM_SHAPES = [n for n in SHAPES if n not in STREAM_REFUSED]
SEED = 11


def _sd(p, seed=SEED):
    return random_state_dict(p, seed, widths=widths_for(p))


def _tsd(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def _noise(shape, seed):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32))


def _cmp(a, b, tol, what):
    """tests/test_dfnet_kernels.py _cmp: largest error relative to max(1, largest reference value); returns it"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))
    print(f"    {what}: {err:.3e} (tol {tol:.0e})")
    assert err <= tol, (what, err)
    return err


def _expect_presplit(p):
    """batch passes read the pre-split copy of feat_spec where the fp16-split fused DF-encoder kernels exist: conv_ch a multiple of 32 and the
    sliding-window pathway conv (dfx_model_create: fuse_c0)"""
    return p.conv_ch % 32 == 0 and p.df_pathway_kernel_size_t <= 5 and 2 * p.df_order <= 16


@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_shapes_match_oracle(backend, shape):
    """DfNet.forward: two full 16-frame tiles and a partial one on the GPU (T >= 16: the norm-scan / PS forms), ragged B."""
    from deepfilternet_amd.model import DfNet

    if emu_subset(backend) and shape not in EMU_FORWARD:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it); every shape runs on the GPU")
    p = shape_params(shape)
    sd = _sd(p)
    model = DfNet(p, sd)
    B, T = (2, 19) if backend == "emu" else (3, 37)
    rng = np.random.default_rng(B + T)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy(rng.standard_normal((B, 1, T, p.nb_df, 2)).astype(np.float32))
    ref = O.dfnet_forward(p, _tsd(sd), widths_for(p), spec, fe, fs)
    spec_e, m, lsnr, coefs = model(spec, fe, fs)
    model.check()
    print(f"  {shape} [{backend}] forward, error / max(1, |ref|max):")
    _cmp(m.cpu(), ref["m"], 3e-5, "mask")
    _cmp(lsnr.cpu(), ref["lsnr"], 3e-5, "lsnr")
    _cmp(coefs.cpu(), ref["df_coefs"], 5e-5, "df_coefs")
    _cmp(spec_e.cpu(), ref["spec_e"], 5e-5, "spec_e")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_enhance_shapes_match_oracle(backend, shape):
    from deepfilternet_amd.enhance import enhance, init_df

    if emu_subset(backend) and shape not in EMU_ENHANCE:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it); every shape runs on the GPU")
    p = shape_params(shape)
    sd = _sd(p)
    model, df_state, _, _ = init_df(params=p, state_dict=sd, epoch="none")
    B, hops = (2, 19) if backend == "emu" else (3, 37)
    x = _noise((B, hops * p.hop_size + 7), 5)
    ref = O.enhance(p, _tsd(sd), x.numpy())
    for call in range(1 if backend == "emu" else 2):   # (GPU: the second call runs in the workspace the first one left)
        before = model.query(model.Q_PASSES_C0_PRESPLIT)
        y = enhance(model, df_state, x)
        model.check()
        plan = model.last_plan()
        assert plan["presplit"] == _expect_presplit(p), plan
        assert model.query(model.Q_PASSES_C0_PRESPLIT) - before == (1 if plan["presplit"] else 0)
        err = rms(y.cpu().numpy() - ref)
        print(f"  {shape} [{backend}] enhance call {call}: rms error {err:.3e} (signal rms {rms(ref):.3e})")
        assert y.shape == x.shape and err < 2e-6, (shape, call, err)


# Decisions that check_cfg leaves only one side of, each with the arithmetic that excludes the other side.  Only such bits may stand here.
UNREACHABLE = {
    # fuse_dec: dfx_k_erb_dec10 needs E % 2 == 0 && 2 * DFX_DEC10_SMEM(C, E) <= 160 KiB.  check_cfg takes nb_erb in multiples of 8 up to 64 (even)
    # and conv_ch 16 / 32 / 64; DFX_DEC10_SMEM(C, E) = (3C/4 + 4C/4 + 3C/4) * 16 + 16 * (E * (C + 4) + 4 E) bytes grows with both, and at the
    # largest, C = 64, E = 64, it is 2560 + 16 * 4608 = 76288 bytes: 2 * 76288 = 152576 <= 163840.  So fuse_dec is never false: the layer-by-layer
    # end (a separate convt1, then dfx_k_conv_out) is gone from the library, and a static_assert beside check_cfg holds the bound.
    ("fuse_dec", False),
}


def test_every_plan_decision_is_seen_both_ways(backend):
    """The union of DfNet.last_plan() over SHAPES and the four named configurations shows every decision of a pass both taken and not taken, and
    every form of df_out — so a kernel family cannot lose its only test shape unnoticed.  One two-hop enhance() per configuration decides
    everything but the form of the GRU phase, which takes a long pass with internal streams: the GPU run adds one (pipe, use_seq)."""
    from deepfilternet_amd.enhance import enhance, init_df
    from deepfilternet_amd.model import DfNet

    sized = ("pipe", "use_seq")   # decided by the size of the pass and the device, not by the shape
    seen = {k: set() for k in DfNet.PLAN_BITS}
    forms, plans = set(), {}
    for name in list(SHAPES) + list(NAMED):
        p = shape_params(name)
        model, df_state, _, _ = init_df(params=p, epoch="none", seed=1)
        assert model.query(model.Q_LAST_PLAN) == 0   # no pass yet
        enhance(model, df_state, _noise((1, 2 * p.hop_size), 3))
        model.check()
        plan = plans[name] = model.last_plan()
        assert not plan["pipe"] and not plan["use_seq"], (name, plan)   # three frames: the serial form of the GRU phase
        forms.add(plan["df_out"])
        for k in seen:
            seen[k].add(plan[k])
    if backend == "hip":
        p = shape_params("df3")
        model, df_state, _, _ = init_df(params=p, epoch="none", seed=1)
        enhance(model, df_state, _noise((2, 70 * p.hop_size), 3))
        model.check()
        plan = model.last_plan()
        assert plan["pipe"] and plan["use_seq"] and model.query(model.Q_PASSES_PERSISTENT) == 1, plan
        for k in sized:
            seen[k].add(plan[k])
    else:
        for k in sized:
            del seen[k]
    print("  decisions per configuration:")
    for name, plan in plans.items():
        print(f"    {name:16s} df_out {plan['df_out']:9s} " + " ".join(k for k in DfNet.PLAN_BITS if plan[k]))
    for k, vals in seen.items():
        missing = {True, False} - vals - {v for kk, v in UNREACHABLE if kk == k}
        assert not missing, f"no configuration of the suite decides {k} = {sorted(missing)}"
        for kk, v in UNREACHABLE:
            assert not (kk == k and v in vals), f"{k} = {v} is listed as unreachable but was seen"
    assert forms == {"resident", "streaming", "ggemm"}, forms
    # what tests/helpers.py says its shapes flip against df3
    df3 = plans["df3"]
    assert all(df3[k] for k in DfNet.PLAN_BITS if k not in sized) and df3["df_out"] == "resident", df3
    flips = {"e64": ("fuse_enc", "fuse_enc4"), "c32_e64": ("fuse_enc", "fuse_enc4"), "kt7": ("c0_fused", "fuse_h3", "presplit", "dfenc"),
             "lg8": ("fan", "fan_skp"), "lg4_elg16": ("fan", "fan_skp", "enc_fan", "dfenc"), "fft512": ("rows_finish",), "hop240": ("rows_finish",),
             "kt2_o3": ("rows_finish",), "kt4_o8": ("rows_finish",), "o1": ("rows_finish",),
             "c16_e16_f32_o6": ("fuse_h3", "presplit", "fuse_tail", "fuse_enc4", "dfenc", "rows_finish")}
    for name, bits in flips.items():
        for k in bits:
            assert not plans[name][k], (name, k, plans[name])
    assert plans["kt4_o8"]["c0_fused"] and plans["f128"]["rows_finish"]
    assert plans["lg8"]["df_out"] == "streaming" and plans["lg4_elg16"]["df_out"] == "ggemm"


GRU_SHAPES = ["defaults", "pf32", "l4_d1", "l4_d3", "l5_d3", "l2_d1", "e24_f64", "lg8", "c16_e16_f32_o6"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GRU_SHAPES)
def test_gru_phase_forms_agree_on_other_shapes(hip_backend, shape, monkeypatch):
    """The serial, the event-synchronised and the persistent form of the GRU phase (the latter on pairs of CUs and on single ones) on other
    layer counts and widths than DeepFilterNet3's: 33 clips = two full 16-clip groups and one clip, a pair with an empty half, several
    follower blocks per sequence.  In this order, so that a failure names the first form that breaks."""
    from deepfilternet_amd.enhance import enhance, init_df

    p = shape_params(shape)
    sd = _sd(p, 17)
    x = _noise((33, p.hop_size * 70 + 11), 4)
    switches = ("DFX_STREAMS", "DFX_GRU_SEQ", "DFX_GRU_PAIR")

    def run(env):
        for k in switches:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model, df_state, _, _ = init_df(params=p, state_dict=sd, epoch="none")   # (the switches are read when the handle is created)
        y = enhance(model, df_state, x)
        model.check()
        return y.cpu(), model.query(model.Q_PASSES_PERSISTENT), model.last_plan()

    rows = [0, 32]
    ref = O.enhance(p, _tsd(sd), x[rows].numpy())
    outs = {}
    for form, env in (("serial", {"DFX_STREAMS": "0"}), ("event", {"DFX_GRU_SEQ": "0"}), ("persistent_single", {"DFX_GRU_PAIR": "0"}),
                      ("persistent", {})):
        y, passes, plan = run(env)
        persistent = form.startswith("persistent")
        assert plan["pipe"] == (form != "serial") and plan["use_seq"] == persistent, (form, plan)
        assert (passes >= 1) if persistent else (passes == 0), (form, passes)
        err = rms(y[rows].numpy() - ref)
        print(f"  {shape} {form}: rms error of rows 0, 32 against the oracle {err:.3e}")
        assert err < 2e-6, (form, err)
        for other, yo in outs.items():
            d = rms((y - yo).numpy())
            print(f"  {shape} {form} - {other}: rms {d:.3e}")
            assert d < 1e-6, (form, other, d)
        outs[form] = y
    assert torch.equal(outs["persistent"], outs["persistent_single"])   # the same arithmetic on pairs of CUs and on single ones


def _run_stream(rt, x, cuts):
    hop = rt.frame_length
    out, pos = [], 0
    for n in cuts:
        out.append(rt.process(x[:, pos * hop:(pos + n) * hop]))
        pos += n
    assert pos * hop == x.shape[1]
    return torch.cat(out, dim=1)


@pytest.mark.parametrize("shape", STREAM_SHAPES)
def test_stream_shapes_equal_batch_delayed(backend, shape):
    """tests/test_streaming.py test_stream_equals_batch_delayed on every shape the frame-by-frame runtime takes: its output is the batch path's
    (itself held to the oracle here) delayed by the model's lookahead, however the signal is cut into calls; the warm-up hops are silence."""
    from deepfilternet_amd.enhance import enhance, init_df
    from deepfilternet_amd.streaming import DfStream

    if emu_subset(backend) and shape not in EMU_STREAM:
        pytest.skip("interpreter subset (DFX_EMU_ALL=1 runs it); every shape runs on the GPU")
    p = shape_params(shape)
    assert not p.mask_pf
    sd = _sd(p, 9)
    model, df_state, _, _ = init_df(params=p, state_dict=sd, epoch="none")
    hop, T = p.hop_size, (9 if backend == "emu" else 23)
    x = _noise((3, hop * T), 2)
    ref = enhance(model, df_state, x, pad=False)
    assert rms(ref.cpu().numpy() - O.enhance(p, _tsd(sd), x.numpy(), pad=False)) < 2e-6
    rt = DfStream(model, df_state, streams=3, max_frames=7)
    d = rt.delay_frames
    assert d == p.df_lookahead and rt.frame_length == hop
    for cuts in (([1, 3, 1, 4],) if backend == "emu" else ([1] * T, [7, 7, 7, 2], [3, 1, 5, 2, 7, 1, 4])):
        rt.reset()
        y = _run_stream(rt, x, cuts)
        assert y.shape == x.shape
        if d:
            assert float(y[:, : d * hop].abs().max()) == 0.0   # warm-up hops are silence
        err = rms((y[:, d * hop:] - ref[:, : (T - d) * hop]).cpu().numpy())
        print(f"  {shape} [{backend}] cuts {cuts if len(cuts) < 9 else '1 x %d' % len(cuts)}: rms {err:.3e}")
        assert err < 1e-6, (cuts, err)
    model.check()
    assert not model.last_plan()["presplit"]   # the runtime's passes keep the fp32 features


def _df3(**kw):
    p = ModelParams.deepfilternet3()
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


F_DF3 = ModelParams.deepfilternet3().freq_bins
# just outside check_cfg: (configuration, exception of check_supported(), a piece of dfx_last_error()'s text)
REFUSED = {
    "nb_erb_12": (_df3(nb_erb=12), NotImplementedError, "nb_erb must be a multiple of 8"),
    "nb_erb_72": (_df3(nb_erb=72), NotImplementedError, "nb_erb must be a multiple of 8"),
    "nb_df_97": (_df3(nb_df=97), NotImplementedError, "nb_df must be even"),
    "nb_df_F_plus_1": (_df3(nb_df=F_DF3 + 1), NotImplementedError, "nb_df must be even and <= F"),
    "order_17": (_df3(df_order=17), NotImplementedError, "df_lookahead < df_order <= 16"),
    "lookahead_eq_order": (_df3(df_order=2, df_lookahead=2, conv_lookahead=2), NotImplementedError, "df_lookahead < df_order"),
    "kt_0": (_df3(df_pathway_kernel_size_t=0), NotImplementedError, "df_pathway_kernel_size_t must be 1..8"),
    "kt_9": (_df3(df_pathway_kernel_size_t=9), NotImplementedError, "df_pathway_kernel_size_t must be 1..8"),
    "kt8_o16": (_df3(df_pathway_kernel_size_t=8, df_order=16), NotImplementedError, "df_convp group shape"),
    "nb_df_130": (_df3(nb_df=130), NotImplementedError, "enc_linear_groups=32 does not tile df_fc_emb"),
    "emb_layers_1": (_df3(emb_num_layers=1), NotImplementedError, "emb_num_layers >= 2"),
    "conv_ch_48": (_df3(conv_ch=48), NotImplementedError, "conv_ch=48"),
}


def test_shapes_refused_loudly(backend, tmp_path):
    """Configurations just outside the accepted space are refused by ModelParams.check_supported() with the library's own message and by
    dfx_model_create with the same code; what the frame-by-frame runtime cannot run is refused when it is created — by DfStream(...) and by the
    C API's df_create — not by its first hop."""
    from deepfilternet_amd import _lib, export_dfx
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    L = _lib.lib()
    for name, (p, exc, text) in REFUSED.items():
        with pytest.raises(exc) as ei:
            p.check_supported()
        msg = L.dfx_last_error().decode()
        assert text in msg and msg in str(ei.value), (name, msg, str(ei.value))
        cfg, n, h = p.to_cfg(), C.c_int64(), C.c_void_p()
        rc = L.dfx_model_blob_floats(C.byref(cfg), C.byref(n))
        dummy = np.zeros(16, np.float32)   # (never read: the configuration is checked first)
        assert rc == _lib.DFX_ERR_UNSUPPORTED
        assert L.dfx_model_create(C.byref(cfg), dummy.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h)) == rc and not h.value, name
        assert text in L.dfx_last_error().decode(), name
    for name, text in STREAM_REFUSED.items():
        p = shape_params(name)
        p.check_supported()   # a model, not a stream
        sd = random_state_dict(p, 3)
        model, df_state, _, _ = init_df(params=p, state_dict=sd, epoch="none")
        with pytest.raises(_lib.DfxError) as ei:
            DfStream(model, df_state, streams=2, max_frames=2)
        assert ei.value.code == _lib.DFX_ERR_UNSUPPORTED and "dfx_stream_create:" in str(ei.value) and text in str(ei.value), (name, str(ei.value))
        if name in ("e64", "kt7"):   # the C API creates its state through the same function: no handle that could never process a hop
            path = export_dfx(str(tmp_path / f"{name}.dfx"), params=p, state_dict=sd)
            capi = C.CDLL(_lib.library_path())
            capi.df_create.restype, capi.df_create.argtypes = C.c_void_p, [C.c_char_p, C.c_float, C.c_char_p]
            assert capi.df_create(path.encode(), 100.0, None) is None
            assert "dfx_stream_create:" in L.dfx_last_error().decode() and text in L.dfx_last_error().decode()
