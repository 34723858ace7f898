"""The network kernels, the GRU phase first of all, against a FLOAT64 oracle under weights that make the GRUs work.

Why: the tolerances of the other forward tests (3e-5 .. 5e-5 of max(1, |ref|max), against a float32 oracle) are 150 to 300 times what the kernels
achieve, and under random_state_dict the GRU stacks are almost idle (|h| <= 0.19, no gate saturates): rounding all ten GRU matrices to f16 — the
lo half of the fp16-split product gone — stays inside them.  Here

  * the weights are tests/helpers.py lively_state_dict (gates saturate, z holds states over many frames, h moves by tenths per step:
    test_lively_weights_make_the_grus_work holds the recipe to that);
  * the reference is oracle/dfnet_oracle.py run in float64 (it follows the dtype of what it is given);
  * the bound comes from the oracle alone, per case and output k (mask, lsnr, df_coefs, spec_e), |a - b| the largest absolute difference:
        E32 = |oracle_f32 - oracle_f64|                      float32's own error on this model and these inputs
        S21 = |oracle_f64(W (1 +- 2^-21)) - oracle_f64(W)|   every weight tensor of two or more dimensions with a seeded random sign per element:
                                                             the documented size of ONE fp16-split product error, propagated
        the kernel passes when |kernel - oracle_f64| <= MARGIN * max(E32, S21)
    MARGIN = 4 is two factors of two: the kernel splits BOTH operands of a product where S21 perturbs one, and the kernel's summation order is a
    second, independent draw of a rounding error the size of E32.  Nothing in the bound is derived from what the kernels return.
  * the test shows that it sees what it is for: mutants of the ORACLE (a family's weights rounded to f16 — what that family's kernel would compute
    without the lo halves) must move an output they reach by at least 10 * MARGIN * max(E32, S21).  All seven families of DESIGN §4 are asserted
    on every case (both GRU mutants, erb_conv1-3 pointwise, df_conv0 / df_conv1 / df_fc_emb, df_convp, df_out, conv0_out).  One cell needed other
    inputs: df_out on l5_d3 (see ERB_SCALE below).

The achieved ratio |kernel - oracle_f64| / max(E32, S21) is printed per output, form and backend (pytest -s); docs/measurements.md records it."""
import functools

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from tests.helpers import lively_state_dict, shape_params, widths_for

MARGIN = 4.0
SEES = 10.0       # a mutant must move an output by SEES * MARGIN * max(E32, S21)
SEED = 11
OUTS = ("m", "lsnr", "df_coefs", "spec_e")
SWITCHES = ("DFX_GRU_SEQ", "DFX_EXACT_FP32", "DFX_GRU_PAIR", "DFX_GRU_PAIR_FAR", "DFX_STREAMS")

# the fp16-split families of DESIGN §4 as sets of state-dict keys (tensors of two or more dimensions under these prefixes)
FAMILIES = {
    "decoder GRUs": lambda k, v: k.startswith(("erb_dec.emb_gru.gru.weight_", "df_dec.df_gru.gru.weight_")),
    "encoder GRU": lambda k, v: k.startswith("enc.emb_gru.gru.weight_"),
    "erb_conv1-3 pointwise": lambda k, v: k.startswith(("enc.erb_conv1.", "enc.erb_conv2.", "enc.erb_conv3.")) and tuple(v.shape[2:]) == (1, 1),
    "df_conv0 / df_conv1 / df_fc_emb": lambda k, v: k.startswith(("enc.df_conv0.", "enc.df_conv1.", "enc.df_fc_emb.")),
    "df_convp": lambda k, v: k.startswith("df_dec.df_convp."),
    "df_out": lambda k, v: k.startswith("df_dec.df_out."),
    "conv0_out": lambda k, v: k.startswith("erb_dec.conv0_out."),
}
# Standard deviation of the ERB features, per shape (0.5 unless listed: the recipe of tests/test_model_shapes.py).  l5_d3: with three DF GRU layers S21 on
# the coefficients grows with the depth of the stack (1.8e-5 against 1.2e-5 on df3) while the movement of the df_out mutant does not, and at 0.5
# that mutant reaches 8.9 times, not 10.  The decoders see the inputs only through emb, a bounded function of the encoder GRU's state, so no
# input has much leverage on this cell: over six input seeds it came to 6.7 ... 12.2 at 0.5 and 7.0 ... 11.9 at 1.5, and features correlated
# over time gave the same range (docs/measurements.md).  As the condition is the one to keep, l5_d3 runs the inputs that reach it: 1.5 with
# the seed of every other case gives 11.9 (every other family 21 or more).
ERB_SCALE = {"l5_d3": 1.5}


def _inputs(p, B, T, erb_scale=0.5):
    """the recipe of tests/test_model_shapes.py test_forward_shapes_match_oracle"""
    rng = np.random.default_rng(B + T)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((erb_scale * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy(rng.standard_normal((B, 1, T, p.nb_df, 2)).astype(np.float32))
    return spec, fe, fs


def _oracle(p, sd, x, dtype):
    return O.dfnet_forward(p, O.to_dtype(sd, dtype), widths_for(p), *(t.to(dtype) for t in x), manual_gru=True)


def round_to_f16(sd, family):
    """(the state dict with the family's matrices rounded to f16 and back, how many tensors that were)"""
    out, n = dict(sd), 0
    for k, v in sd.items():
        v = torch.as_tensor(v)
        if v.ndim >= 2 and v.is_floating_point() and FAMILIES[family](k, v):
            out[k], n = v.to(torch.float32).half().to(v.dtype), n + 1
    return out, n


def _perturbed(sd64):
    """W (1 +- 2^-21): a seeded random sign per element of every weight tensor of two or more dimensions"""
    g = torch.Generator().manual_seed(21)
    out = {}
    for k, v in sd64.items():
        if v.ndim >= 2 and v.is_floating_point():
            v = v * (1.0 + (2.0 * torch.randint(0, 2, v.shape, generator=g).to(v.dtype) - 1.0) * 2.0 ** -21)
        out[k] = v
    return out


def _diff(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


@functools.lru_cache(maxsize=None)
def reference(shape, B, T):
    """Everything a case needs from the oracle, computed once per (shape, B, T) and left unchanged: parameters, weights, inputs, the float64
    outputs, base[k] = max(E32, S21) and the mutants' movement in units of MARGIN * base."""
    p = shape_params(shape)
    sd = lively_state_dict(p, SEED)
    x = _inputs(p, B, T, ERB_SCALE.get(shape, 0.5))
    r64, r32 = _oracle(p, sd, x, torch.float64), _oracle(p, sd, x, torch.float32)
    assert all(r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32 for k in OUTS)
    rp = O.dfnet_forward(p, _perturbed(O.to_dtype(sd, torch.float64)), widths_for(p), *(t.double() for t in x), manual_gru=True)
    e32, s21 = {k: _diff(r32[k], r64[k]) for k in OUTS}, {k: _diff(rp[k], r64[k]) for k in OUTS}
    base = {k: max(e32[k], s21[k]) for k in OUTS}
    assert all(0 < base[k] < 1e-4 for k in OUTS), base   # (float32-sized: a bound of another order would say the oracle itself is off)
    mutants = {}
    for fam in FAMILIES:
        sdm, n = round_to_f16(sd, fam)
        assert n >= 1, fam
        rm = _oracle(p, sdm, x, torch.float64)
        mutants[fam] = {k: _diff(rm[k], r64[k]) / (MARGIN * base[k]) for k in OUTS}
    return {"p": p, "sd": sd, "x": x, "r64": {k: r64[k] for k in OUTS}, "e32": e32, "s21": s21, "base": base, "mutants": mutants}


def _check_mutants(ref, label):
    print(f"  {label}: oracle only, E32 / S21 and what a family's weights rounded to f16 move, in units of MARGIN * max(E32, S21):")
    print("    E32  " + "  ".join(f"{k} {ref['e32'][k]:.2e}" for k in OUTS))
    print("    S21  " + "  ".join(f"{k} {ref['s21'][k]:.2e}" for k in OUTS))
    for fam, moved in ref["mutants"].items():
        print(f"    {fam:32s}" + "  ".join(f"{k} {moved[k]:6.1f}" for k in OUTS))
    for fam in FAMILIES:
        assert max(ref["mutants"][fam].values()) >= SEES, (label, fam, ref["mutants"][fam])


def _check_kernel(ref, outs, label):
    """outs: (spec_e, m, lsnr, coefs) of the engine"""
    got = dict(zip(("spec_e", "m", "lsnr", "df_coefs"), outs))
    ratios = {}
    for k in OUTS:
        a = got[k].cpu()
        assert a.shape == ref["r64"][k].shape and torch.isfinite(a).all(), (label, k)
        ratios[k] = _diff(a, ref["r64"][k]) / ref["base"][k]
    print(f"  {label}: |kernel - oracle_f64| / max(E32, S21):  " + "  ".join(f"{k} {ratios[k]:.2f}" for k in OUTS))
    for k in OUTS:
        assert ratios[k] <= MARGIN, (label, k, ratios[k])
    return ratios


def _model(monkeypatch, ref, env, pipeline=None):
    from deepfilternet_amd.model import DfNet

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = DfNet(ref["p"], ref["sd"])   # (the switches are read when the handle is created)
    assert model.query(model.Q_EXACT_FP32) == int(env.get("DFX_EXACT_FP32") == "1")
    if pipeline:
        model.set_pipeline(**pipeline)
    return model


def _forward(model, ref, form):
    """one pass, with the form of its GRU phase asserted: 'serial', 'events', 'persistent' (one CU per 16 clips) or 'pair'"""
    before, before_pair = model.query(model.Q_PASSES_PERSISTENT), model.query(model.Q_PASSES_PAIR)
    outs = model(*ref["x"])
    model.check()
    plan = model.last_plan()
    persistent = form in ("persistent", "pair")
    assert plan["pipe"] == (form != "serial") and plan["use_seq"] == persistent, (form, plan)
    assert model.query(model.Q_PASSES_PERSISTENT) - before == int(persistent), form
    assert model.query(model.Q_PASSES_PAIR) - before_pair == int(form == "pair"), form
    if persistent:
        assert model.query(model.Q_GRU_PERSISTENT) == 1
    return outs


CHUNKED = {"time_chunks": 12, "min_chunk_frames": 2}   # sequences this short only take the layer-pipelined forms with short chunks allowed


def test_lively_weights_make_the_grus_work():
    """Oracle only, DeepFilterNet3 at (3, 37): in each of the three GRU stacks at least 15 % of the states have |h| > 0.9, h moves by at least
    0.1 (std) per step, and nothing an fp16-split kernel has to split comes near the f16 range (tests/test_fp16_range.py's guard stays quiet)."""
    ref = reference("df3", 3, 37)
    p, x = ref["p"], ref["x"]
    sd = O.to_dtype(ref["sd"], torch.float64)
    out = O.dfnet_forward(p, sd, widths_for(p), *(t.double() for t in x), manual_gru=True)
    lin = lambda v, key: torch.relu(O.grouped_linear(v, sd[key]))
    stacks = {"enc.emb_gru": (out["emb_in"], 1), "erb_dec.emb_gru": (out["emb"], p.emb_num_layers - 1), "df_dec.df_gru": (out["emb"], p.df_num_layers)}
    # what the fused DF-encoder kernels, the decoder tail's matrix forms and erb_conv1 split (tests/test_fp16_range.py), and the pointwise convolutions' inputs
    co_in = O.conv_norm_act(out["e0"], sd, "erb_dec.conv0p", p.conv_ch, p.conv_ch, (1, 1)) + out["d1"]
    split_max = max(float(v.abs().max()) for v in (out["c0"], out["c1"], co_in, x[1], x[2], out["e0"], out["e1"], out["e2"], out["cemb"]))
    for prefix, (v, layers) in stacks.items():
        xl = lin(v, f"{prefix}.linear_in.0.weight")
        big, moves = [], []
        for l in range(layers):   # layer by layer, to see every layer's states
            one = {f"g.{n}_l0": sd[f"{prefix}.gru.{n}_l{l}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
            split_max = max(split_max, float(xl.abs().max()))   # the projection's operand (scaled per row before its split; bounded all the same)
            xl = O.gru_manual(xl, one, "g", 1)[0]
            big.append((xl.abs() > 0.9).double().mean().item())
            moves.append((xl[:, 1:] - xl[:, :-1]).std().item())
        share, move = min(big), min(moves)   # the least lively layer of the stack
        print(f"  {prefix}: share of |h| > 0.9 per layer {['%.2f' % b for b in big]}, std of h[t] - h[t-1] per layer {['%.2f' % s for s in moves]}")
        assert share >= 0.15 and move >= 0.1, (prefix, big, moves)
    print(f"  largest value an fp16-split kernel has to split: {split_max:.3g}")
    assert split_max < 6.0e4


@pytest.mark.parametrize("arith", ["fp16x3", "exact_fp32"])
def test_df3_against_float64_oracle(backend, arith, monkeypatch):
    """DeepFilterNet3 through DfNet.__call__ in the serial form of the GRU phase (37 frames are one chunk), default arithmetic and exact fp32."""
    ref = reference("df3", *((2, 19) if backend == "emu" else (3, 37)))
    _check_mutants(ref, "df3")
    model = _model(monkeypatch, ref, {"DFX_EXACT_FP32": "1"} if arith == "exact_fp32" else {})
    _check_kernel(ref, _forward(model, ref, "serial"), f"df3 [{backend}] serial {arith}")


@pytest.mark.gpu
@pytest.mark.parametrize("form,env", [("pair", {}), ("persistent", {"DFX_GRU_PAIR": "0"}), ("events", {"DFX_GRU_SEQ": "0"}),
                                      ("persistent", {"DFX_EXACT_FP32": "1"})], ids=["pair", "single_cu", "events", "exact_fp32"])
def test_df3_layer_pipelined_forms_against_float64_oracle(hip_backend, form, env, monkeypatch):
    """20 clips x 40 frames (tile 1 of the only pair partly live, several follower blocks) in short chunks: the persistent phase on a pair of CUs,
    on one CU per 16 clips, the event-synchronised form, and the exact fp32 persistent phase (which has no pair form)."""
    ref = reference("df3", 20, 40)
    _check_mutants(ref, "df3 20 x 40")
    model = _model(monkeypatch, ref, env, CHUNKED)
    _check_kernel(ref, _forward(model, ref, form), f"df3 20 x 40 [hip] {form} {'exact_fp32' if 'DFX_EXACT_FP32' in env else 'fp16x3'}")


LIVELY_SHAPES = ["l4_d3", "l5_d3", "l2_d1", "lg8", "e16", "c16_e16_f32_o6", "pf32", "df3_o10"]
EMU_SHAPE = "l2_d1"   # the one the interpreter runs: three GRU layers, the shortest stacks


def _shape_case(monkeypatch, backend, shape):
    """(3, 37) in the serial form (the default chunking) and, in short chunks, in the layer-pipelined form the backend takes: the persistent phase
    with this shape's followers on the GPU (3 clips: one CU per layer), the event-synchronised form on the interpreter."""
    ref = reference(shape, 3, 37)
    _check_mutants(ref, shape)
    _check_kernel(ref, _forward(_model(monkeypatch, ref, {}), ref, "serial"), f"{shape} [{backend}] serial fp16x3")
    form = "persistent" if backend == "hip" else "events"
    _check_kernel(ref, _forward(_model(monkeypatch, ref, {}, CHUNKED), ref, form), f"{shape} [{backend}] {form} fp16x3")


# every shape on the GPU, EMU_SHAPE on the interpreter too: the conftest's backend fixture, handed its parameter from here
@pytest.mark.parametrize("backend,shape", [pytest.param("hip", s, marks=pytest.mark.gpu) for s in LIVELY_SHAPES] + [("emu", EMU_SHAPE)],
                         indirect=["backend"])
def test_other_shapes_against_float64_oracle(backend, shape, monkeypatch):
    _shape_case(monkeypatch, backend, shape)
