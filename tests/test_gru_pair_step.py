"""The pair form's time step in two passes (csrc/dfx_gru_pair.h: clip tile 0's matrix operations, then clip tile 1's with tile 0's gate math issued
between them) against the two forms that do not share its code: the persistent phase with one CU per 16 clips (DFX_GRU_PAIR=0) and the
event-synchronised form with one launch per layer and time chunk (DFX_GRU_SEQ=0).  Identical samples are required.

Shapes: the smallest at which the reordered step can go wrong.  Clips 17 (tile 1 of the only pair has ONE live clip), 20 (tile 1 partly live), 48
(three 16-clip groups: the last pair's second half is empty); frames per clip 5 (fewer steps than a block of the emb follower), 17 (a full block of
the projection followers plus one step) and 40.  Sequences this short only take the layer-pipelined forms when the shortest chunk worth a launch is
lowered (DfNet.set_pipeline): every case asserts through DfNet.last_plan() / Q_GRU_PERSISTENT that the persistent phase really ran and through
Q_PASSES_PAIR that its recurrences ran on pairs of CUs (and, under DFX_GRU_PAIR=0 / DFX_GRU_SEQ=0, that they did not).

Weights: the seeded random ones, and tests/helpers.py lively_state_dict, under which the forms are compared where h actually moves and gates saturate
(tests/test_gru_precision.py ties each form to a float64 oracle under the same kind of weights)."""
import numpy as np
import pytest
import torch

from tests.helpers import lively_state_dict, named_params

HOP = 480
SWITCHES = ("DFX_GRU_SEQ", "DFX_EXACT_FP32", "DFX_GRU_PAIR", "DFX_GRU_PAIR_FAR")


def _run(monkeypatch, p, x, env, persistent, pair=False, state_dict=None):
    from deepfilternet_amd.enhance import enhance, init_df

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, df_state, _, _ = init_df(params=p, state_dict=state_dict, epoch="none", seed=4)   # (the switches are read when the handle is created; no state_dict: seeded random weights)
    model.set_pipeline(time_chunks=12, min_chunk_frames=2)
    before, before_pair = model.query(model.Q_PASSES_PERSISTENT), model.query(model.Q_PASSES_PAIR)
    ys = [enhance(model, df_state, x, pad=False).cpu() for _ in range(3)]
    model.check()
    plan = model.last_plan()
    assert plan["pipe"], plan
    assert plan["use_seq"] == persistent, plan
    assert model.query(model.Q_GRU_PERSISTENT) == int(persistent)
    assert model.query(model.Q_PASSES_PERSISTENT) - before == (3 if persistent else 0)
    assert model.query(model.Q_PASSES_PAIR) - before_pair == (3 if pair else 0)   # dfx_k_gru_seq_p2 ran / did not run
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    return ys[0]


# weights: "random" = init_df's seeded random_state_dict, under which the GRUs are almost idle (|h| <= 0.19); "lively" = tests/helpers.py
# lively_state_dict: h moves by tenths per step and gates saturate, so what a hand-over delivers a step late or to the wrong rows shows in the samples
@pytest.mark.gpu
@pytest.mark.parametrize("clips,frames,weights", [pytest.param(c, f, w, id=f"{c}-{f}" + ("" if w == "random" else "-lively"))
                                                  for w in ("random", "lively") for f in (5, 17, 40) for c in (17, 20, 48)])
def test_pair_step_gives_the_bits_of_the_other_forms(hip_backend, clips, frames, weights, monkeypatch):
    p = named_params("df3")
    sd = lively_state_dict(p, 4) if weights == "lively" else None
    x = torch.from_numpy((0.1 * np.random.default_rng(100 * clips + frames).standard_normal((clips, frames * HOP))).astype(np.float32)).cuda()
    y_pair = _run(monkeypatch, p, x, {}, True, pair=True, state_dict=sd)
    assert torch.isfinite(y_pair).all() and float(y_pair.abs().max()) > 0
    assert torch.equal(y_pair, _run(monkeypatch, p, x, {"DFX_GRU_PAIR": "0"}, True, state_dict=sd))
    assert torch.equal(y_pair, _run(monkeypatch, p, x, {"DFX_GRU_SEQ": "0"}, False, state_dict=sd))


@pytest.mark.gpu
def test_pair_step_with_agent_scope_hand_overs(hip_backend, monkeypatch):
    """DFX_GRU_PAIR_FAR=1: the hand-overs a pair takes whose halves sit on different XCDs."""
    p = named_params("df3")
    clips, frames = 20, 17
    x = torch.from_numpy((0.1 * np.random.default_rng(7).standard_normal((clips, frames * HOP))).astype(np.float32)).cuda()
    y_far = _run(monkeypatch, p, x, {"DFX_GRU_PAIR_FAR": "1"}, True, pair=True)
    assert torch.equal(y_far, _run(monkeypatch, p, x, {}, True, pair=True))
    assert torch.equal(y_far, _run(monkeypatch, p, x, {"DFX_GRU_PAIR": "0"}, True))


@pytest.mark.gpu
def test_exact_fp32_phase_on_one_cu_gives_the_bits_of_the_launch_form(hip_backend, monkeypatch):
    """DFX_EXACT_FP32=1: the persistent phase runs dfx_k_gru_seq_x32 (one CU per 16 clips: the exact mode has no pair form) fed by
    dfx_k_proj_follow_x32, whose hand-overs are those of csrc/dfx_gru_sync.h, against one launch per layer and time chunk.  20 clips x 17
    frames: a partly live second group, a full block of the projection followers plus one step."""
    p = named_params("df3")
    clips, frames = 20, 17
    x = torch.from_numpy((0.1 * np.random.default_rng(11).standard_normal((clips, frames * HOP))).astype(np.float32)).cuda()
    y_seq = _run(monkeypatch, p, x, {"DFX_EXACT_FP32": "1"}, True)   # the persistent phase ran, not on pairs
    assert torch.isfinite(y_seq).all() and float(y_seq.abs().max()) > 0
    assert torch.equal(y_seq, _run(monkeypatch, p, x, {"DFX_EXACT_FP32": "1", "DFX_GRU_SEQ": "0"}, False))   # neither ran
