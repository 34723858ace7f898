"""Streaming in every engine configuration the batch path serves: exact fp32 arithmetic (DFX_EXACT_FP32=1: every contraction on fp32 matrix
ops, the GRU layers of a one-hop call on dfx_k_gru_step_x32, of a several-hop call on dfx_k_proj256 + dfx_k_gru_rec_x32 with the handle's state)
and mask-only models (init_df(mask_only=True): no DF stage).  The oracles are those of test_streaming.py / test_streaming_gated.py /
test_stream_slots.py / test_capi.py at their tolerances: the batch path of the same handle mode delayed by the lookahead (itself pinned to
the torch oracle), oracle/stream_oracle.py for the gated runtime, a fresh stream for a reset slot, DfStream for the C API.

The interpreter runs the small conv_ch=32 model without post filter and at most 9 hops (an exact one-hop pass is ~1500 fp32 matrix ops per
wave there); the GPU runs cover the other models and the kernel's edges."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from oracle import stream_oracle as S
from tests.helpers import named_params, rms, torch_sd
from tests.test_streaming_gated import _run as _run_gated
from tests.test_streaming_gated import _signals, _thresholds

HOP = 480
OPEN = (-1e9, 1e9, 1e9)        # thresholds with which no stage is ever skipped
CAPI_THRESHOLDS = (-15.0, 35.0, 35.0)


def _init(monkeypatch, exact, **kw):
    """init_df in the given arithmetic (the variable is read when the model is created, as in tests/test_fp16_range.py)."""
    from deepfilternet_amd.enhance import init_df

    monkeypatch.setenv("DFX_EXACT_FP32", "1" if exact else "0")
    model, df_state, _, _ = init_df(epoch="none", **kw)
    assert model.query(model.Q_EXACT_FP32) == (1 if exact else 0)
    return model, df_state


def _cut(rt, x, cuts):
    out, pos = [], 0
    for n in cuts:
        out.append(rt.process(x[:, pos * HOP:(pos + n) * HOP]).cpu())
        pos += n
    assert pos * HOP == x.shape[1]
    return torch.cat(out, dim=1)


def _noise(rows, T, seed):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal((rows, HOP * T))).astype(np.float32))


# ---- a. exact streaming == exact batch path, however the signal is cut
A_CUTS = ["ones", "lookahead+1", "mixed", "fours"]


def _a_cuts(kind, T, L):
    if kind == "ones":
        return [1] * T
    if kind == "lookahead+1":      # the first call carries the warm-up hops and ONE network hop: the one-hop form
        return [L + 1] + [1] * (T - L - 1)
    if kind == "mixed":
        return [3, 1, 5] if T == 9 else [3, 1, 5, 2, 1]
    return [4, 4, 1] if T == 9 else [4, 4, 4]


@pytest.mark.parametrize("kind", A_CUTS)
@pytest.mark.parametrize("name", ["pf32_nopf", "df3", "defaults"])
def test_exact_stream_equals_exact_batch_delayed(backend, monkeypatch, name, kind):
    from deepfilternet_amd.enhance import enhance
    from deepfilternet_amd.streaming import DfStream

    if backend == "emu" and name != "pf32_nopf":
        pytest.skip("the interpreter is slow: it covers the conv_ch=32 model (kt=3, lookahead 1); the GPU run covers all three")
    p = named_params(name)
    model, df_state = _init(monkeypatch, True, params=p, seed=9)
    T = 9 if backend == "emu" else 12
    x = _noise(3, T, 2)
    ref = enhance(model, df_state, x, pad=False)
    e_batch = rms(ref.numpy() - O.enhance(p, torch_sd(p, 9), x.numpy(), pad=False))
    print(f"{name}: exact batch path vs torch oracle {e_batch:.3e}")
    assert e_batch < 2e-6
    rt = DfStream(model, df_state, streams=3, max_frames=5)        # (refused before exact handles could stream)
    d = rt.delay_frames
    assert d == p.df_lookahead
    cuts = _a_cuts(kind, T, d)
    y = _cut(rt, x, cuts)
    assert y.shape == x.shape
    if d:
        assert float(y[:, : d * HOP].abs().max()) == 0.0             # warm-up hops are silence
    err = rms((y[:, d * HOP:] - ref[:, : (T - d) * HOP]).numpy())
    print(f"{name} {cuts}: exact streaming vs exact batch {err:.3e} (signal {rms(ref.numpy()):.3e})")
    assert err < 1e-6, (cuts, err)
    model.check()


# ---- b. the one-step kernel at its edges
@pytest.mark.gpu
@pytest.mark.parametrize("streams", [3, 130])
def test_exact_one_hop_kernel_agrees_with_the_general_path(hip_backend, monkeypatch, streams):
    """3 streams: one partial 16-row tile; 130: two 128-row blocks, the second with two live rows (clamped loads, unstored rows, the grid padded
    to 8 row blocks).  Single hops (dfx_k_gru_step_x32), calls of three hops (dfx_k_proj256 + dfx_k_gru_rec_x32) and a mixed cut agree
    within the bound of test_one_hop_kernels_agree_with_the_general_path."""
    from deepfilternet_amd.streaming import DfStream

    p = named_params("df3")
    model, df_state = _init(monkeypatch, True, params=p, seed=12)
    T = 48
    x = _noise(streams, T, 3).cuda()
    run = lambda cuts: _cut(DfStream(model, df_state, streams=streams, max_frames=3), x, cuts).numpy()   # noqa: E731
    ones = run([1] * T)
    threes = run([3] * (T // 3))
    mixed = run([1] * 9 + [2, 3, 1, 1, 1, 2] + [1] * (T - 19))
    scale = float(np.sqrt((ones ** 2).mean()))
    assert np.isfinite(ones).all() and float(np.abs(ones).max()) > 1e-4
    assert float(np.abs(ones[-1]).max()) > 1e-4                       # the last row (the second block's) was stored
    for tag, y in (("threes", threes), ("mixed", mixed)):
        print(f"{streams} streams, {tag}: {rms(y - ones):.3e} (scale {scale:.3e})")
        assert rms(y - ones) < 2e-6 * max(scale, 1e-3) + 1e-7, (tag, rms(y - ones), scale)
    model.check()


@pytest.mark.gpu
def test_exact_one_hop_kernel_with_64_unit_workgroups(hip_backend, monkeypatch):
    """The host gives a workgroup 64 hidden units (CT = 4) instead of 32 when such workgroups fill the chip: at 4096 streams the two decoders'
    stacks, which run side by side (32 row blocks x 4 unit blocks x 2 stacks = 256 = the MI355X's compute units); the encoder's layer keeps 32
    units there.  Reached by size, not by a switch: 4096 streams x 6 hops (df3: two warm-up hops), single hops against calls of three hops
    — whose first call carries one network hop (the one-hop form on the zero state), the second three (the general path)."""
    from deepfilternet_amd.streaming import DfStream

    p = named_params("df3")
    model, df_state = _init(monkeypatch, True, params=p, seed=12)
    streams, T = 4096, 6
    x = _noise(streams, T, 5).cuda()
    ones = _cut(DfStream(model, df_state, streams=streams, max_frames=3), x, [1] * T).numpy()
    threes = _cut(DfStream(model, df_state, streams=streams, max_frames=3), x, [3, 3]).numpy()
    scale = float(np.sqrt((ones ** 2).mean()))
    assert np.isfinite(ones).all() and float(np.abs(ones[:, 2 * HOP:]).max(axis=1).min()) > 1e-4      # every stream answered
    print(f"4096 streams: {rms(threes - ones):.3e} (scale {scale:.3e})")
    assert rms(threes - ones) < 2e-6 * max(scale, 1e-3) + 1e-7, (rms(threes - ones), scale)
    model.check()


# ---- c. the fused form really runs
def test_exact_one_hop_call_is_one_launch_per_gru_layer(backend, monkeypatch):
    """A steady one-hop call of an exact handle records what the fp16-split handle of the same model records: one launch per GRU layer in the
    recurrence scope and none in the projection scope.  A call of several hops records a projection and a recurrence per layer."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32_nopf")
    layers = 1 + (p.emb_num_layers - 1) + p.df_num_layers      # enc.emb_gru has one layer, the ERB decoder the rest of emb_num_layers
    x = _noise(3, p.df_lookahead + 4, 2)
    counts = {}
    for exact in (False, True):
        model, df_state = _init(monkeypatch, exact, params=p, seed=9)
        rt = DfStream(model, df_state, streams=3, max_frames=2)
        pos = 0
        for _ in range(p.df_lookahead + 1):                            # warm-up, then the first network hop
            rt.process(x[:, pos * HOP:(pos + 1) * HOP])
            pos += 1
        _lib.prof_enable(["dfx_k_gru_rec", "dfx_k_proj256"])
        try:
            got = []
            for n in (1, 2):
                _lib.prof_reset()
                rt.process(x[:, pos * HOP:(pos + n) * HOP])
                pos += n
                r = _lib.prof_read()
                got.append((r.get("dfx_k_gru_rec", (0.0, 0))[1], r.get("dfx_k_proj256", (0.0, 0))[1]))
        finally:
            _lib.prof_enable(None)
        counts[exact] = got
    print(f"(recurrence, projection) launches of a one-hop and a two-hop call: split {counts[False]}, exact {counts[True]}")
    assert counts[True][0] == counts[False][0] == (layers, 0)
    assert counts[True][1] == counts[False][1] == (layers, layers)


# ---- d. gating in exact mode
@pytest.mark.parametrize("name,T,cuts", [
    pytest.param("pf32_nopf", 24, [4] * 6, id="pf32_nopf"),      # kt = 3, lookahead 1
    pytest.param("df3", 30, [5] * 6, id="df3"),                  # kt = 5, lookahead 2, conv_ch 64
])
def test_exact_gated_stream_matches_oracle(backend, monkeypatch, name, T, cuts):
    """The comparison of test_gated_stream_matches_oracle (signals, thresholds inside the observed lsnr distribution, tolerances) on an exact
    handle: one hop per pass, every GRU layer on the one-step kernel, skipped decoders and frozen streams get the state of the other
    buffer back; df_convp reads the per-stream c0 window (the form of every handle without fp16-split fragments)."""
    from deepfilternet_amd.streaming import DfStream

    if backend == "emu" and name != "pf32_nopf":
        pytest.skip("the interpreter covers the conv_ch=32 model; df3 runs on the GPU")
    seed = 2
    if backend == "emu":
        T, cuts = 9, [3, 3, 3]
    p = named_params(name)
    sd = torch_sd(p, 9)
    x = _signals(T, seed)
    thr = _thresholds(p, sd, x, (0.15, 0.85, 0.5))
    ref = [S.process_stream(p, sd, xi, thresholds=thr) for xi in x]
    # conditions on the input, taken from the oracle's own decisions: at least two different stage outcomes, one frozen stretch, and no
    # lsnr within 1e-4 dB of a threshold
    seen = {f for r in ref for f in r[2]["flags"]}
    assert len(seen) >= 2, seen
    assert any(len(r[2]["accepted"]) < T for r in ref)
    for r in ref:
        v = np.asarray(r[2]["lsnr_pass1"])
        assert min(np.abs(v - t).min() for t in thr) > 1e-4
    model, df_state = _init(monkeypatch, True, params=p, seed=9)
    rt = DfStream(model, df_state, streams=3, max_frames=max(cuts), gating=True, thresholds=thr)
    y, lsnr = _run_gated(rt, x, cuts)
    d = p.df_lookahead
    for i, (yr, lr, info) in enumerate(ref):
        print(f"{name} stream {i}: {rms(y[i] - yr):.3e}, outcomes {sorted(set(info['flags']))}, accepted {len(info['accepted'])} of {T}")
        assert rms(y[i] - yr) < 1e-6, (i, rms(y[i] - yr))
        acc = info["accepted"]
        live = np.zeros(T, bool)
        live[acc[d:]] = True
        assert np.abs(lsnr[i] - lr)[live].max() < 1e-3
        frozen = np.ones(T, bool)
        frozen[acc] = False
        assert np.all(lsnr[i][frozen] == -15.0)
        assert np.all(y[i].reshape(T, HOP)[frozen] == 0.0)
    model.check()


def test_exact_process_raw_matches_oracle(backend, monkeypatch):
    """dfx_stream_process_raw on an exact handle against oracle.stream_oracle.process_raw_frames, as tests/test_capi.py checks the split one:
    stage 1 always, stage 2 for the lower half of the observed lsnr values."""
    from deepfilternet_amd.state_dict import random_state_dict
    from deepfilternet_amd.streaming import DfStream
    from oracle import libdf_oracle as L

    p = named_params("pf32_nopf")
    sd_np = random_state_dict(p, 9)
    sd = torch_sd(p, 9)
    K = 6 if backend == "emu" else 24
    rng = np.random.default_rng(11)
    x = (0.1 * rng.standard_normal((2, HOP * K))).astype(np.float32)
    x[1] *= np.linspace(0.02, 2.0, HOP * K).astype(np.float32)
    spec = L.DF(p.sr, p.fft_size, p.hop_size, p.nb_erb, p.min_nb_freqs).analysis(x)        # [2, K, F] complex64
    free = [S.process_raw_frames(p, sd, spec[i], thresholds=OPEN) for i in range(2)]
    vals = np.sort([r[0] for f in free for r in f if r[0] is not None])
    j = max(range(len(vals) // 2 - 2, len(vals) // 2 + 2), key=lambda i: vals[i + 1] - vals[i])
    thr = (-1e9, 1e9, float(vals[j] + vals[j + 1]) / 2)
    assert min(abs(v - thr[2]) for v in vals) > 1e-4
    ref = [S.process_raw_frames(p, sd, spec[i], thresholds=thr) for i in range(2)]
    assert any(r[2] is None and r[1] is not None for f in ref for r in f) and any(r[2] is not None for f in ref for r in f)
    model, df_state = _init(monkeypatch, True, params=p, state_dict=sd_np)
    rt = DfStream(model, df_state, streams=2, gating=True, thresholds=thr)
    for k in range(K):
        lsnr, gains, coefs, stages = rt.process_raw(torch.from_numpy(np.ascontiguousarray(spec[:, k])))
        for i in range(2):
            rl, rg, rc = ref[i][k]
            if rl is None:
                assert int(stages[i]) == 0 and float(lsnr[i]) == -15.0
                continue
            assert abs(float(lsnr[i]) - rl) < 1e-3
            assert bool(int(stages[i]) & 2) == (rg is not None) and bool(int(stages[i]) & 8) == (rc is not None)
            if rg is not None:
                assert np.abs(gains[i].numpy() - rg).max() < 1e-5
            if rc is not None:
                assert np.abs(coefs[i].numpy() - rc).max() < 1e-5
    model.check()


# ---- e. mask-only models
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("name", ["pf32_nopf", "df3"])
def test_mask_only_stream(backend, monkeypatch, name, exact):
    """init_df(mask_only=True): ungated, the stream equals enhance() of the mask-only model delayed; gated with thresholds that skip nothing
    it equals the oracle's "mask only on every hop" (its thresholds (-1e9, 1e9, -1e9): stage 1 always, stage 2 never); process_raw reports
    gains and never coefficients."""
    from deepfilternet_amd.enhance import enhance
    from deepfilternet_amd.streaming import DfStream
    from oracle import libdf_oracle as L

    if backend == "emu" and name != "pf32_nopf":
        pytest.skip("the interpreter covers the conv_ch=32 model; df3 runs on the GPU")
    p = named_params(name)
    sd = torch_sd(p, 9)
    model, df_state = _init(monkeypatch, exact, params=p, seed=9, mask_only=True)   # (refused before mask-only models could stream)
    T = 9 if backend == "emu" else 12
    x = _noise(3, T, 2)
    ref = enhance(model, df_state, x, pad=False)
    rt = DfStream(model, df_state, streams=3, max_frames=3)
    d = rt.delay_frames
    cuts = [1, 1, 1, 3, 1, 2] if T == 9 else [1, 1, 1, 3, 1, 2, 3]
    y = _cut(rt, x, cuts)
    if d:
        assert float(y[:, : d * HOP].abs().max()) == 0.0
    err = rms((y[:, d * HOP:] - ref[:, : (T - d) * HOP]).numpy())
    print(f"{name} mask-only ungated: {err:.3e}")
    assert err < 1e-6, err
    Tg = 5 if backend == "emu" else T
    rg = DfStream(model, df_state, streams=3, max_frames=2, gating=True, thresholds=OPEN)
    yg, _ = _run_gated(rg, x[:, : Tg * HOP].numpy(), [1] * Tg)
    for i in range(3):
        yr = S.process_stream(p, sd, x[i, : Tg * HOP].numpy(), thresholds=(-1e9, 1e9, -1e9))[0]
        print(f"{name} mask-only gated stream {i}: {rms(yg[i] - yr):.3e}")
        assert rms(yg[i] - yr) < 1e-6, (i, rms(yg[i] - yr))
    K = d + 2
    spec = L.DF(p.sr, p.fft_size, p.hop_size, p.nb_erb, p.min_nb_freqs).analysis(np.ascontiguousarray(x[:2, : K * HOP].numpy()))
    rr = DfStream(model, df_state, streams=2, gating=True, thresholds=OPEN)
    for k in range(K):
        lsnr, gains, coefs, stages = rr.process_raw(torch.from_numpy(np.ascontiguousarray(spec[:, k])))
        if k >= d:
            assert np.all(stages.numpy() == 2), stages                # gains present, never coefficients
            assert float(coefs.abs().max()) == 0.0 and float(gains.abs().max()) > 0.0
        else:
            assert np.all(stages.numpy() == 0)
    model.check()


# ---- f. slots of an exact handle
@pytest.mark.gpu
def test_exact_reset_stream_equals_a_fresh_stream(hip_backend, monkeypatch):
    """test_reset_stream_equals_a_fresh_stream on an exact df3 handle, one hop per call: stream 1 of three is reset mid-run (its warm-up hops
    zero the buffer the one-step kernel has just written); it then equals a fresh stream, the other two keep their bits."""
    from deepfilternet_amd.streaming import DfStream
    from tests.test_stream_slots import _drive, _fresh_stream_oracle

    p = named_params("df3")
    sd = torch_sd(p, 9)
    model, df_state = _init(monkeypatch, True, params=p, seed=9)
    d = p.df_lookahead
    H = max(2 + p.df_pathway_kernel_size_t - 1, p.df_order - 1 - d)
    t0 = max(6, H + d + 1) + 1
    T = t0 + 12
    x = (0.1 * np.random.default_rng(2).standard_normal((3, HOP * T))).astype(np.float32)
    y = _drive(DfStream(model, df_state, streams=3), x, [1] * T, {t0: [1]})
    y_plain = _drive(DfStream(model, df_state, streams=3), x, [1] * T)
    ref = _fresh_stream_oracle(p, sd, x[1, t0 * HOP:])
    got = y[1, t0 * HOP:]
    assert float(np.abs(got[: d * HOP]).max()) == 0.0
    err = rms(got - ref)
    print(f"exact df3: reset stream vs fresh-stream oracle {err:.3e}; without the reset {rms(y_plain[1, t0 * HOP:] - ref):.3e}")
    assert err < 1e-6, err
    assert rms(y_plain[1, t0 * HOP:] - ref) > 20 * 1e-6
    assert np.array_equal(y[[0, 2]], y_plain[[0, 2]])
    assert np.array_equal(y[1, : t0 * HOP], y_plain[1, : t0 * HOP])
    model.check()


# ---- g. the C API under DFX_EXACT_FP32=1
def test_df_capi_in_exact_mode(backend, monkeypatch, tmp_path):
    """df_create / df_process_frame / df_free on an exported .dfx with DFX_EXACT_FP32=1 in the environment: the bits of a one-stream DfStream
    on the same model in the same mode with the C API's settings (capi.rs:27-34: thresholds -15 / 35 / 35 dB, post filter off)."""
    from deepfilternet_amd import _lib, export_dfx
    from deepfilternet_amd.state_dict import random_state_dict
    from deepfilternet_amd.streaming import DfStream
    from tests.test_capi import _capi, _process

    p = named_params("pf32_nopf" if backend == "emu" else "df3")
    sd_np = random_state_dict(p, 9)
    path = export_dfx(str(tmp_path / "model.dfx"), params=p, state_dict=sd_np)
    T = 4 if backend == "emu" else 20
    x = (0.1 * np.random.default_rng(7).standard_normal(HOP * T)).astype(np.float32)
    model, df_state = _init(monkeypatch, True, params=p, state_dict=sd_np)          # (leaves DFX_EXACT_FP32=1 set for df_create)
    lib = _capi(C.CDLL(_lib.library_path()))
    st = lib.df_create(os.fsencode(path), 100.0, None)
    assert st, "df_create refused the model under DFX_EXACT_FP32=1"
    assert lib.df_get_frame_length(st) == HOP
    y, lsnr = _process(lib, st, x)
    lib.df_free(st)
    rt = DfStream(model, df_state, streams=1, gating=True, thresholds=CAPI_THRESHOLDS)
    rt.set_post_filter_beta(0.0)
    rt.set_atten_lim(100.0)
    outs = [rt.process(torch.from_numpy(x[None, k * HOP:(k + 1) * HOP]), return_lsnr=True) for k in range(T)]
    yr = torch.cat([o[0] for o in outs], 1).numpy()[0]
    lr = torch.cat([o[1] for o in outs], 1).numpy()[0]
    assert float(np.abs(yr).max()) > 1e-4
    assert np.array_equal(y, yr) and np.array_equal(lsnr, lr)
    model.check()
