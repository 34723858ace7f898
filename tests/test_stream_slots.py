"""Slots of a running DfStream (dfx_stream_reset_streams): a stream that is reset while the others run on behaves, from the next call,
like a stream of a freshly created handle — `delay_frames` hops of silence, then the enhancement of its own signal since the reset,
delayed — and no other stream notices.  The oracles are the ones of test_streaming.py / test_streaming_gated.py (the batch oracle, or
oracle/stream_oracle.py where the runtime and the batch path are different reference code: post filter, gating, channels), at their
tolerances, applied to the post-reset signal of the reset stream alone."""
import re

import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from oracle import stream_oracle as S
from tests.helpers import emu_subset, named_params, rms, torch_sd

HOP = 480
OPEN = (-1e9, 1e9, 1e9)   # thresholds with which no stage is ever skipped


def _fresh_stream_oracle(p, sd, sig):
    """What a fresh ungated stream answers to `sig` [T*hop]: enhance(pad=False) delayed by the lookahead — through libDF's own post filter
    where the model has one (the comparison test_stream_equals_batch_delayed makes at 1e-6 for such models)."""
    if p.mask_pf:
        return S.process_stream(p, sd, sig, pf_beta=p.pf_beta, thresholds=OPEN)[0]
    d = p.df_lookahead * HOP
    ref = O.enhance(p, sd, sig[None], pad=False)[0]
    return np.concatenate([np.zeros(d, np.float32), ref[: len(sig) - d]])


def _drive(rt, x, cuts, resets=None, lsnr=False):
    """Feeds x [rows, T*hop] cut into calls of `cuts` hops; resets: {hop index: ids} applied before the call that starts at that hop."""
    outs, ls, pos = [], [], 0
    for n in cuts:
        if resets and pos in resets:
            rt.reset(resets[pos])
        r = rt.process(torch.from_numpy(x[:, pos * HOP:(pos + n) * HOP]), return_lsnr=lsnr)
        outs.append(r[0] if lsnr else r)
        if lsnr:
            ls.append(r[1])
        pos += n
    assert pos * HOP == x.shape[1]
    y = torch.cat(outs, 1).numpy()
    return (y, torch.cat(ls, 1).numpy()) if lsnr else y


def _noise(rows, T, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal((rows, HOP * T))).astype(np.float32)


def _copy_launches(rt, x, cuts, resets=None):
    """_drive with the number of window-copy launches (dfx_k_copy_rows and the ring steps counted with it) of every call: what tells the
    forms of the windows apart (see test_reset_stream_equals_a_fresh_stream)."""
    from deepfilternet_amd import _lib

    outs, counts, pos = [], [], 0
    _lib.prof_enable(["dfx_k_copy_rows"])
    try:
        for n in cuts:
            if resets and pos in resets:
                rt.reset(resets[pos])
            _lib.prof_reset()
            outs.append(rt.process(torch.from_numpy(x[:, pos * HOP:(pos + n) * HOP])))
            counts.append(_lib.prof_read().get("dfx_k_copy_rows", (0.0, 0))[1])
            pos += n
    finally:
        _lib.prof_enable(None)
    return torch.cat(outs, 1).numpy(), counts


@pytest.mark.parametrize("mode", ["linear-wrap", "ring", "twice"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_reset_stream_equals_a_fresh_stream(backend, monkeypatch, name, mode):
    """One hop per call, stream 1 of three reset after hop t0 - 1 (well past the window of H + L hops).  linear-wrap: the linear windows go
    back to the front in the call that carries the reset stream's first hop (DFX_STREAM_LINEAR=6, read at every create: a wrap every few
    hops); ring: the ring form of the windows (DFX_STREAM_LINEAR=0); twice: a second reset of the same stream one hop after the first,
    while it is still in warm-up (models with less than two hops of lookahead run with two here).  The form is proven, not assumed: the
    ring form steps three windows in every call, the first call included; the linear form has extra copies in its first call and in the
    call in which the windows go back to the front, which must be call t0.  Streams 0 and 2 are bit-equal to the run without a reset;
    and the same comparison on that run shows that a missing reset is seen (more than 20 x the tolerance away)."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    if backend == "emu" and name != "pf32":
        pytest.skip("the interpreter is slow: it covers the conv_ch=32 model (kt=3); the GPU run covers all three")
    if emu_subset(backend) and mode != "linear-wrap":
        pytest.skip("interpreter subset: the wrapping linear windows run here, the other forms on the GPU (DFX_EMU_ALL=1 runs all)")
    p = named_params(name)
    if mode == "twice" and p.df_lookahead < 2:
        p.df_lookahead = p.conv_lookahead = 2                          # a warm-up long enough to be reset inside it
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    monkeypatch.setenv("DFX_STREAM_LINEAR", "0" if mode == "ring" else "6")
    d = p.df_lookahead
    # the window (dfx_stream_create): H history frames + L.  DFX_STREAM_LINEAR=6, one hop per call: slack max(6, H + L + 1), capacity
    # H + L + 1 + slack; call k appends at frame k + H + L, so call slack + 1 is the first that does not fit: the windows go back then
    H = max(2 + p.df_pathway_kernel_size_t - 1, p.df_order - 1 - d)
    t0 = max(6, H + d + 1) + 1
    T = t0 + ((6 if mode == "twice" else 5) if backend == "emu" else 12)
    x = _noise(3, T, 2)
    resets = {t0: [1]}
    start = t0
    if mode == "twice":
        resets[t0 + 1] = torch.tensor([1], dtype=torch.int32)
        start = t0 + 1
    y, counts = _copy_launches(DfStream(model, df_state, streams=3), x, [1] * T, resets)
    y_plain = _drive(DfStream(model, df_state, streams=3), x, [1] * T)
    print(f"{name}/{mode}: window-copy launches per call {counts}")
    if mode == "ring":
        assert counts == [3] * T, counts                              # spectra, ERB and DF feature rings, every call
    else:
        steady = counts[t0 - 1]
        assert counts[0] > 3                                           # the ring history moves into the linear buffer first
        assert counts[d + 1:t0] == [steady] * (t0 - d - 1) and counts[t0] > steady, counts   # ... which goes back to the front in call t0
        assert counts[t0 + 1:t0 + 6] == [steady] * len(counts[t0 + 1:t0 + 6]), counts
    ref = _fresh_stream_oracle(p, sd, x[1, start * HOP:])
    got = y[1, start * HOP:]
    if d:
        assert float(np.abs(got[: d * HOP]).max()) == 0.0            # the reset stream's next `delay_frames` hops are silence
    err = rms(got - ref)
    print(f"{name}/{mode}: reset stream vs fresh-stream oracle {err:.3e}; without the reset {rms(y_plain[1, start * HOP:] - ref):.3e}")
    assert err < 1e-6, err
    assert rms(y_plain[1, start * HOP:] - ref) > 20 * 1e-6             # the test can see a reset that did not happen
    assert np.array_equal(y[[0, 2]], y_plain[[0, 2]])                  # bystanders: the same bits
    assert np.array_equal(y[1, : t0 * HOP], y_plain[1, : t0 * HOP])
    model.check()


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_reset_before_a_call_of_several_hops(backend, name):
    """max_frames = 3, cuts [3, 1, 2, 3, ...], stream 1 reset in front of a 3-hop call (which the library may cut differently while the
    stream warms up): every stream within 1e-6 of its oracle, the bystanders within the bar of
    test_one_hop_kernels_agree_with_the_general_path of the run without the reset."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    if backend == "emu" and name != "pf32":
        pytest.skip("the interpreter is slow: it covers the conv_ch=32 model; the GPU run covers all three")
    if emu_subset(backend):
        pytest.skip("interpreter subset: one hop per call runs there (DFX_EMU_ALL=1 runs this too)")
    p = named_params(name)
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    cuts = [3, 1, 2, 3, 3, 1, 2] + ([] if backend == "emu" else [3, 2, 1, 3])
    t0, T = 9, sum(cuts)                                               # the fifth call: three hops
    x = _noise(3, T, 3)
    y = _drive(DfStream(model, df_state, streams=3, max_frames=3), x, cuts, {t0: [1]})
    y_plain = _drive(DfStream(model, df_state, streams=3, max_frames=3), x, cuts)
    for i in (0, 2):
        assert rms(y[i] - _fresh_stream_oracle(p, sd, x[i])) < 1e-6
        scale = float(np.sqrt((y_plain[i] ** 2).mean()))
        assert rms(y[i] - y_plain[i]) < 2e-6 * max(scale, 1e-3) + 1e-7
    ref = _fresh_stream_oracle(p, sd, x[1, t0 * HOP:])
    if p.df_lookahead:   # (a model without lookahead has no silent hops)
        assert float(np.abs(y[1, t0 * HOP:(t0 + p.df_lookahead) * HOP]).max()) == 0.0
    assert rms(y[1, t0 * HOP:] - ref) < 1e-6, rms(y[1, t0 * HOP:] - ref)
    assert rms(y_plain[1, t0 * HOP:] - ref) > 20 * 1e-6
    assert rms(y[1, : t0 * HOP] - _fresh_stream_oracle(p, sd, x[1, : t0 * HOP])) < 1e-6
    model.check()


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_reset_on_a_gated_handle(backend, name):
    """gating=True with thresholds inside the lsnr distribution (as test_streaming_gated.py takes them).  Stream 1 is digitally silent for
    the 8 hops before the reset — frozen, its counter above 5 — and starts over with noise: counter 0, flags clear, the DF decoder's delay
    line empty, i.e. oracle/stream_oracle.py on its post-reset signal (output 1e-6, lsnr 1e-3).  The others: the same bits as without."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream
    from tests.test_streaming_gated import _thresholds

    if backend == "emu" and name != "pf32":
        pytest.skip("the interpreter covers the conv_ch=32 model; the others run on the GPU")
    p = named_params(name)
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    t0 = 10
    T = t0 + (6 if backend == "emu" else 14)
    x = _noise(3, T, 2)
    x[1, (t0 - 8) * HOP: t0 * HOP] = 0
    x[2] *= np.linspace(0.01, 3, HOP * T).astype(np.float32)
    post = x[1, t0 * HOP:]
    # quantiles of test_streaming_gated.py's scenarios: the first set under which the oracle freezes the silent stream (a silent hop only
    # counts towards freezing while stage 1 is skipped; with the first set the conv_ch=16 model keeps running it on silence)
    for quantiles in ((0.15, 0.85, 0.5), (0.0, 0.3, 0.15)):
        thr = _thresholds(p, sd, [x[0], x[1], x[2], post], quantiles)
        before = S.process_stream(p, sd, x[1], thresholds=thr)[2]
        if t0 - 1 not in before["accepted"]:
            break
    assert t0 - 1 not in before["accepted"]                            # the stream is frozen when it is reset
    yr, lr, info = S.process_stream(p, sd, post, thresholds=thr)
    assert min(np.abs(np.asarray(info["lsnr_pass1"]) - t).min() for t in thr) > 1e-4    # robust decisions only
    y, lsnr = _drive(DfStream(model, df_state, streams=3, gating=True, thresholds=thr), x, [1] * T, {t0: [1]}, lsnr=True)
    y_plain, lsnr_plain = _drive(DfStream(model, df_state, streams=3, gating=True, thresholds=thr), x, [1] * T, lsnr=True)
    assert float(np.abs(y_plain[1, (t0 - 1) * HOP: t0 * HOP]).max()) == 0.0 and lsnr_plain[1, t0 - 1] == -15.0
    err = rms(y[1, t0 * HOP:] - yr)
    assert err < 1e-6, err
    n, d, acc = T - t0, p.df_lookahead, info["accepted"]
    live = np.zeros(n, bool)
    live[acc[d:]] = True                                               # hops that emitted a net position
    assert np.abs(lsnr[1, t0:] - lr)[live].max() < 1e-3
    frozen = np.ones(n, bool)
    frozen[acc] = False
    assert np.all(lsnr[1, t0:][frozen] == -15.0)
    assert np.array_equal(y[[0, 2]], y_plain[[0, 2]]) and np.array_equal(lsnr[[0, 2]], lsnr_plain[[0, 2]])
    assert np.array_equal(y[1, : t0 * HOP], y_plain[1, : t0 * HOP])
    model.check()


def test_reset_of_a_multichannel_stream(backend):
    """channels=2, four rows: reset([1]) resets rows 2 and 3 together (one reduced mask per stream: stream_oracle on the post-reset
    pair); rows 0 and 1 keep their bits."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    if emu_subset(backend):
        pytest.skip("interpreter subset: mono streams run there (DFX_EMU_ALL=1 runs this too)")
    p = named_params("pf32")
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    t0 = 7
    T = t0 + (5 if backend == "emu" else 12)
    x = _noise(4, T, 5)
    x[1] *= 0.3
    x[3] *= 0.5
    mk = lambda: DfStream(model, df_state, streams=4, channels=2, reduce_mask="mean")   # noqa: E731
    y = _drive(mk(), x, [1] * T, {t0: [1]})
    y_plain = _drive(mk(), x, [1] * T)
    ref = S.process_stream(p, sd, x[2:4, t0 * HOP:], thresholds=OPEN, reduce_mask="mean")[0]
    assert rms(y[2:4, t0 * HOP:] - ref) < 1e-6, rms(y[2:4, t0 * HOP:] - ref)
    assert rms(y_plain[2:4, t0 * HOP:] - ref) > 20 * 1e-6
    assert np.array_equal(y[:2], y_plain[:2])
    with pytest.raises(RuntimeError):
        mk().reset([2])                                                # two streams: the indices are 0 and 1


def test_ages_and_the_pass_through_setting(backend):
    """DfStream.frames: hops of network time per stream since its own last reset.  The pass-through setting of the attenuation limit
    does not advance them (as it does not advance the handle's count); a stream reset after such a stretch matches its oracle (the
    oracle has no mid-stream switch, so the reset that is checked comes after it); reset() without a list: all ages 0."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32")
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    n_after = 4 if backend == "emu" else 10
    T = 3 + 2 + 1 + n_after
    x = _noise(2, T, 7)
    rt = DfStream(model, df_state, streams=2)
    hop_at = lambda k: torch.from_numpy(x[:, k * HOP:(k + 1) * HOP])   # noqa: E731
    assert rt.frames.tolist() == [0, 0] and rt.frames.dtype == torch.int64
    for k in range(3):
        rt.process(hop_at(k))
    rt.reset([0])
    assert rt.frames.tolist() == [0, 3]
    for k in range(3, 5):
        rt.process(hop_at(k))
    assert rt.frames.tolist() == [2, 5]
    rt.set_atten_lim(0.0)
    assert torch.equal(rt.process(hop_at(5)), hop_at(5))
    assert rt.frames.tolist() == [2, 5]
    rt.set_atten_lim(100.0)
    rt.reset(torch.tensor([0]))
    y = torch.cat([rt.process(hop_at(k)) for k in range(6, T)], 1).numpy()
    assert rt.frames.tolist() == [n_after, 5 + n_after]
    ref = _fresh_stream_oracle(p, sd, x[0, 6 * HOP:])
    assert rms(y[0] - ref) < 1e-6, rms(y[0] - ref)
    rt.reset()
    assert rt.frames.tolist() == [0, 0]
    model.check()


def test_errors_and_the_empty_list(backend):
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32")
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    T = 4
    x = _noise(2, T, 8)
    rt = DfStream(model, df_state, streams=2)
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(_lib.DfxError) as e:
            rt.reset(bad)
        assert e.value.code == 1                                                        # DFX_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        rt.reset([0.5])
    import ctypes as C

    assert _lib.lib().dfx_stream_reset_streams(rt._h, None, 1, _lib.stream()) == 1      # DFX_ERR_INVALID_ARG: null list with count > 0
    assert _lib.lib().dfx_stream_reset_streams(rt._h, None, 0, _lib.stream()) == 0
    assert _lib.lib().dfx_stream_frames(rt._h, C.cast(None, C.POINTER(C.c_int64))) == 1
    y = _drive(rt, x, [1] * T, {2: []})                                                    # an empty list is a no-op
    y_plain = _drive(DfStream(model, df_state, streams=2), x, [1] * T)
    assert np.array_equal(y, y_plain)
    assert rt.frames.tolist() == [T, T]


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import os

    from deepfilternet_amd import _lib
    from deepfilternet_amd.build import build
    from tests.hipemu.build_emu import build as emu_build

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo, "include", "dfx.h")).read(), flags=re.S)
    for lib_path in (build(), emu_build()):
        lib = C.CDLL(lib_path)
        for name in ("dfx_stream_reset_streams", "dfx_stream_frames"):
            assert re.search(r"\b%s\s*\(" % name, header), name
            assert name in _lib.SIGNATURES and hasattr(lib, name), (name, lib_path)


@pytest.mark.gpu
def test_churn_at_full_size(hip_backend):
    """4096 streams of the released model, 40 hops; from the 10th hop on every call is preceded by the reset of a rotating group of 64
    streams.  8 reset streams (fixed seed; at least 2 of them reset more than once) against their oracles, 8 never-reset streams
    bit-equal to the run without churn."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("df3")
    sd = torch_sd(p, 12)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=12)
    B, T, first, group = 4096, 40, 9, 64
    # groups rotate through the first 1280 streams: 20 groups, so hops 29 .. 39 reset the groups of hops 9 .. 19 a second time
    pool = 20
    resets = {t: list(range(((t - first) % pool) * group, ((t - first) % pool + 1) * group)) for t in range(first, T)}
    rng = np.random.default_rng(21)
    twice = rng.choice(np.arange(0, 6 * group), 3, replace=False)             # reset at hop 9 + g and again at 29 + g (g < 6: hops to compare remain)
    once = rng.choice(np.arange(11 * group, pool * group), 5, replace=False)
    never = rng.choice(np.arange(pool * group, B), 8, replace=False)
    base = (0.1 * np.random.default_rng(22).standard_normal((64, HOP * T))).astype(np.float32)
    x = np.ascontiguousarray(np.tile(base, (B // 64, 1)))
    x *= np.linspace(0.5, 1.5, B, dtype=np.float32)[:, None]                  # every stream its own signal
    xd = torch.from_numpy(x).cuda()

    def run(with_resets):
        rt = DfStream(model, df_state, streams=B)
        out = []
        for t in range(T):
            if with_resets and t in resets:
                rt.reset(resets[t])
            out.append(rt.process(xd[:, t * HOP:(t + 1) * HOP]))
        return rt, torch.cat(out, 1)

    rt, y = run(True)
    _, y_plain = run(False)
    ages = rt.frames
    for s in list(twice) + list(once):
        last = max(t for t in resets if s in range(resets[t][0], resets[t][-1] + 1))
        n_resets = sum(1 for t in resets if resets[t][0] <= s <= resets[t][-1])
        assert n_resets == (2 if s in twice else 1)
        assert int(ages[s]) == T - last
        ref = _fresh_stream_oracle(p, sd, x[s, last * HOP:])
        got = y[s, last * HOP:].cpu().numpy()
        assert float(np.abs(got[: p.df_lookahead * HOP]).max()) == 0.0
        assert rms(got - ref) < 1e-6, (s, rms(got - ref))
    idx = torch.from_numpy(never).cuda()
    assert torch.equal(y[idx], y_plain[idx])
    assert all(int(ages[s]) == T for s in never)
    model.check()
