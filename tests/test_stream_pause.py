"""Paused streams of a pausable DfStream (dfx_stream_set_pausable / dfx_stream_process_active): a stream that sits calls out behaves like a
stream that was never on a shared handle.  Its oracle is the oracle of the hops it DELIVERED, concatenated — _fresh_stream_oracle of
test_stream_slots.py or oracle/stream_oracle.py — compared with the concatenation of its outputs over the calls it took part in, at the
streaming tolerances of test_stream_slots.py / test_streaming_gated.py (output 1e-6 RMS, lsnr 1e-3 on robust decisions).  In a call it
sits out its rows are exact zeros and its lsnr NaN, and no other stream notices."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from oracle import stream_oracle as S
from tests.helpers import emu_subset, named_params, rms, torch_sd
from tests.test_stream_slots import OPEN, _fresh_stream_oracle

HOP = 480


def _noise(rows, T, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal((rows, HOP * T))).astype(np.float32)


def _window(p):
    """H (history frames of dfx_stream_create) and the lookahead L."""
    d = p.df_lookahead
    return max(2 + p.df_pathway_kernel_size_t - 1, p.df_order - 1 - d), d


def _masks(T, ns, paused):
    """paused: {stream: calls it sits out} -> one bool list per call."""
    return [[t not in paused.get(s, ()) for s in range(ns)] for t in range(T)]


def _run(rt, sig, cuts, masks, fill_seed=None, use_mask=True, resets=None, before=None):
    """Every stream owns a clock: stream s (ch rows) delivers its next n hops of sig [rows, *] in a call in which masks[call][s] holds; in
    the others its rows of x carry filler (zeros, or noise of fill_seed) and — with use_mask — the call pauses it: zeros and NaN come
    back.  Returns per stream the concatenated outputs [ch, hops * HOP] and lsnr [hops] of its active calls, and the hops it delivered."""
    rows = sig.shape[0]
    ns = len(masks[0])
    ch = rows // ns
    rng = np.random.default_rng(fill_seed) if fill_seed is not None else None
    pos, ys, ls = [0] * ns, [[] for _ in range(ns)], [[] for _ in range(ns)]
    for c, (n, m) in enumerate(zip(cuts, masks)):
        if resets and c in resets:
            rt.reset(resets[c])
        if before and c in before:
            before[c]()
        x = np.zeros((rows, n * HOP), np.float32)
        for s in range(ns):
            r = slice(s * ch, (s + 1) * ch)
            if m[s]:
                x[r] = sig[r, pos[s] * HOP:(pos[s] + n) * HOP]
            elif rng is not None:
                x[r] = 0.1 * rng.standard_normal((ch, n * HOP))
        y, l = rt.process(torch.from_numpy(x), return_lsnr=True, active=m if use_mask else None)
        y, l = y.cpu().numpy(), l.cpu().numpy()
        for s in range(ns):
            r = slice(s * ch, (s + 1) * ch)
            if m[s]:
                ys[s].append(y[r])
                ls[s].append(l[s * ch])
                pos[s] += n
            elif use_mask:
                assert float(np.abs(y[r]).max()) == 0.0 and np.isnan(l[r]).all(), (c, s)     # exact zeros, no estimate
    return [np.concatenate(v, 1) for v in ys], [np.concatenate(v) for v in ls], pos


def _models(backend, name):
    if backend == "emu" and name != "pf32":
        pytest.skip("the interpreter is slow: it covers the conv_ch=32 model (kt=3); the GPU run covers all three")


@pytest.mark.parametrize("linear", ["0", "6"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_resume_where_it_stopped(backend, monkeypatch, name, linear):
    """Three streams, one hop per call.  Stream 0 never pauses; stream 1 pauses in three separate stretches, one of them the call in which
    the linear windows go back to the front (DFX_STREAM_LINEAR=6; =0: the ring form); stream 2 pauses from call 0 on and again later.
    The same schedule without masks on a plain handle — the filler processed — is far from the oracle: the test sees a missing pause."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    _models(backend, name)
    if emu_subset(backend) and linear == "0":
        pytest.skip("interpreter subset: the wrapping linear windows run here, the ring form on the GPU (DFX_EMU_ALL=1 runs both)")
    p = named_params(name)
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    monkeypatch.setenv("DFX_STREAM_LINEAR", linear)
    H, d = _window(p)
    t0 = max(6, H + d + 1) + 1                                          # the call in which the windows go back (test_stream_slots.py)
    T = t0 + 5 if backend == "emu" else H + d + 13
    assert T > t0 + 3
    paused = {1: {2, 3, t0, t0 + 2}, 2: {0, 1, 5, t0 + 1}}
    masks = _masks(T, 3, paused)
    sig = _noise(3, T, 2)
    rt = DfStream(model, df_state, streams=3, pausable=True)
    ys, _, pos = _run(rt, sig, [1] * T, masks, fill_seed=5)
    assert pos == [T, T - 4, T - 4] and rt.frames.tolist() == pos
    yp, _, _ = _run(DfStream(model, df_state, streams=3), sig, [1] * T, masks, fill_seed=5, use_mask=False)
    for s in range(3):
        ref = _fresh_stream_oracle(p, sd, sig[s, : pos[s] * HOP])
        err, err_plain = rms(ys[s][0] - ref), rms(yp[s][0] - ref)
        print(f"{name}/linear={linear}: stream {s} vs its oracle {err:.3e}; the filler processed instead {err_plain:.3e}")
        assert err < 1e-6, (s, err)
        if s:
            assert err_plain > 20 * 1e-6
    model.check()


def test_bystanders_keep_their_bits(backend):
    """Every call pauses someone; the two runs differ in who (streams 1 and 2) and in the filler of the paused rows: stream 0 — same bits."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32")
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    T = 8 if backend == "emu" else 16
    sig = _noise(3, T, 3)
    a = _masks(T, 3, {1: set(range(0, T, 2)), 2: set(range(1, T, 2))})
    b = _masks(T, 3, {1: set(range(1, T, 3)) | {0}, 2: set(range(T)) - set(range(1, T, 3)) - {0}})
    assert all(not all(m) for m in a + b)
    ya, la, _ = _run(DfStream(model, df_state, streams=3, pausable=True), sig, [1] * T, a, fill_seed=1)
    yb, lb, _ = _run(DfStream(model, df_state, streams=3, pausable=True), sig, [1] * T, b, fill_seed=2)
    assert np.array_equal(ya[0], yb[0]) and np.array_equal(la[0], lb[0])
    assert float(np.abs(ya[0]).max()) > 0
    model.check()


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_several_hops_per_call(backend, name):
    """max_frames=3, cuts [3, 1, 2, 3, 3, 1, 2, ...], another mask in every call: the mask holds for all hops of its call."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    _models(backend, name)
    if emu_subset(backend):
        pytest.skip("interpreter subset: one hop per call runs there (DFX_EMU_ALL=1 runs this too)")
    p = named_params(name)
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    cuts = [3, 1, 2, 3, 3, 1, 2] + ([] if backend == "emu" else [3, 2, 1, 3])
    masks = _masks(len(cuts), 3, {1: {1, 2, 5}, 2: {0, 4, 6}})
    sig = _noise(3, sum(cuts), 3)
    rt = DfStream(model, df_state, streams=3, max_frames=3, pausable=True)
    ys, _, pos = _run(rt, sig, cuts, masks, fill_seed=4)
    assert rt.frames.tolist() == pos and pos[1] < pos[0] > pos[2]
    for s in range(3):
        err = rms(ys[s][0] - _fresh_stream_oracle(p, sd, sig[s, : pos[s] * HOP]))
        assert err < 1e-6, (s, err)
    model.check()


@pytest.mark.parametrize("case", ["reserved-slot", "inside-warm-up", "inside-window"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_pause_and_reset(backend, name, case):
    """Two hops of lookahead.  reset([1]) before call t0, then — reserved-slot: three paused calls, then active; inside-warm-up: one active
    hop, two paused calls, then active; inside-window: L + 1 active hops, two paused calls (the stream is younger than H + L), then active.
    The stream's first delay_frames active hops are silence, then it follows the oracle of its post-reset delivered hops; the others have
    the bits of the same run without that reset."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    _models(backend, name)
    if emu_subset(backend) and case == "inside-window":
        pytest.skip("interpreter subset: the pauses around the warm-up run here, this one on the GPU (DFX_EMU_ALL=1 runs all)")
    p = named_params(name)
    if p.df_lookahead < 2:
        p.df_lookahead = p.conv_lookahead = 2
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    H, d = _window(p)
    t0 = H + d + 2                                                      # stream 1 is past its window when it is reset
    T = t0 + (7 if backend == "emu" else 14)
    lead = {"reserved-slot": 0, "inside-warm-up": 1, "inside-window": d + 1}[case]
    gap = 3 if case == "reserved-slot" else 2
    paused = {1: set(range(t0 + lead, t0 + lead + gap)), 2: {3, t0 + 1}}
    masks = _masks(T, 3, paused)
    sig = _noise(3, T, 6)
    rt = DfStream(model, df_state, streams=3, pausable=True)
    ys, _, pos = _run(rt, sig, [1] * T, masks, resets={t0: [1]})
    yp, _, _ = _run(DfStream(model, df_state, streams=3, pausable=True), sig, [1] * T, masks)
    assert rt.frames.tolist() == [T, T - t0 - gap, T - 2]
    got = ys[1][0, t0 * HOP:]                                           # (stream 1 took part in every call before t0)
    assert float(np.abs(got[: d * HOP]).max()) == 0.0
    ref = _fresh_stream_oracle(p, sd, sig[1, t0 * HOP: pos[1] * HOP])
    err = rms(got - ref)
    print(f"{name}/{case}: reset and paused stream vs its oracle {err:.3e}; without the reset {rms(yp[1][0, t0 * HOP:] - ref):.3e}")
    assert err < 1e-6, err
    assert rms(yp[1][0, t0 * HOP:] - ref) > 20 * 1e-6
    assert np.array_equal(ys[0], yp[0]) and np.array_equal(ys[2], yp[2])
    assert np.array_equal(ys[1][0, : t0 * HOP], yp[1][0, : t0 * HOP])
    model.check()


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_pause_on_a_gated_handle(backend, name):
    """gating=True, thresholds inside the lsnr distribution.  Stream 1 delivers k hops of noise, 7 silent hops and noise again, and sits out
    six calls after the third silent hop: it freezes on the hop on which the oracle freezes its delivered signal (a pause that counted as
    silence would freeze it earlier, one that cleared the counter later).  Stream 2 (a ramp: every stage decision occurs) sits out two
    calls right after its first net positions, its DF decoder's delay line partly filled, and again later."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream
    from tests.test_streaming_gated import _thresholds

    _models(backend, name)
    p = named_params(name)
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    d = p.df_lookahead
    k = d + 3
    n_del = k + 7 + (2 if backend == "emu" else 6)                      # hops stream 1 delivers
    T = n_del + 6
    sig = _noise(3, T, 2)
    sig[1, k * HOP:(k + 7) * HOP] = 0
    sig[2] *= np.linspace(0.01, 3, HOP * T).astype(np.float32)
    paused = {1: set(range(k + 3, k + 9)), 2: {d + 1, d + 2, k + 4}}
    masks = _masks(T, 3, paused)
    n2 = T - 3
    for quantiles in ((0.15, 0.85, 0.5), (0.0, 0.3, 0.15)):            # (as in test_reset_on_a_gated_handle: the first set that freezes)
        thr = _thresholds(p, sd, [sig[0], sig[1, : n_del * HOP], sig[2, : n2 * HOP]], quantiles)
        if k + 6 not in S.process_stream(p, sd, sig[1, : n_del * HOP], thresholds=thr)[2]["accepted"]:
            break
    rt = DfStream(model, df_state, streams=3, gating=True, thresholds=thr, pausable=True)
    ys, ls, pos = _run(rt, sig, [1] * T, masks, fill_seed=8)
    assert pos == [T, n_del, n2] and rt.frames.tolist() == pos
    for s in range(3):
        yr, lr, info = S.process_stream(p, sd, sig[s, : pos[s] * HOP], thresholds=thr)
        assert min(np.abs(np.asarray(info["lsnr_pass1"]) - t).min() for t in thr) > 1e-4    # robust decisions only
        acc = info["accepted"]
        frozen = np.ones(pos[s], bool)
        frozen[acc] = False
        if s == 1:
            assert frozen[k + 6] and not frozen[: k + 1].any() and not frozen[k + 7:].any()   # frozen inside the silence, where the oracle says
        err = rms(ys[s][0] - yr)
        print(f"{name}: gated stream {s} vs oracle {err:.3e}; frozen hops {np.flatnonzero(frozen).tolist()}")
        assert err < 1e-6, (s, err)
        live = np.zeros(pos[s], bool)
        live[acc[d:]] = True                                           # hops that emitted a net position
        assert np.abs(ls[s] - lr)[live].max() < 1e-3
        assert np.all(ls[s][frozen] == -15.0)
        assert float(np.abs(ys[s][0].reshape(-1, HOP)[frozen]).max(initial=0.0)) == 0.0
    model.check()


def test_pause_of_a_multichannel_stream(backend):
    """channels=2, four rows, a mask of two entries: rows 2 and 3 pause as one stream; rows 0 and 1 keep their bits whatever stream 1 does."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    if emu_subset(backend):
        pytest.skip("interpreter subset: mono streams run there (DFX_EMU_ALL=1 runs this too)")
    p = named_params("pf32")
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    T = 9 if backend == "emu" else 16
    sig = _noise(4, T, 5)
    sig[1] *= 0.3
    sig[3] *= 0.5
    mk = lambda: DfStream(model, df_state, streams=4, channels=2, reduce_mask="mean", pausable=True)   # noqa: E731
    rt = mk()
    ya, _, pa = _run(rt, sig, [1] * T, _masks(T, 2, {1: {0, 3, 4, 7}}), fill_seed=1)
    yb, _, pb = _run(mk(), sig, [1] * T, _masks(T, 2, {1: {2, 5}}), fill_seed=2)
    assert rt.frames.tolist() == [T, T - 4]
    for y, pos in ((ya, pa), (yb, pb)):
        ref = S.process_stream(p, sd, sig[2:4, : pos[1] * HOP], thresholds=OPEN, reduce_mask="mean")[0]
        assert rms(y[1] - ref) < 1e-6, rms(y[1] - ref)
    assert np.array_equal(ya[0], yb[0])
    with pytest.raises(ValueError):
        mk().process(torch.from_numpy(sig[:, :HOP]), active=[True] * 4)


@pytest.mark.parametrize("mode", ["exact", "mask-only"])
def test_pause_in_the_other_engine_configurations(backend, monkeypatch, mode):
    """A DFX_EXACT_FP32=1 model and a mask-only model, as tests/test_stream_modes.py runs them: the oracle is the model's own batch path on
    the delivered hops, delayed (what that file compares an unpaused stream with at 1e-6)."""
    from deepfilternet_amd.enhance import enhance
    from deepfilternet_amd.streaming import DfStream
    from tests.test_stream_modes import _init

    p = named_params("pf32_nopf")
    model, df_state = _init(monkeypatch, mode == "exact", params=p, seed=9, mask_only=mode == "mask-only")
    d = p.df_lookahead
    T = 9 if backend == "emu" else 14
    sig = _noise(3, T, 2)
    rt = DfStream(model, df_state, streams=3, pausable=True)
    ys, _, pos = _run(rt, sig, [1] * T, _masks(T, 3, {1: {1, 4, 5}, 2: {0, 6}}), fill_seed=3)
    assert rt.frames.tolist() == pos
    for s in range(3):
        x = torch.from_numpy(sig[s: s + 1, : pos[s] * HOP])
        ref = enhance(model, df_state, x, pad=False)[0].numpy()
        assert float(np.abs(ys[s][0, : d * HOP]).max()) == 0.0
        err = rms(ys[s][0, d * HOP:] - ref[: (pos[s] - d) * HOP])
        print(f"{mode}: stream {s} vs its own batch path on the delivered hops {err:.3e}")
        assert err < 1e-6, (s, err)
    model.check()


def test_pause_and_the_pass_through_setting(backend):
    """set_atten_lim(0): active rows return their input bit for bit, paused rows zeros (and NaN), and nobody ages; back at 100 dB and after
    a reset of all streams the handle follows its oracles again, pauses included."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32")
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    n_after = 5 if backend == "emu" else 10
    x = _noise(2, 3 + 2 + n_after, 7)
    hop_at = lambda k: torch.from_numpy(x[:, k * HOP:(k + 1) * HOP])   # noqa: E731
    rt = DfStream(model, df_state, streams=2, pausable=True)
    for k in range(3):
        rt.process(hop_at(k), active=[True, k != 1])
    assert rt.frames.tolist() == [3, 2]
    rt.set_atten_lim(0.0)
    for k in (3, 4):
        y, lsnr = rt.process(hop_at(k), return_lsnr=True, active=[k == 3, k == 4])
        a = k - 3
        assert torch.equal(y[a], hop_at(k)[a]) and float(lsnr[a]) == 35.0
        assert float(y[1 - a].abs().max()) == 0.0 and bool(torch.isnan(lsnr[1 - a]).all())
        assert rt.frames.tolist() == [3, 2]
    rt.set_atten_lim(100.0)
    rt.reset([0, 1])
    assert rt.frames.tolist() == [0, 0]
    ys, _, pos = _run(rt, x[:, 5 * HOP:], [1] * n_after, _masks(n_after, 2, {1: {1, 2}}))
    assert rt.frames.tolist() == pos == [n_after, n_after - 2]
    for s in range(2):
        err = rms(ys[s][0] - _fresh_stream_oracle(p, sd, x[s, 5 * HOP:(5 + pos[s]) * HOP]))
        assert err < 1e-6, (s, err)
    model.check()


def test_edges_and_errors(backend):
    from deepfilternet_amd import _lib
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32")
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    T = 4
    x = _noise(2, T, 8)
    hop_at = lambda k: torch.from_numpy(x[:, k * HOP:(k + 1) * HOP])   # noqa: E731
    ra, rb = DfStream(model, df_state, streams=2, pausable=True), DfStream(model, df_state, streams=2, pausable=True)
    for k in range(T):                                                  # an all-true mask is the call without a mask
        ya, la = ra.process(hop_at(k), return_lsnr=True, active=torch.tensor([1, 1], dtype=torch.int32))
        yb, lb = rb.process(hop_at(k), return_lsnr=True)
        assert torch.equal(ya, yb) and torch.equal(la, lb)
    assert float(ya.abs().max()) > 0
    y, lsnr = ra.process(hop_at(0), return_lsnr=True, active=[False, False])   # everybody sits out: nothing moves
    assert float(y.abs().max()) == 0.0 and bool(torch.isnan(lsnr).all()) and ra.frames.tolist() == [T, T]
    ya, yb = ra.process(hop_at(1)), rb.process(hop_at(1))
    assert torch.equal(ya, yb)
    with pytest.raises(ValueError):
        ra.process(hop_at(0), active=[True])
    with pytest.raises(TypeError):
        ra.process(hop_at(0), active=[1.0, 0.0])
    plain = DfStream(model, df_state, streams=2)
    with pytest.raises(_lib.DfxError) as e:
        plain.process(hop_at(0), active=[True, True])
    assert e.value.code == 1                                            # DFX_ERR_INVALID_ARG: a mask on a handle that is not pausable
    lib = _lib.lib()
    assert lib.dfx_stream_set_pausable(plain._h, 1) == 0                # nothing consumed yet (the refused call does not count)
    plain.process(hop_at(0), active=[True, False])
    assert lib.dfx_stream_set_pausable(plain._h, 0) == 1                # a hop was consumed
    plain.reset()
    assert lib.dfx_stream_set_pausable(plain._h, 0) == 0
    assert lib.dfx_stream_set_pausable(None, 1) == 1
    one = torch.zeros(2, dtype=torch.uint8)
    xd = hop_at(0).to(_lib.device()).contiguous()
    yd = torch.empty_like(xd)
    args = lambda h, xp, n, yp: lib.dfx_stream_process_active(h, xp, n, yp, None, C.c_void_p(one.data_ptr()), _lib.stream())   # noqa: E731
    assert args(None, _lib.ptr(xd), 1, _lib.ptr(yd)) == 1
    assert args(ra._h, None, 1, _lib.ptr(yd)) == 1
    assert args(ra._h, _lib.ptr(xd), 1, None) == 1
    assert args(ra._h, _lib.ptr(xd), 0, _lib.ptr(yd)) == 1
    assert args(ra._h, _lib.ptr(xd), 2, _lib.ptr(yd)) == 1             # max_frames = 1
    model.check()


def test_new_symbols_are_declared_bound_and_exported():
    import os

    from deepfilternet_amd import _lib
    from deepfilternet_amd.build import build
    from tests.hipemu.build_emu import build as emu_build

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo, "include", "dfx.h")).read(), flags=re.S)
    for lib_path in (build(), emu_build()):
        lib = C.CDLL(lib_path)
        for name in ("dfx_stream_set_pausable", "dfx_stream_process_active"):
            assert re.search(r"\b%s\s*\(" % name, header), name
            assert name in _lib.SIGNATURES and hasattr(lib, name), (name, lib_path)


MASK_LAUNCH = 4096   # streams whose mask bits one launch of dfx_k_stream_pause carries (DFX_PAUSE_STREAMS)


@pytest.mark.gpu
@pytest.mark.parametrize("streams,T,pauses,check,gating", [
    (70, 12, {15: {0, 4}, 16: {1, 2, 3}, 63: {5, 9}, 64: {5, 6}, 69: {0, 11}}, None, True),
    (MASK_LAUNCH + 1, 8, {MASK_LAUNCH - 1: {2, 3}, MASK_LAUNCH: {0, 5, 6}, 31: {4}}, (31, MASK_LAUNCH - 1, MASK_LAUNCH), False),
])
def test_row_group_boundaries(hip_backend, streams, T, pauses, check, gating):
    """Pauses on both sides of the 16-row groups of the silent-input kernel and of the 32-bit words of the mask (70 streams, every row
    checked; gating on with thresholds that skip nothing, so that dfx_k_gate_pre_lds runs and the oracle stays the ungated one), and one
    stream more than a launch of the mask kernel carries (three rows checked)."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("pf32")
    sd = torch_sd(p, 9)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    base = _noise(70, T, 11)
    sig = np.ascontiguousarray(np.tile(base, (-(-streams // 70), 1))[:streams])
    sig *= np.linspace(0.5, 1.5, streams, dtype=np.float32)[:, None]
    xd = torch.from_numpy(sig).cuda()
    rt = DfStream(model, df_state, streams=streams, pausable=True, gating=gating, thresholds=OPEN if gating else None)
    pos = np.zeros(streams, np.int64)
    rows = torch.arange(streams).cuda()
    out = torch.zeros_like(xd)
    for t in range(T):
        active = np.ones(streams, bool)
        for s, calls in pauses.items():
            active[s] = t not in calls
        at = torch.from_numpy(pos).cuda()
        x = torch.gather(xd.view(streams, T, HOP), 1, at.view(-1, 1, 1).expand(-1, 1, HOP))[:, 0]     # every stream's next hop
        y = rt.process(x, active=active)
        act = torch.from_numpy(active).cuda()
        assert active.all() or float(y[~act].abs().max()) == 0.0
        out.view(streams, T, HOP)[rows[act], at[act]] = y[act]
        pos += active
    assert rt.frames.tolist() == pos.tolist()
    out = out.cpu().numpy()
    for s in (range(streams) if check is None else check):
        err = rms(out[s, : pos[s] * HOP] - _fresh_stream_oracle(p, sd, sig[s, : pos[s] * HOP]))
        assert err < 1e-6, (s, err)
    model.check()


@pytest.mark.gpu
def test_jitter_at_full_size(hip_backend):
    """4096 streams of the released model, 40 hops; from hop 5 on every call pauses a pseudo-random tenth of the streams (fixed seed).
    Eight streams with at least three pauses each — 63, 64 and 4095 among them — against their oracles and ages; eight others bit-equal to
    a second run in which only the other streams' pauses differ."""
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.streaming import DfStream

    p = named_params("df3")
    sd = torch_sd(p, 12)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=12)
    B, T, first = 4096, 40, 5
    rng = np.random.default_rng(1)
    active = np.ones((2, T, B), bool)
    active[0, first:] = rng.random((T - first, B)) >= 0.1
    active[1, first:] = rng.random((T - first, B)) >= 0.1
    often = np.flatnonzero((~active[0]).sum(0) >= 3)
    assert {63, 64, 4095} <= set(often.tolist())                        # (what the seed was picked for)
    checked = [63, 64, 4095] + [int(s) for s in often if s not in (63, 64, 4095)][:5]
    same = rng.choice(np.setdiff1d(np.arange(B), checked), 8, replace=False)
    active[1][:, same] = active[0][:, same]                             # these keep their own schedule; everybody else's differs
    base = (0.1 * np.random.default_rng(22).standard_normal((64, HOP * T))).astype(np.float32)
    sig = np.ascontiguousarray(np.tile(base, (B // 64, 1)))
    sig *= np.linspace(0.5, 1.5, B, dtype=np.float32)[:, None]
    xd = torch.from_numpy(sig).cuda().view(B, T, HOP)
    rows = torch.arange(B).cuda()

    def run(act_all):
        rt = DfStream(model, df_state, streams=B, pausable=True)
        pos = torch.zeros(B, dtype=torch.int64).cuda()
        out = torch.zeros(B, T, HOP).cuda()
        for t in range(T):
            x = torch.gather(xd, 1, pos.clamp(max=T - 1).view(-1, 1, 1).expand(-1, 1, HOP))[:, 0]
            y = rt.process(x, active=act_all[t])
            act = torch.from_numpy(act_all[t]).cuda()
            out[rows[act], pos[act]] = y[act]
            pos += act
        return rt, out.view(B, -1), pos.cpu().numpy()

    rt, y, pos = run(active[0])
    _, y2, pos2 = run(active[1])
    ages = rt.frames.numpy()
    assert np.array_equal(ages, pos) and np.array_equal(pos, active[0].sum(0))
    for s in checked:
        n = int(pos[s])
        assert n <= T - 3
        err = rms(y[s, : n * HOP].cpu().numpy() - _fresh_stream_oracle(p, sd, sig[s, : n * HOP]))
        assert err < 1e-6, (s, err)
    idx = torch.from_numpy(same).cuda()
    assert torch.equal(y[idx], y2[idx]) and np.array_equal(pos[same], pos2[same])
    assert not np.array_equal(pos, pos2)
    model.check()
