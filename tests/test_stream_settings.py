"""Settings that belong to one stream of a DfStream (dfx_stream_set_atten_lim_streams / _post_filter_beta_streams / _thresholds_streams,
``DfStream.set_*(..., streams=ids)``): in the reference the attenuation limit, the post-filter beta and the thresholds are properties of one
DfTract, i.e. of one caller (capi.rs:136-156, tract.rs:160-170).  Every stream of a handle with per-stream settings must behave like that
stream of a handle that was given the same values handle-wide — to the bit — and like oracle/stream_oracle.py with those values, at the bar
tests/test_stream_pause.py holds the runtime to (1e-6 RMS); streams whose settings were not touched keep their bits."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import stream_oracle as S
from tests.helpers import emu_subset, named_params, rms, torch_sd
from tests.test_stream_slots import OPEN, _fresh_stream_oracle, _noise
from tests.test_streaming_gated import _thresholds

HOP = 480
BAR = 1e-6            # RMS against the oracle (tests/test_stream_pause.py)
SET_IDS = 192         # streams per launch of the setter kernel (DFX_SET_IDS)
NEW = ("dfx_stream_set_atten_lim_streams", "dfx_stream_set_post_filter_beta_streams", "dfx_stream_set_thresholds_streams",
       "dfx_stream_get_settings")


def _setup(backend, name):
    from deepfilternet_amd.enhance import init_df

    if backend == "emu" and name != "pf32":
        pytest.skip("the interpreter covers the conv_ch=32 model (kt=3, lookahead 1, post filter); the GPU run covers all three")
    p = named_params(name)
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    return p, model, df_state


@functools.lru_cache(maxsize=None)
def _sd(name):
    return torch_sd(named_params(name), 9)


def _window(p):
    """H + L of dfx_stream_create: the hops after which a stream is past its start."""
    return max(2 + p.df_pathway_kernel_size_t - 1, p.df_order - 1 - p.df_lookahead) + p.df_lookahead


def _hops(p, backend, emu=6):
    """Hops of a run: past the window by 13 on the GPU, by at most 6 on the interpreter (which takes seconds per call: a test that needs
    no long stretch behind the window asks for fewer there)."""
    return _window(p) + (emu if backend == "emu" else 13)


def _model_beta(p):
    return p.pf_beta if p.mask_pf else 0.0


def _drive(rt, x, at=None, active=None):
    """One hop per call; at: {call index: function(rt)} run in front of that call; active: {call index: mask}.  -> y, lsnr"""
    ys, ls = [], []
    for t in range(x.shape[1] // HOP):
        if at and t in at:
            at[t](rt)
        y, l = rt.process(torch.from_numpy(x[:, t * HOP:(t + 1) * HOP]), return_lsnr=True, active=active.get(t) if active else None)
        ys.append(y), ls.append(l)
    return torch.cat(ys, 1).numpy(), torch.cat(ls, 1).numpy()


@functools.lru_cache(maxsize=None)
def _oracle(name, seed, rows, T, s, lim_db, beta, thr=OPEN):
    """stream s of _noise(rows, T, seed) through the oracle: computed once per case, shared between the tests."""
    p = named_params(name)
    y, l, info = S.process_stream(p, _sd(name), _noise(rows, T, seed)[s], atten_lim_db=lim_db, pf_beta=beta, thresholds=thr)
    y.setflags(write=False)
    return y, l, info


def _mixed_settings(p):
    return [(100.0, 0.0), (12.0, _model_beta(p)), (100.0, 0.05), (6.0, 0.02)]


_RUNS = {}


def _mixed_run(backend, name):
    """Four streams with four (lim_db, beta) on one handle — shared by the uniform-handle test and the oracle test."""
    from deepfilternet_amd.streaming import DfStream

    key = (backend, name)
    if key not in _RUNS:
        p, model, df_state = _setup(backend, name)
        x = _noise(4, _hops(p, backend, 2), 31)
        rt = DfStream(model, df_state, streams=4)
        cfg = _mixed_settings(p)
        rt.set_atten_lim([c[0] for c in cfg], streams=[0, 1, 2, 3])
        rt.set_post_filter_beta([cfg[0][1], cfg[2][1], cfg[3][1]], streams=[0, 2, 3])   # stream 1: never given one (the model's setting)
        _RUNS[key] = (p, model, df_state, x, _drive(rt, x))
    return _RUNS[key]


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_every_stream_equals_a_uniform_handle_with_its_settings(backend, name):
    """Row s of the per-stream handle == row s of a fresh handle that was given stream s's values handle-wide, output and lsnr, to the bit.
    Stream 0 (no limit, no post filter) is the case in which the uniform handle runs the finishing kernel's PF = false instance.  Streams
    1 to 3 are more than 20 bars away from the all-default handle: a setter that does nothing is seen."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state, x, (y, lsnr) = _mixed_run(backend, name)
    y_def, _ = _drive(DfStream(model, df_state, streams=4), x)
    for s, (lim_db, beta) in enumerate(_mixed_settings(p)):
        rt = DfStream(model, df_state, streams=4)
        rt.set_atten_lim(lim_db)
        if s != 1:
            rt.set_post_filter_beta(beta)
        yu, lu = _drive(rt, x)
        print(f"{name}: stream {s} ({lim_db} dB, beta {beta}): vs uniform {rms(y[s] - yu[s]):.3e}, vs all-default handle {rms(y[s] - y_def[s]):.3e}")
        assert np.array_equal(y[s], yu[s]) and np.array_equal(lsnr[s], lu[s]), s
        if s > 0:
            assert rms(y[s] - y_def[s]) > 20 * BAR, s
    model.check()


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_every_stream_equals_the_oracle_with_its_settings(backend, name):
    p, model, _, x, (y, lsnr) = _mixed_run(backend, name)
    T = x.shape[1] // HOP
    for s, (lim_db, beta) in enumerate(_mixed_settings(p)):
        yr, lr, _ = _oracle(name, 31, 4, T, s, lim_db, beta)
        err = rms(y[s] - yr)
        print(f"{name}: stream {s} ({lim_db} dB, beta {beta}) vs oracle {err:.3e}")
        assert err < BAR, (s, err)
        assert np.abs(lsnr[s] - lr)[p.df_lookahead:].max() < 1e-3
    model.check()


GATED_SEED = 2


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_per_stream_thresholds_on_a_gated_handle(backend, name):
    """gating=True: stream 0 with thresholds that skip nothing, streams 1 and 2 with two triples from inside the lsnr distribution of these
    signals (tests/test_streaming_gated.py's two quantile sets).  The oracle shows on the CPU that each triple skips stages for its stream
    and that no decision hinges on the last bits.  Each stream == the uniform gated handle with its triple (bits) == the oracle with its
    triple (bar); streams 1 and 2 under each other's triple are more than 20 bars away."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, name)
    sd, T = _sd(name), _hops(p, backend)
    x = _noise(3, T, GATED_SEED)
    x[2] *= np.linspace(0.05, 2, HOP * T).astype(np.float32)           # a level ramp: a wider lsnr distribution
    thr = [OPEN, _thresholds(p, sd, x, (0.15, 0.85, 0.5)), _thresholds(p, sd, x, (0.0, 0.3, 0.15))]
    assert thr[1] != thr[2]
    ref = [S.process_stream(p, sd, x[s], thresholds=thr[s]) for s in range(3)]
    for s in (1, 2):
        assert any(f != (True, False, True) for f in ref[s][2]["flags"]), s          # the triple really skips stages for its stream
        assert min(np.abs(np.asarray(ref[s][2]["lsnr_pass1"]) - t).min() for t in thr[s]) > 1e-4
    rt = DfStream(model, df_state, streams=3, gating=True, thresholds=OPEN)
    rt.set_thresholds(*zip(thr[1], thr[2]), streams=[1, 2])
    y, lsnr = _drive(rt, x)
    uni = {s: _drive(DfStream(model, df_state, streams=3, gating=True, thresholds=thr[s]), x) for s in (1, 2)}
    uni[0] = _drive(DfStream(model, df_state, streams=3, gating=True, thresholds=OPEN), x)
    d = p.df_lookahead
    for s in range(3):
        assert np.array_equal(y[s], uni[s][0][s]) and np.array_equal(lsnr[s], uni[s][1][s]), s
        err = rms(y[s] - ref[s][0])
        print(f"{name}: stream {s} thresholds {thr[s]} vs oracle {err:.3e}")
        assert err < BAR, (s, err)
        live = np.zeros(T, bool)
        live[ref[s][2]["accepted"][d:]] = True
        assert np.abs(lsnr[s] - ref[s][1])[live].max() < 1e-3
    assert rms(uni[2][0][1] - y[1]) > 20 * BAR and rms(uni[1][0][2] - y[2]) > 20 * BAR   # each other's triple: seen
    model.check()


def test_per_stream_thresholds_reach_process_raw(backend):
    """dfx_stream_process_raw reads the thresholds too: stages, gains and coefficients of a per-stream handle == those of the uniform
    handles, stream by stream; the two triples (quartiles of the lsnr these frames get, taken from a run that skips nothing) decide
    differently somewhere."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, "pf32")
    K = p.df_lookahead + (5 if backend == "emu" else 12)
    rng = np.random.default_rng(6)
    spec = torch.from_numpy((0.5 * rng.standard_normal((K, 3, p.fft_size // 2 + 1, 2))).astype(np.float32))
    spec *= torch.tensor([1e-3, 1.0, 30.0]).view(1, 3, 1, 1) * torch.linspace(0.2, 3, K).view(K, 1, 1, 1)

    def raw(rt):
        out = [rt.process_raw(torch.view_as_complex(spec[k].contiguous())) for k in range(K)]
        return [torch.stack([o[i] for o in out]).numpy() for i in range(4)]   # lsnr [K, 3], gains, coefs, stages

    mk = lambda thr: DfStream(model, df_state, streams=3, gating=True, thresholds=thr)   # noqa: E731
    ls = np.sort(raw(mk(OPEN))[0][p.df_lookahead:].reshape(-1))
    q = lambda f: float(ls[int(f * (len(ls) - 1))] + ls[int(f * (len(ls) - 1)) + 1]) / 2   # noqa: E731
    thr = [OPEN, (q(0.15), q(0.8), q(0.5)), (q(0.05), q(0.4), q(0.2))]
    rt = mk(OPEN)
    rt.set_thresholds([t[0] for t in thr[1:]], [t[1] for t in thr[1:]], [t[2] for t in thr[1:]], streams=torch.tensor([1, 2]))
    got = raw(rt)
    uni = [raw(mk(t)) for t in thr]
    d = p.df_lookahead                                                    # (the first `lookahead` frames have no net position: placeholders)
    for s in range(3):
        st = got[3][d:, s]
        assert np.array_equal(st, uni[s][3][d:, s]) and np.array_equal(got[0][d:, s], uni[s][0][d:, s]), s
        assert np.array_equal(got[1][d:, s][(st & 2) != 0], uni[s][1][d:, s][(st & 2) != 0]), s      # gains where they exist
        assert np.array_equal(got[2][d:, s][(st & 8) != 0], uni[s][2][d:, s][(st & 8) != 0]), s      # coefficients likewise
    assert any(not np.array_equal(uni[1][3][d:, s], uni[2][3][d:, s]) for s in range(3))     # the triples differ in their decisions
    assert not np.array_equal(uni[0][3][d:], uni[1][3][d:])
    model.check()


@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_mid_stream_change(backend, name):
    """Stream 1's limit and beta are set between calls c - 1 and c, c past the window: stream 1 == (bits) a handle on which the handle-wide
    setters were called at the same point; streams 0 and 2 keep the bits of a run without the change."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, name)
    T, c = _hops(p, backend, 3), _window(p) + 1
    x = _noise(3, T, 33)

    def per_stream(rt):
        rt.set_atten_lim(9.0, streams=[1])
        rt.set_post_filter_beta(0.04, streams=[1])

    def handle_wide(rt):
        rt.set_atten_lim(9.0)
        rt.set_post_filter_beta(0.04)

    y, lsnr = _drive(DfStream(model, df_state, streams=3), x, {c: per_stream})
    yu, lu = _drive(DfStream(model, df_state, streams=3), x, {c: handle_wide})
    y0, l0 = _drive(DfStream(model, df_state, streams=3), x)
    assert np.array_equal(y[1], yu[1]) and np.array_equal(lsnr[1], lu[1])
    assert np.array_equal(y[[0, 2]], y0[[0, 2]]) and np.array_equal(lsnr[[0, 2]], l0[[0, 2]])         # the bystanders
    assert np.array_equal(y[1, : (c - 1) * HOP], y0[1, : (c - 1) * HOP])
    assert rms(y[1, c * HOP:] - y0[1, c * HOP:]) > 20 * BAR                                           # the change is seen
    model.check()


def test_with_pauses_and_resets(backend):
    """A pausable handle.  Stream 1 sits calls c .. c + 2 out and gets a limit while it is paused; stream 2 is reset in front of call c and
    then given its own limit and beta.  Each stream against the oracle on the hops it delivered with the settings in force.  Stream 1's
    setting changes mid-stream and the oracle has no such switch: its hops before the change are the oracle's without the limit, its hops
    after it the oracle's with it — except the first hop after the change, whose samples overlap-add the last frame before and the first
    frame after (that hop is pinned by test_mid_stream_change).  Setters do not move rt.frames."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, "pf32")
    sd = _sd("pf32")
    T, c = _hops(p, backend), _window(p) + 1
    x = _noise(3, T, 34)
    rt = DfStream(model, df_state, streams=3, pausable=True)
    ages = {}

    def at_c(rt):
        rt.reset([2])
        before = rt.frames.tolist()
        rt.set_atten_lim(6.0, streams=[2])
        rt.set_post_filter_beta(0.05, streams=[2])
        assert rt.frames.tolist() == before == [c, c, 0]

    def at_c1(rt):
        before = rt.frames.tolist()
        rt.set_atten_lim(12.0, streams=[1])                             # stream 1 is paused in the calls around this
        ages["c1"] = (before, rt.frames.tolist())

    paused = {t: [1, 0, 1] for t in (c, c + 1, c + 2)}
    y, _ = _drive(rt, x, {c: at_c, c + 1: at_c1}, paused)
    assert ages["c1"][0] == ages["c1"][1] == [c + 1, c, 1]
    assert rt.frames.tolist() == [T, T - 3, T - c]
    assert rms(y[0] - _fresh_stream_oracle(p, sd, x[0])) < BAR
    assert float(np.abs(y[1, c * HOP:(c + 3) * HOP]).max()) == 0.0
    sig1 = np.concatenate([x[1, : c * HOP], x[1, (c + 3) * HOP:]])       # what stream 1 delivered
    got1 = np.concatenate([y[1, : c * HOP], y[1, (c + 3) * HOP:]])
    plain, limited = _fresh_stream_oracle(p, sd, sig1), S.process_stream(p, sd, sig1, atten_lim_db=12.0, pf_beta=p.pf_beta, thresholds=OPEN)[0]
    assert rms(got1[: c * HOP] - plain[: c * HOP]) < BAR
    assert rms(got1[(c + 1) * HOP:] - limited[(c + 1) * HOP:]) < BAR
    assert rms(got1[(c + 1) * HOP:] - plain[(c + 1) * HOP:]) > 20 * BAR
    assert rms(y[2, : c * HOP] - _fresh_stream_oracle(p, sd, x[2, : c * HOP])) < BAR
    ref2 = S.process_stream(p, sd, x[2, c * HOP:], atten_lim_db=6.0, pf_beta=0.05, thresholds=OPEN)[0]
    assert rms(y[2, c * HOP:] - ref2) < BAR, rms(y[2, c * HOP:] - ref2)
    assert rms(y[2, c * HOP:] - _fresh_stream_oracle(p, sd, x[2, c * HOP:])) > 20 * BAR
    model.check()


def test_multichannel_streams_with_their_own_settings(backend):
    """channels=2: a stream's values hold for both its rows, and the post filter's walk over the stream's flattened two-channel frame (the
    last (2 * F) % 4 bins are left alone, lib.rs:446-471) runs on each stream's own beta."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, "pf32")
    sd, T = _sd("pf32"), _hops(p, backend)
    x = _noise(4, T, 35)
    x[1] *= 0.3
    x[3] *= 0.5
    rt = DfStream(model, df_state, streams=4, channels=2, reduce_mask="mean")
    rt.set_atten_lim([12.0, 6.0], streams=[0, 1])
    rt.set_post_filter_beta(0.05, streams=[0])
    y, _ = _drive(rt, x)
    cfg = [(12.0, 0.05), (6.0, p.pf_beta)]
    for k, (lim_db, beta) in enumerate(cfg):
        ref = S.process_stream(p, sd, x[2 * k: 2 * k + 2], atten_lim_db=lim_db, pf_beta=beta, thresholds=OPEN, reduce_mask="mean")[0]
        err = rms(y[2 * k: 2 * k + 2] - ref)
        assert err < BAR, (k, err)
        other = S.process_stream(p, sd, x[2 * k: 2 * k + 2], atten_lim_db=cfg[1 - k][0], pf_beta=cfg[1 - k][1], thresholds=OPEN, reduce_mask="mean")[0]
        assert rms(y[2 * k: 2 * k + 2] - other) > 20 * BAR
    s = rt.settings
    assert s["atten_lim_db"].tolist() == [12.0, 6.0] and s["post_filter_beta"].shape == (2,) and s["thresholds"].shape == (2, 3)
    model.check()


def _launches(rt, x, t0, n):
    """Launch counts of every profiled kernel over calls t0 .. t0 + n - 1 (the calls before them are driven first)."""
    from deepfilternet_amd import _lib

    _drive(rt, x[:, : t0 * HOP])
    _lib.prof_enable("all")
    try:
        _lib.prof_reset()
        y, _ = _drive(rt, x[:, t0 * HOP:(t0 + n) * HOP])
        counts = {k: v[1] for k, v in _lib.prof_read().items()}
    finally:
        _lib.prof_enable(None)
    return y, counts


@pytest.mark.parametrize("gating", [False, True])
def test_handle_wide_setters_restore_uniformity(backend, gating):
    """After per-stream values the three handle-wide setters make the handle uniform again: the same bits as a handle that never was
    per-stream, and over ten steady hops the same launch count of every kernel.  A handle that IS per-row has those counts too: the
    steady hop gains no launch."""
    from deepfilternet_amd.streaming import DfStream

    if emu_subset(backend) and not gating:
        pytest.skip("interpreter subset: the gated handle (which reads all three settings) runs here, the ungated one on the GPU (DFX_EMU_ALL=1 runs both)")
    p, model, df_state = _setup(backend, "pf32")
    W = p.df_lookahead if backend == "emu" else _window(p)               # calls in front of the ten that are counted (the same for every handle)
    T = W + 1 + 10
    x = _noise(3, T, 36)
    thr = (-5.0, 25.0, 12.0)
    mk = lambda: DfStream(model, df_state, streams=3, gating=gating)   # noqa: E731

    def per_row(rt):
        rt.set_atten_lim([12.0, 6.0], streams=[0, 2])
        rt.set_post_filter_beta(0.05, streams=[1])
        rt.set_thresholds(-8.0, 28.0, 15.0, streams=[2])

    def uniform(rt):
        rt.set_atten_lim(100.0)
        rt.set_post_filter_beta(0.03)
        rt.set_thresholds(*thr)

    never = mk()
    uniform(never)
    y_never, n_never = _launches(never, x, W + 1, 10)
    back = mk()
    per_row(back)
    uniform(back)
    y_back, n_back = _launches(back, x, W + 1, 10)
    assert np.array_equal(y_back, y_never)
    assert n_back == n_never and sum(n_never.values()) > 10, (n_back, n_never)
    rows = mk()
    per_row(rows)
    y_rows, n_rows = _launches(rows, x, W + 1, 10)
    assert n_rows == n_never, (n_rows, n_never)
    assert not np.array_equal(y_rows, y_never)
    s = back.settings
    assert s["atten_lim_db"].tolist() == [100.0] * 3 and np.allclose(s["post_filter_beta"].numpy(), 0.03)
    assert np.allclose(s["thresholds"].numpy(), np.tile(np.float32(thr), (3, 1)))
    model.check()


def test_pass_through_stays_a_handle_wide_mode(backend):
    """set_atten_lim(0) handle-wide: the input comes back undelayed, lsnr 35 (tract.rs:540-543).  set_atten_lim(0, streams=[1]): stream 1's
    input comes back delayed by delay_frames hops plus the STFT's fft - hop samples (the mix with lim = 0.99999994, like dfx_enhance), its
    lsnr is the network's, and the other streams are enhanced as ever."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, "pf32")
    T = _hops(p, backend, 2)
    x = _noise(3, T, 37)
    rt = DfStream(model, df_state, streams=3)
    rt.set_atten_lim(0.0)
    y, l = rt.process(torch.from_numpy(x[:, :HOP]), return_lsnr=True)
    assert np.array_equal(y.numpy(), x[:, :HOP]) and np.all(l.numpy() == 35.0)
    rt = DfStream(model, df_state, streams=3)
    rt.set_atten_lim(0.0, streams=[1])
    y, lsnr = _drive(rt, x)
    y0, _ = _drive(DfStream(model, df_state, streams=3), x)
    d = rt.delay_frames * HOP + p.fft_size - p.hop_size
    err = rms(y[1, d:] - x[1, :-d])
    print(f"stream 1 vs its delayed input {err:.3e}")
    assert err < BAR and float(np.abs(y[1, : rt.delay_frames * HOP]).max()) == 0.0
    live = lsnr[1, rt.delay_frames:]
    assert np.all(np.isfinite(live)) and np.all(live != 35.0)
    assert np.array_equal(y[[0, 2]], y0[[0, 2]])
    assert rt.settings["atten_lim_db"].tolist() == [100.0, 0.0, 100.0]
    model.check()


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("atten_lim_db", "post_filter_beta", "thresholds"))


def test_edges_and_errors(backend):
    import ctypes as C

    from deepfilternet_amd import _lib
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup(backend, "pf32")
    T = p.df_lookahead + 3
    x = _noise(3, T, 38)
    rt = DfStream(model, df_state, streams=3)
    s0 = rt.settings
    assert s0["atten_lim_db"].tolist() == [100.0] * 3 and s0["thresholds"].tolist() == [[-10.0, 30.0, 20.0]] * 3
    assert np.allclose(s0["post_filter_beta"].numpy(), p.pf_beta)                      # the model's value where none was set
    # an empty id list is a no-op
    rt.set_atten_lim([], streams=[])
    rt.set_post_filter_beta(0.5, streams=torch.zeros(0, dtype=torch.int64))
    rt.set_thresholds(0.0, 1.0, 2.0, streams=[])
    assert _same(rt.settings, s0)
    L = _lib.lib()
    for fn in NEW[:3]:
        assert getattr(L, fn)(rt._h, None, 0, None, _lib.stream()) == 0
        assert getattr(L, fn)(rt._h, None, 1, None, _lib.stream()) == 1                # DFX_ERR_INVALID_ARG
        assert getattr(L, fn)(None, None, 0, None, _lib.stream()) == 1
    assert L.dfx_stream_get_settings(rt._h, C.cast(None, C.POINTER(C.c_float))) == 1
    # errors change nothing
    bad = [lambda: rt.set_atten_lim(6.0, streams=[3]), lambda: rt.set_atten_lim([6.0, 6.0], streams=[0, -1]),
           lambda: rt.set_post_filter_beta([0.1, -0.1], streams=[0, 1]), lambda: rt.set_atten_lim([6.0, float("nan")], streams=[0, 1]),
           lambda: rt.set_thresholds(0.0, [1.0, float("nan")], 2.0, streams=[0, 1]), lambda: rt.set_post_filter_beta(float("nan"), streams=[2])]
    for f in bad:
        with pytest.raises(_lib.DfxError) as e:
            f()
        assert e.value.code == 1
        assert _same(rt.settings, s0)
    with pytest.raises(TypeError):
        rt.set_atten_lim(6.0, streams=[0.5])
    with pytest.raises(ValueError):
        rt.set_atten_lim([6.0, 7.0, 8.0], streams=[0, 1])
    with pytest.raises(ValueError):
        rt.set_thresholds([0.0], 1.0, 2.0, streams=[0, 1])
    assert _same(rt.settings, s0)
    y_plain, _ = _drive(DfStream(model, df_state, streams=3), x)
    y, _ = _drive(rt, x)
    assert np.array_equal(y, y_plain)                                                  # nothing of the above reached the device either
    # duplicate ids: the last occurrence wins; settings round-trip; resets leave them alone
    rt = DfStream(model, df_state, streams=3)
    rt.set_atten_lim([20.0, -9.0, 12.0, 250.0], streams=[1, 0, 1, 2])
    rt.set_post_filter_beta([0.5, 0.0], streams=[2, 2])
    rt.set_thresholds([-1.0, -2.0], [5.0, 6.0], [3.0, 4.0], streams=[0, 0])
    s = rt.settings
    assert s["atten_lim_db"].tolist() == [9.0, 12.0, 100.0]
    assert np.allclose(s["post_filter_beta"].numpy(), [p.pf_beta, p.pf_beta, 0.0])
    assert s["thresholds"].tolist() == [[-2.0, 6.0, 4.0], [-10.0, 30.0, 20.0], [-10.0, 30.0, 20.0]]
    y, _ = _drive(rt, x)
    want = DfStream(model, df_state, streams=3)
    want.set_atten_lim([9.0, 12.0], streams=[0, 1])
    want.set_post_filter_beta(0.0, streams=[2])
    yw, _ = _drive(want, x)
    assert np.array_equal(y, yw)
    assert rms(y[1] - y_plain[1]) > 20 * BAR
    rt.reset([1])
    rt.reset()
    assert _same(rt.settings, s)
    y2, _ = _drive(rt, x)
    assert np.array_equal(y2, y)                                                       # ... on the device too
    model.check()


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
        for name in NEW:
            assert re.search(r"\b%s\s*\(" % name, header), name
            assert name in _lib.SIGNATURES and hasattr(lib, name), (name, lib_path)


@pytest.mark.gpu
@pytest.mark.parametrize("streams,channels", [(9, 1), (520, 1), (520, 2), (1100, 1)])
def test_row_groups_and_id_chunks(hip_backend, streams, channels):
    """Every stream its own limit (6 + s % 7 dB), every third one beta 0.05, all set in ONE call per setting over all ids: the rows cross
    the 8-clip groups of the finishing kernel and, at 1100 streams, the id chunks of the setter kernel.  Rows 0, 7, 8, the last of the
    first id chunk, the first of the next and the last row against the oracle; at 9 streams every row against handles that were given one
    of the limits handle-wide."""
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _setup("hip", "pf32")
    sd = _sd("pf32")
    T = p.df_lookahead + 4
    n = streams // channels
    base = _noise(16, T, 39)
    x = np.ascontiguousarray(np.tile(base, (streams // 16 + 1, 1))[:streams])
    x *= np.linspace(0.5, 1.5, streams, dtype=np.float32)[:, None]
    lim = [6.0 + (s % 7) for s in range(n)]
    third = list(range(0, n, 3))
    rt = DfStream(model, df_state, streams=streams, channels=channels)
    rt.set_atten_lim(lim, streams=torch.arange(n))
    rt.set_post_filter_beta(0.05, streams=third)
    y, _ = _drive(rt, x)
    for s in sorted({0, 7, 8, SET_IDS - 1, SET_IDS, n - 1} & set(range(n))):
        sig = x[s] if channels == 1 else x[s * channels:(s + 1) * channels]
        ref = S.process_stream(p, sd, sig, atten_lim_db=lim[s], pf_beta=0.05 if s % 3 == 0 else p.pf_beta, thresholds=OPEN, reduce_mask="mean")[0]
        got = y[s] if channels == 1 else y[s * channels:(s + 1) * channels]
        err = rms(got - ref)
        assert err < BAR, (s, err)
    if streams == 9:
        for v in sorted(set(lim)):
            for beta in (0.05, p.pf_beta):
                u = DfStream(model, df_state, streams=streams)
                u.set_atten_lim(v)
                u.set_post_filter_beta(beta)
                yu, _ = _drive(u, x)
                for s in range(n):
                    if lim[s] == v and (0.05 if s % 3 == 0 else p.pf_beta) == beta:
                        assert np.array_equal(y[s], yu[s]), s
    model.check()
