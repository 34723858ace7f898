"""Streams that move between DfStream handles (dfx_stream_export_streams / dfx_stream_import_streams): a stream exported from one handle
and imported into another continues there as if it had never moved — in bits where both handles run it through the same kernels in the
same slot (twin handles), within the bars of test_stream_slots.py / test_streaming_gated.py against the oracles where the place, the
hop count, the cut into calls or the form of the windows differ — and nobody else notices: the source runs on, the destination's other
streams keep their bits, a refused import changes nothing, and past H + L hops the destination enqueues what it always did."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import stream_oracle as S
from tests.helpers import emu_subset, named_params, rms, torch_sd
from tests.test_stream_slots import HOP, _fresh_stream_oracle, _noise

BAR = 1e-6   # a stream against its oracle (test_stream_slots.py)


def _window(p):
    """(H, L) of dfx_stream_create: history frames in front of the new ones, lookahead."""
    return max(2 + p.df_pathway_kernel_size_t - 1, p.df_order - 1 - p.df_lookahead), p.df_lookahead


def _emu_only_pf32(backend, name):
    if backend == "emu" and name != "pf32":
        pytest.skip("the interpreter is slow: it covers the conv_ch=32 model (kt=3); the GPU run covers all three")


def _hop(x, k, n=1, hop=HOP):
    return torch.from_numpy(np.ascontiguousarray(x[:, k * hop:(k + n) * hop]))


@functools.lru_cache(maxsize=None)
def _model(name, lookahead=None):
    from deepfilternet_amd.enhance import init_df

    p = named_params(name)
    if lookahead is not None and p.df_lookahead < lookahead:
        p.df_lookahead = p.conv_lookahead = lookahead
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=9)
    return p, torch_sd(p, 9), model, df_state


@functools.lru_cache(maxsize=None)
def _gated_scenario(name, T, quantiles=(0.15, 0.85, 0.5)):
    """test_streaming_gated.py's three signals with thresholds inside their lsnr distribution, and the oracle's answer to each."""
    from tests.test_streaming_gated import _signals, _thresholds

    p, sd, _, _ = _model(name)
    x = _signals(T, 2)
    thr = _thresholds(p, sd, x, quantiles)
    ref = [S.process_stream(p, sd, xi, thresholds=thr) for xi in x]
    for r in ref:   # robust decisions only
        assert min(np.abs(np.asarray(r[2]["lsnr_pass1"]) - t).min() for t in thr) > 1e-4
    return x, thr, ref


@functools.lru_cache(maxsize=None)
def _frozen_scenario(name):
    """test_reset_on_a_gated_handle's scenario: three streams of noise, stream 1 digitally silent for the 9 hops up to and including hop t,
    under the first threshold set with which the oracle has it frozen at hops t - 1 and t.  Returns (x, thresholds, t)."""
    from tests.test_streaming_gated import _thresholds

    p, sd, _, _ = _model(name)
    t, T = 10, 20
    x = _noise(3, T, 2)
    x[1, (t - 8) * HOP: (t + 1) * HOP] = 0
    x[2] *= np.linspace(0.01, 3, HOP * T).astype(np.float32)
    for quantiles in ((0.15, 0.85, 0.5), (0.0, 0.3, 0.15)):
        thr = _thresholds(p, sd, [x[0], x[1], x[2]], quantiles)
        info = S.process_stream(p, sd, x[1], thresholds=thr)[2]
        if t - 1 not in info["accepted"] and t not in info["accepted"]:
            break
    assert t - 1 not in info["accepted"] and t not in info["accepted"]
    assert min(np.abs(np.asarray(info["lsnr_pass1"]) - v).min() for v in thr) > 1e-4   # robust decisions only
    return x, thr, t


# ---- 1. completeness, in bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2])
@pytest.mark.parametrize("kind", ["plain", "gated", "pausable", "sr16k", "ch2"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_moved_stream_continues_in_bits(backend, name, kind, lead):
    """Twin handles A and A' (same size, one hop per call, the same input on streams 0 and 2; stream 1 of A' hears other noise).  After t
    hops (t > H + L) A's stream 1 is exported and imported into A' stream 1; from then on, given A's input, A' stream 1 is bit-equal to
    A's: same slot, same size, same kernels, so any difference is a state row that did not travel.  lead: A' is that many hops ahead of A
    (fed as many extra leading hops): other parity, other pending-sum slot for kt = 3, other place in the linear windows; the comparison
    is aligned on A's time.  A is bit-equal to a run without the export, A' streams 0 and 2 to a run without the import.  gated: stream 1
    is silent-skipped (frozen) at hop t; pausable: it sat out the call before the export."""
    from deepfilternet_amd.streaming import DfStream

    _emu_only_pf32(backend, name)
    if emu_subset(backend) and (kind != "plain" or lead != 1):
        pytest.skip("interpreter subset: the plain handle one hop ahead runs here, the rest on the GPU (DFX_EMU_ALL=1 runs all)")
    p, sd, model, df_state = _model(name)
    H, L = _window(p)
    t = H + L + 2
    T = t + (4 if backend == "emu" else 10)
    ch = 2 if kind == "ch2" else 1
    hop = HOP // 3 if kind == "sr16k" else HOP
    kw = {}
    if kind == "gated":
        x, thr, t = _frozen_scenario(name)
        T = x.shape[1] // HOP
        kw = dict(gating=True, thresholds=thr)
    else:
        x = (0.1 * np.random.default_rng(2).standard_normal((3 * ch, hop * T))).astype(np.float32)
        if ch == 2:
            x[1::2] *= 0.5
    if kind == "pausable":
        kw = dict(pausable=True)
    if kind == "sr16k":
        kw = dict(sr=16000)
    rows1 = slice(ch, 2 * ch)
    other = (0.1 * np.random.default_rng(3).standard_normal((3 * ch, hop * (T + lead)))).astype(np.float32)
    xp = np.concatenate([other[:, : lead * hop], x], 1)     # A' input: `lead` hops of its own first
    xp[rows1, : (lead + t) * hop] = other[rows1, : (lead + t) * hop]
    mk = lambda: DfStream(model, df_state, streams=3 * ch, channels=ch, **kw)   # noqa: E731
    lsnr = kind == "gated"
    every = [True] * 3 if kind == "pausable" else None
    sits_out = lambda k: [True, k != t - 1, True] if kind == "pausable" else None   # noqa: E731  (A's stream 1 in the call before the export)

    def run(rt, sig, first, move, mask):
        """hops [first, first + T) of sig, one per call; move(): in front of the hop that is hop t of A's time"""
        out, ls = [], []
        for k in range(T):
            if move and k == t:
                move()
            r = rt.process(_hop(sig, first + k, hop=hop), return_lsnr=lsnr, active=mask(k))
            out.append(r[0] if lsnr else r)
            if lsnr:
                ls.append(r[1])
        return torch.cat(out, 1).cpu().numpy(), (torch.cat(ls, 1).cpu().numpy() if lsnr else None)

    A, A_plain, Ap, Ap_plain = mk(), mk(), mk(), mk()
    for rt in (Ap, Ap_plain):
        for k in range(lead):
            rt.process(_hop(xp, k, hop=hop))
    snaps = []
    ya, la = run(A, x, 0, lambda: snaps.append(A.export_streams([1])), sits_out)
    assert snaps[0].ages.tolist() == [t - (1 if kind == "pausable" else 0)]
    yp, lp = run(Ap, xp, lead, lambda: Ap.import_streams([1], snaps[0]), lambda k: every)
    ya_plain, la_plain = run(A_plain, x, 0, None, sits_out)
    yp_plain, _ = run(Ap_plain, xp, lead, None, lambda k: every)
    assert np.array_equal(ya[rows1, t * hop:], yp[rows1, t * hop:]), np.abs(ya[rows1, t * hop:] - yp[rows1, t * hop:]).max()
    assert not np.array_equal(ya_plain[rows1, t * hop:], yp_plain[rows1, t * hop:])   # (without the move the two streams differ)
    assert np.array_equal(ya, ya_plain)                                                # the source did not notice
    by = [r for r in range(3 * ch) if not ch <= r < 2 * ch]
    assert np.array_equal(yp[by], yp_plain[by])                                        # nor did the destination's other streams
    assert np.array_equal(yp[rows1, : t * hop], yp_plain[rows1, : t * hop])
    if lsnr:
        assert float(np.abs(ya[1, (t - 1) * HOP: (t + 1) * HOP]).max()) == 0.0 and la[1, t - 1] == -15.0 and la[1, t] == -15.0   # moved while frozen
        assert np.array_equal(la[1, t:], lp[1, t:], equal_nan=True) and np.array_equal(la, la_plain, equal_nan=True)
    assert A.frames.tolist()[1] == Ap.frames.tolist()[1]
    model.check()


# ---- 2. another place, against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one-hop", "cuts", "ring-to-linear", "linear-to-ring"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_moved_stream_matches_its_oracle(backend, monkeypatch, name, mode):
    """Stream 1 of a 3-stream handle is exported at hop t and imported into slot 0 of a 2-stream handle that has run t' hops of other
    noise (t - t' = 3: odd and no multiple of kt - 1 — other parity, other pending-sum slot).  Source output before the move followed
    by destination output after it is within 1e-6 RMS of the fresh-stream oracle on the whole signal; the same comparison without the
    import is more than 20 x that away.  cuts: max_frames = 3 and calls of [3, 1, 2, 3, ...] hops on both sides (stale pending sums:
    the destination rebuilds them); ring-to-linear / linear-to-ring: DFX_STREAM_LINEAR=0 on one side only."""
    from deepfilternet_amd.streaming import DfStream

    _emu_only_pf32(backend, name)
    if emu_subset(backend) and mode != "one-hop":
        pytest.skip("interpreter subset: one hop per call runs here, the rest on the GPU (DFX_EMU_ALL=1 runs all)")
    p, sd, model, df_state = _model(name)
    H, L = _window(p)
    kt = p.df_pathway_kernel_size_t
    if mode == "cuts":
        src_cuts, dst_before, dst_after = [3, 1, 2, 3, 2], [3, 1, 2, 2], [3, 1, 2, 3] if backend != "emu" else [3, 1]
    else:
        src_cuts, dst_before, dst_after = [1] * 11, [1] * 8, [1] * (4 if backend == "emu" else 9)
    t, tp, n_after = sum(src_cuts), sum(dst_before), sum(dst_after)
    assert (t - tp) % 2 == 1 and (kt == 1 or (t - tp) % (kt - 1) != 0 or kt == 2) and tp >= H + L
    mf = 3 if mode == "cuts" else 1
    sig = _noise(1, t + n_after, 11)[0]
    xs = _noise(3, t, 12)
    xs[1] = sig[: t * HOP]
    xd = _noise(2, tp + n_after, 13)

    def make(side, streams):
        monkeypatch.setenv("DFX_STREAM_LINEAR", "0" if mode.startswith("ring" if side == "src" else "linear") and "-to-" in mode else "1")
        return DfStream(model, df_state, streams=streams, max_frames=mf)

    def drive(rt, x, cuts, pos=0):
        out = []
        for n in cuts:
            out.append(rt.process(_hop(x, pos, n)))
            pos += n
        return torch.cat(out, 1).cpu().numpy()

    src = make("src", 3)
    y_src = drive(src, xs, src_cuts)
    dst, dst_plain = make("dst", 2), make("dst", 2)
    drive(dst, xd, dst_before), drive(dst_plain, xd, dst_before)
    dst.import_streams([0], src.export_streams([1]))
    assert dst.frames.tolist() == [t, tp]
    xd[0, tp * HOP:] = sig[t * HOP:]
    y_dst, y_plain = drive(dst, xd, dst_after, tp), drive(dst_plain, xd, dst_after, tp)
    ref = _fresh_stream_oracle(p, sd, sig)
    err = rms(np.concatenate([y_src[1], y_dst[0]]) - ref)
    miss = rms(np.concatenate([y_src[1], y_plain[0]]) - ref)
    print(f"{name}/{mode}: moved stream vs oracle {err:.3e}; without the import {miss:.3e}")
    assert err < BAR, err
    assert miss > 20 * BAR, miss
    if mode != "cuts":   # one hop per call on both runs: the bystander keeps its bits (cuts: the library may cut the calls differently for a while)
        assert np.array_equal(y_dst[1], y_plain[1])
    else:
        assert rms(y_dst[1] - y_plain[1]) < 2e-6 * max(rms(y_plain[1]), 1e-3) + 1e-7
    assert dst.frames.tolist() == [t + n_after, tp + n_after]
    model.check()


# ---- 3. ages --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["warm-up", "inside-window", "old-into-fresh", "old-into-young"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_ages_travel(backend, name, case):
    """warm-up: a stream of age 1 < L (models with less than two hops of lookahead run with two here) enters a handle at hop >> H + L;
    inside-window: one of age L + 1 < H + L; old-into-fresh: one of age >> H + L enters a fresh handle at hop 0 (its birth there is
    negative); old-into-young: the same into a handle that has run 2 hops.  Each time the moved stream meets the oracle on its whole
    signal, DfStream.frames reports the travelled age, and the destination's other stream equals its own oracle (on the fresh handle:
    `delay_frames` hops of silence first)."""
    from deepfilternet_amd.streaming import DfStream

    _emu_only_pf32(backend, name)
    if emu_subset(backend) and case != "old-into-fresh":
        pytest.skip("interpreter subset: the fresh destination runs here, the rest on the GPU (DFX_EMU_ALL=1 runs all)")
    p, sd, model, df_state = _model(name, 2)
    H, L = _window(p)
    assert L >= 2
    big = H + L + 6
    age, tp = {"warm-up": (1, big), "inside-window": (L + 1, big), "old-into-fresh": (big, 0), "old-into-young": (big, 2)}[case]
    n_after = (L + 3) if backend == "emu" else (H + L + 6)
    sig = _noise(1, age + n_after, 21)[0]
    xs = _noise(2, age, 22)
    xs[1] = sig[: age * HOP]
    xd = _noise(2, tp + n_after, 23)
    src, dst = DfStream(model, df_state, streams=2), DfStream(model, df_state, streams=2)
    y_src = torch.cat([src.process(_hop(xs, k)) for k in range(age)], 1).cpu().numpy()
    y_before = [dst.process(_hop(xd, k)) for k in range(tp)]
    snap = src.export_streams([1])
    assert snap.ages.tolist() == [age]
    dst.import_streams([0], snap)
    assert dst.frames.tolist() == [age, tp]
    xd[0, tp * HOP:] = sig[age * HOP:]
    y_dst = torch.cat(y_before + [dst.process(_hop(xd, tp + k)) for k in range(n_after)], 1).cpu().numpy()
    assert dst.frames.tolist() == [age + n_after, tp + n_after]
    err = rms(np.concatenate([y_src[1], y_dst[0, tp * HOP:]]) - _fresh_stream_oracle(p, sd, sig))
    other = rms(y_dst[1] - _fresh_stream_oracle(p, sd, xd[1]))
    print(f"{name}/{case}: moved stream vs oracle {err:.3e}, the destination's other stream {other:.3e}")
    assert err < BAR, err
    assert other < BAR, other
    if tp == 0:
        assert float(np.abs(y_dst[1, : L * HOP]).max()) == 0.0
    model.check()


# ---- 4. gated continuation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["silent", "df-skipped"])
@pytest.mark.parametrize("name", ["pf32", "df3", "defaults"])
def test_gated_stream_moves_mid_stretch(backend, name, where):
    """gating=True, test_streaming_gated.py's signals and thresholds.  silent: stream 1 moves in the middle of its frozen stretch (counter
    above 5, flags set, nothing processed); df-skipped: a stream moves between two hops whose positions skip stage 2 (the DF decoder's
    state and delay line stand still while the rest advances).  Output 1e-6, lsnr 1e-3 against oracle/stream_oracle.py on the whole
    signal, frozen hops -15 dB and zeros — test_streaming_gated.py's tolerances."""
    from deepfilternet_amd.streaming import DfStream

    _emu_only_pf32(backend, name)
    if emu_subset(backend):
        pytest.skip("interpreter subset: the gated forms move on the GPU (DFX_EMU_ALL=1 runs them here too)")
    p, sd, model, df_state = _model(name)
    H, L = _window(p)
    T = 24
    if where == "silent":   # (the first of test_streaming_gated.py's threshold sets under which stream 1 has a frozen stretch of four hops)
        i = 1
        for quantiles in ((0.15, 0.85, 0.5), (0.0, 0.3, 0.15)):
            x, thr, ref = _gated_scenario(name, T, quantiles)
            acc = ref[1][2]["accepted"]
            spots = [a for a in range(2, T - 2) if all(b not in acc for b in (a - 2, a - 1, a, a + 1))]
            if spots:
                break
        t = spots[0]
    else:
        x, thr, ref = _gated_scenario(name, T)
        i, t = next((i, ref[i][2]["accepted"][q + L]) for i in (0, 2, 1) for q in range(H + L, len(ref[i][2]["flags"]) - 1)
                    if not ref[i][2]["flags"][q - 1][2] and not ref[i][2]["flags"][q][2] and ref[i][2]["flags"][q][0]
                    and ref[i][2]["accepted"][q + L] - 1 == ref[i][2]["accepted"][q + L - 1])
    yr, lr, info = ref[i]
    tp = t + 3
    xd = _noise(3, tp + T - t, 31)
    mk = lambda: DfStream(model, df_state, streams=3, gating=True, thresholds=thr)   # noqa: E731
    src, dst = mk(), mk()
    outs = [src.process(_hop(x, k), return_lsnr=True) for k in range(t)]
    for k in range(tp):
        dst.process(_hop(xd, k))
    dst.import_streams([2], src.export_streams([i]))
    xd[2, tp * HOP:] = x[i, t * HOP:]
    outs += [tuple(v[2:3] for v in dst.process(_hop(xd, tp + k), return_lsnr=True)) for k in range(T - t)]
    y = np.concatenate([o[0][i if k < t else 0].cpu().numpy() for k, o in enumerate(outs)])
    lsnr = np.concatenate([o[1][i if k < t else 0].cpu().numpy() for k, o in enumerate(outs)])
    err = rms(y - yr)
    print(f"{name}/{where}: stream {i} moved at hop {t}: output vs oracle {err:.3e}")
    assert err < 1e-6, err
    acc = info["accepted"]
    live = np.zeros(T, bool)
    live[acc[L:]] = True
    assert np.abs(lsnr - lr)[live].max() < 1e-3
    frozen = np.ones(T, bool)
    frozen[acc] = False
    assert np.all(lsnr[frozen] == -15.0) and np.all(y.reshape(T, HOP)[frozen] == 0.0)
    if where == "silent":
        assert frozen[t - 1] and frozen[t]
    model.check()


# ---- 5. settings ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_settings", [True, False])
def test_settings_travel_when_asked(backend, with_settings):
    """Twin 2-stream handles on the same input; A's stream 1 has a 12 dB limit, its own beta and thresholds, A' has none.  After the move
    with settings=True A' reports A's settings for the stream and its output is A's, in bits (the limit is applied: it differs from the
    unlimited run); with settings=False the slot keeps its own settings and the output is the unlimited run's, in bits, from the second hop
    after the move on: the inputs are the same, so the state that travelled is the state the slot had, except the synthesis overlap memory
    (fft - hop samples = one hop), which holds the tail of A's limited frame."""
    from deepfilternet_amd.streaming import DfStream

    if emu_subset(backend) and not with_settings:
        pytest.skip("interpreter subset: settings=True runs here (DFX_EMU_ALL=1 runs both)")
    p, sd, model, df_state = _model("pf32")
    t, T = 3, (6 if backend == "emu" else 12)
    x = _noise(2, T, 41)
    A, Ap, plain = (DfStream(model, df_state, streams=2) for _ in range(3))
    A.set_atten_lim(12, streams=[1])
    A.set_post_filter_beta(0.05, streams=[1])
    A.set_thresholds(-12, 31, 21, streams=[1])
    ya, yp, yn = [], [], []
    for k in range(T):
        if k == t:
            Ap.import_streams([1], A.export_streams([1]), settings=with_settings)
        ya.append(A.process(_hop(x, k))), yp.append(Ap.process(_hop(x, k))), yn.append(plain.process(_hop(x, k)))
    ya, yp, yn = (torch.cat(v, 1).cpu().numpy() for v in (ya, yp, yn))
    sa, sp, sn = A.settings, Ap.settings, plain.settings
    assert rms(ya[1, t * HOP:] - yn[1, t * HOP:]) > 1e-3 * rms(yn[1])   # the limit is heard
    for key in sa:
        assert torch.equal(sp[key][0], sn[key][0])
        assert torch.equal(sp[key][1], (sa if with_settings else sn)[key][1]), key
    assert float(sa["atten_lim_db"][1]) == 12.0
    assert p.fft_size - p.hop_size <= HOP
    first = t if with_settings else t + 1   # (settings=False: hop t overlaps A's last limited frame)
    assert np.array_equal(yp[1, first * HOP:], (ya if with_settings else yn)[1, first * HOP:])
    assert np.array_equal(yp[0], yn[0])
    model.check()


# ---- 6. host round trip, and growing a handle -------------------------------------------------------------------------------------------------
def test_snapshot_through_a_file_and_into_a_bigger_handle(backend, tmp_path):
    """snap.cpu() -> torch.save / torch.load of its state_dict -> .to(device) -> import: the same bits as importing the original.  And
    the three lines that grow a handle: every stream of a 2-stream handle continues in a fresh 4-stream one within 1e-6 of its oracle."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.streaming import DfStream, StreamSnapshot

    p, sd, model, df_state = _model("pf32")
    H, L = _window(p)
    t, n_after = H + L + 2, (3 if backend == "emu" else 8)
    x = _noise(2, t + n_after, 51)
    src = DfStream(model, df_state, streams=2)
    y_src = torch.cat([src.process(_hop(x, k)) for k in range(t)], 1).cpu().numpy()
    snap = src.export_streams()
    assert len(snap) == 2 and snap.payload.shape == (2, src.snapshot_bytes) and snap.ages.tolist() == [t, t]
    path = tmp_path / "streams.pt"
    torch.save(snap.cpu().state_dict(), path)
    back = StreamSnapshot.from_state_dict(torch.load(path)).to(_lib.device())
    assert torch.equal(back.payload.cpu(), snap.payload.cpu()) and torch.equal(back.meta, snap.meta)
    big, big2 = DfStream(model, df_state, streams=4), DfStream(model, df_state, streams=4)
    big.import_streams([0, 1], snap)
    big2.import_streams(range(2), back)
    xb = _noise(4, n_after, 52)
    xb[:2] = x[:, t * HOP:]
    y = torch.cat([big.process(_hop(xb, k)) for k in range(n_after)], 1).cpu().numpy()
    y2 = torch.cat([big2.process(_hop(xb, k)) for k in range(n_after)], 1).cpu().numpy()
    assert np.array_equal(y, y2)
    assert big.frames.tolist() == [t + n_after, t + n_after, n_after, n_after]
    for i in range(2):
        err = rms(np.concatenate([y_src[i], y[i]]) - _fresh_stream_oracle(p, sd, x[i]))
        assert err < BAR, (i, err)
    for i in (2, 3):
        assert rms(y[i] - _fresh_stream_oracle(p, sd, xb[i])) < BAR
    model.check()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(backend):
    """Every refused import (and export) leaves the handle as it was: after all of them a process call gives the bits of an untouched twin."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.streaming import DfStream, StreamSnapshot

    p, sd, model, df_state = _model("pf32")
    _, _, model2, df_state2 = _model("pf32_nopf")
    x = _noise(2, 4, 61)
    dst, twin = DfStream(model, df_state, streams=2), DfStream(model, df_state, streams=2)
    for k in range(3):
        dst.process(_hop(x, k)), twin.process(_hop(x, k))
    good = DfStream(model, df_state, streams=3).export_streams([0, 2])
    lib, ids = _lib.lib(), torch.tensor([0, 1], dtype=torch.int64)
    idp = C.cast(ids.data_ptr(), C.POINTER(C.c_int64))

    def refused(snap, to=(0, 1), codes=(1,), match=None):
        with pytest.raises((_lib.DfxError, ValueError)) as e:
            dst.import_streams(list(to), snap)
        if isinstance(e.value, _lib.DfxError):
            assert e.value.code in codes, e.value
            assert match is None or match in str(e.value), e.value

    def refused_raw(snap, code, match):
        """straight at the C entry point, with a payload as large as the destination's records (the Python layer checks sizes first)"""
        n = max(int(snap.payload.shape[1]), dst.snapshot_bytes)
        buf = torch.zeros((2, n), dtype=torch.uint8, device=_lib.device())
        assert lib.dfx_stream_import_streams(dst._h, idp, 2, _lib.ptr(buf), C.c_void_p(snap.meta.data_ptr()), 1, _lib.stream()) == code
        assert match in lib.dfx_last_error().decode()

    others = {
        "another model": DfStream(model2, df_state2, streams=2),
        "gated into ungated": DfStream(model, df_state, streams=2, gating=True),
        "pausable into plain": DfStream(model, df_state, streams=2, pausable=True),
        "sr=16000 into none": DfStream(model, df_state, streams=2, sr=16000),
        "channels": DfStream(model, df_state, streams=4, channels=2),
    }
    for what, rt in others.items():
        snap = rt.export_streams([0, 1])
        refused(snap, match="fingerprint")
        refused_raw(snap, 1, "fingerprint")
    refused(StreamSnapshot(good.payload[:, :-16].contiguous(), good.meta))                       # truncated payload
    bad = good.meta.clone()
    bad[1, 4] += 1
    refused(StreamSnapshot(good.payload, bad), codes=(2,), match="version")
    bad = good.meta.clone()
    bad[0, 0] ^= 0xFF
    refused(StreamSnapshot(good.payload, bad), match="magic")
    refused(good, to=(0, 2), match="not in")
    refused(good, to=(-1, 0), match="not in")
    refused(good, to=(1, 1), match="twice")
    with pytest.raises(ValueError):
        dst.import_streams([0], good)                                                           # two entries, one index
    meta_p, pay_p = C.c_void_p(good.meta.data_ptr()), _lib.ptr(good.payload)
    assert lib.dfx_stream_import_streams(dst._h, None, 2, pay_p, meta_p, 1, _lib.stream()) == 1
    assert lib.dfx_stream_import_streams(dst._h, idp, 2, None, meta_p, 1, _lib.stream()) == 1
    assert lib.dfx_stream_import_streams(dst._h, idp, 2, pay_p, None, 1, _lib.stream()) == 1
    assert lib.dfx_stream_import_streams(None, idp, 2, pay_p, meta_p, 1, _lib.stream()) == 1
    assert lib.dfx_stream_export_streams(dst._h, idp, 2, None, meta_p, _lib.stream()) == 1
    assert lib.dfx_stream_snapshot_bytes(dst._h, None) == 1
    with pytest.raises(_lib.DfxError):
        dst.export_streams([2])
    dst.set_atten_lim(0.0)                                                                      # the handle-wide pass-through: the one excluded mode
    for call in (lambda: dst.import_streams([0, 1], good), lambda: dst.export_streams([0])):
        with pytest.raises(_lib.DfxError) as e:
            call()
        assert e.value.code == 2 and "pass-through" in str(e.value)
    dst.set_atten_lim(100.0)
    assert dst.frames.tolist() == twin.frames.tolist() == [3, 3]
    assert torch.equal(dst.process(_hop(x, 3)), twin.process(_hop(x, 3)))
    dst.import_streams([], StreamSnapshot(good.payload[:0], good.meta[:0]))                     # an empty list is a no-op
    model.check()


def test_new_symbols_are_declared_bound_and_exported():
    import os
    import re

    from deepfilternet_amd import _lib
    from deepfilternet_amd.build import build
    from deepfilternet_amd.streaming import StreamSnapshot
    from tests.hipemu.build_emu import build as emu_build

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(repo, "include", "dfx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for lib_path in (build(), emu_build()):
        lib = C.CDLL(lib_path)
        for name in ("dfx_stream_snapshot_bytes", "dfx_stream_export_streams", "dfx_stream_import_streams"):
            assert re.search(r"\b%s\s*\(" % name, header), name
            assert name in _lib.SIGNATURES and hasattr(lib, name), (name, lib_path)
    assert "dfx_stream_meta" in header and re.search(r"weights are not\s+\*?\s*fingerprinted", raw, flags=re.I)

    class Meta(C.Structure):   # the header's struct, field by field
        _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("fingerprint", C.c_uint64), ("age", C.c_int64), ("settings", C.c_float * 5),
                    ("pending_current", C.c_int32)]

    assert C.sizeof(Meta) == StreamSnapshot.META_BYTES and Meta.age.offset == 16


# ---- 8. the steady state is untouched -------------------------------------------------------------------------------------------------------
def test_steady_call_after_an_import_enqueues_what_it_did(backend):
    """H + L + 1 hops after an import the destination's call has the window-copy launches (test_stream_slots._copy_launches' count) of a
    handle that never imported, and the same bits for its other stream; inside the H + L hops it may differ."""
    from deepfilternet_amd import _lib
    from deepfilternet_amd.streaming import DfStream

    if emu_subset(backend):
        pytest.skip("interpreter subset: the launch counts are read on the GPU (DFX_EMU_ALL=1 runs this here too)")
    p, sd, model, df_state = _model("pf32")
    H, L = _window(p)
    t = H + L + 1
    T = t + H + L + 3
    x = _noise(2, T, 71)
    src = DfStream(model, df_state, streams=2)
    for k in range(4):
        src.process(_hop(x, k))
    snap = src.export_streams([0])
    counts = {}
    outs = {}
    for moved in (True, False):
        rt = DfStream(model, df_state, streams=2)
        counts[moved], outs[moved] = [], []
        _lib.prof_enable(["dfx_k_copy_rows"])
        try:
            for k in range(T):
                if moved and k == t:
                    rt.import_streams([0], snap)
                _lib.prof_reset()
                outs[moved].append(rt.process(_hop(x, k)))
                counts[moved].append(_lib.prof_read().get("dfx_k_copy_rows", (0.0, 0))[1])
        finally:
            _lib.prof_enable(None)
    print(f"window-copy launches per call: with the import {counts[True]}, without {counts[False]}")
    assert counts[True][t + H + L + 1:] == counts[False][t + H + L + 1:] and len(counts[True][t + H + L + 1:]) >= 1
    assert counts[True][:t] == counts[False][:t]
    assert torch.equal(torch.cat(outs[True], 1)[1], torch.cat(outs[False], 1)[1])
    model.check()
