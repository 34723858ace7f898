"""Dev: the same work under two builds of the library (each in its own process), compared bit by bit.
    python tools/dev/lib_diff.py <libA.so|-> <libB.so|-> [clips [samples]]              enhance() of the same clips
    python tools/dev/lib_diff.py --stream <libA.so|-> <libB.so|-> [streams [hops]]      DfStream through a fixed script (STREAM_CASES):
        every call's audio and lsnr (process_raw: gains, coefficients, stages too) and every call's launch count per kernel, under
        DFX_STREAM_LINEAR=0 and =6, and the plain cases again under DFX_EXACT_FP32=1.  One line per case; exit status 1 on any difference.
        A library may be given as <label>=<path> (say parent@<commit>=...): the record then names the label, not a path of the machine."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CUTS = [1, 2, 1, 1, 3, 1, 1, 2, 1]
# case -> (DfStream arguments, what happens before call i).  Events: ("reset", ids), ("lim", dB[, ids]), ("beta", v, ids), ("thr", (a, b, c)[, ids]),
# ("pause", ids): this call only, ("raw", k): the next k hops go through process_raw.  Stream ids are taken modulo the number of streams.
STREAM_CASES = {
    "ungated": ({}, {}),
    "gated": ({"gating": True}, {}),
    "pausable": ({"pausable": True}, {3: [("pause", [1, 17])], 4: [("pause", [1, 17])], 9: [("pause", [0, 18])]}),
    "pausable_gated": ({"pausable": True, "gating": True}, {3: [("pause", [1, 17])], 4: [("pause", [1, 17])], 9: [("pause", [0, 18])]}),
    "reset_streams": ({}, {6: [("reset", [2, 16])], 11: [("reset", [0])]}),
    "reset_streams_gated": ({"gating": True}, {6: [("reset", [2, 16])], 11: [("reset", [0])]}),
    "pass_through": ({}, {7: [("lim", 0.0)], 9: [("lim", 100.0)]}),
    "pass_through_gated": ({"gating": True}, {7: [("lim", 0.0)], 9: [("lim", 100.0)]}),
    "per_stream_settings": ({"gating": True}, {2: [("lim", 12.0, [1, 16]), ("beta", 0.03, [2, 17])], 5: [("thr", None, [0, 3, 18])], 10: [("lim", 100.0)]}),
    "process_raw": ({"gating": True}, {8: [("raw", 3)]}),
}
EXACT_CASES = ("ungated", "gated")


def stream_child(out, streams, hops, exact):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    from deepfilternet_amd import _lib
    from deepfilternet_amd.config import ModelParams
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.state_dict import random_state_dict
    from deepfilternet_amd.streaming import DfStream

    p = ModelParams.defaults()   # the suite's "pf32" model: conv_ch 32, kt 3, lookahead 1, post filter
    p.mask_pf, p.df_lookahead, p.conv_lookahead = True, 1, 1
    p.df_gru_skip, p.df_pathway_kernel_size_t, p.conv_ch = "identity", 3, 32
    model, df_state, _, _ = init_df(params=p, state_dict=random_state_dict(p, 0), epoch="none")
    hop, N = p.hop_size, p.fft_size
    x = (0.1 * np.random.default_rng(1).standard_normal((streams, hops * hop))).astype(np.float32)
    x[streams // 2, 6 * hop:18 * hop] = 0.0   # digital silence: a gated handle freezes these streams after 5 hops
    x[streams - 1, 9 * hop:16 * hop] = 0.0
    x = torch.from_numpy(x)
    xp = torch.cat([torch.zeros(streams, N - hop), x], dim=1)
    spec = torch.fft.rfft(xp.unfold(1, N, hop) * torch.hann_window(N), dim=2).to(torch.complex64)
    cuts, pos = [], 0
    while pos < hops:
        cuts.append(min(CUTS[len(cuts) % len(CUTS)], hops - pos))
        pos += cuts[-1]
    res, thr = {}, None

    def drive(tag, kw, events):
        rt = DfStream(model, df_state, streams=streams, max_frames=3, thresholds=thr if kw.get("gating") else None, **kw)
        pos, raw_left, i = 0, 0, 0
        ids = lambda v: sorted({k % streams for k in v})
        _lib.prof_enable("all")
        while pos < hops:
            active = None
            for ev in events.get(i, ()):
                if ev[0] == "reset":
                    rt.reset(ids(ev[1]))
                elif ev[0] == "lim":
                    rt.set_atten_lim(ev[1], streams=ids(ev[2]) if len(ev) > 2 else None)
                elif ev[0] == "beta":
                    rt.set_post_filter_beta(ev[1], streams=ids(ev[2]))
                elif ev[0] == "thr":
                    t = ev[1] or (thr[0] - 1.0, thr[1] + 0.5, thr[2] - 0.5)
                    rt.set_thresholds(*t, streams=ids(ev[2]) if len(ev) > 2 else None)
                elif ev[0] == "pause":
                    active = torch.ones(streams, dtype=torch.bool)
                    active[ids(ev[1])] = False
                elif ev[0] == "raw":
                    raw_left = ev[1]
            _lib.prof_reset()
            if raw_left:
                n, outs = 1, rt.process_raw(spec[:, pos].contiguous())
                raw_left -= 1
            else:
                n = min(cuts[i % len(cuts)], hops - pos)
                outs = rt.process(x[:, pos * hop:(pos + n) * hop], return_lsnr=True, active=active)
            for j, o in enumerate(outs):
                o = o.cpu()
                res[f"{tag}/{i:02d}/{j}"] = (torch.view_as_real(o) if o.is_complex() else o).numpy()
            counts = {k: int(v[1]) for k, v in _lib.prof_read().items() if v[1]}
            res[f"{tag}/{i:02d}/launches"] = np.frombuffer(json.dumps(counts, sort_keys=True).encode(), dtype=np.uint8)
            pos += n
            i += 1
        _lib.prof_enable(None)

    for linear in ("0", "6"):
        os.environ["DFX_STREAM_LINEAR"] = linear   # read at every create
        for name, (kw, events) in STREAM_CASES.items():
            if exact and name not in EXACT_CASES:
                continue
            tag = f"{name} linear={linear}" + (" exact_fp32" if exact else "")
            drive(tag, kw, events)
            if thr is None:
                # thresholds inside the model's lsnr range (the ungated run's quantiles), so that stages really get skipped; max_db_erb below most
                # of what the silent stretches give: no gains there, so the skip counter passes 5 and those streams freeze
                lsnr = np.concatenate([v for k, v in res.items() if k.endswith("/1")], axis=1)
                q = lambda v, f: float(np.sort(v.ravel())[int(f * (v.size - 1))])
                quiet = np.concatenate([lsnr[streams // 2, 8:18], lsnr[streams - 1, 11:16]])
                thr = (q(lsnr[:, p.df_lookahead:], 0.15), q(quiet, 0.2), q(lsnr[:, p.df_lookahead:], 0.5))
                res["thresholds"] = np.asarray(thr)
    np.savez(out, **res)


def stream_main(la, lb, streams, hops):
    import numpy as np

    bits = lambda v: v.view(np.uint32) if v.dtype == np.float32 else v   # (a paused stream's lsnr is NaN: compared as bits)
    (la_name, la), (lb_name, lb) = [l.split("=", 1) if "=" in l else (l, l) for l in (la, lb)]
    tmp = tempfile.mkdtemp(prefix="lib_diff_")
    runs = []
    for exact in (False, True):
        pair = []
        for i, l in enumerate((la, lb)):
            env = dict(os.environ)
            env.pop("DFX_EXACT_FP32", None)
            if exact:
                env["DFX_EXACT_FP32"] = "1"   # read when the model is created
            if l != "-":
                env["DFX_LIBRARY"] = l
            f = os.path.join(tmp, f"stream_{i}_{int(exact)}.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--stream-child", f, str(streams), str(hops), str(int(exact))], env=env, check=True)
            pair.append(dict(np.load(f)))
        runs.append(pair)
    shutil.rmtree(tmp, ignore_errors=True)
    bad = 0
    print(f"DfStream, {streams} streams, {hops} hops: A = {la_name}, B = {lb_name}")
    for a, b in runs:
        assert a.keys() == b.keys()
        print("thresholds", a["thresholds"].tolist(), "equal" if np.array_equal(a["thresholds"], b["thresholds"]) else "DIFFERENT")
        for tag in dict.fromkeys(k.split("/")[0] for k in a if "/" in k):
            keys = [k for k in a if k.startswith(tag + "/")]
            data = [k for k in keys if not k.endswith("/launches")]
            calls = [k for k in keys if k.endswith("/launches")]
            diff = sum(int((bits(a[k]) != bits(b[k])).sum()) if a[k].shape == b[k].shape else a[k].size for k in data)
            nan = sum(int(np.isnan(a[k]).sum()) for k in data)
            same = [k for k in calls if a[k].tobytes() == b[k].tobytes()]
            la_n = [sum(json.loads(a[k].tobytes()).values()) for k in calls]
            lb_n = [sum(json.loads(b[k].tobytes()).values()) for k in calls]
            frozen = sum(int((a[k] == -15.0).sum()) for k in data if k.endswith("/1"))
            print(f"{tag}: calls {len(calls)} values {sum(a[k].size for k in data)} (NaN {nan}: paused lsnr; lsnr == -15: {frozen}) differing samples {diff}; "
                  f"launches A/B {sum(la_n)} {sum(lb_n)} per-call counts identical in {len(same)} of {len(calls)} calls")
            bad += diff + len(calls) - len(same)
    print("IDENTICAL" if not bad else "DIFFERENT")
    return 1 if bad else 0


if len(sys.argv) > 1 and sys.argv[1] == "--stream-child":
    stream_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] == "1")
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--stream":
    sys.exit(stream_main(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 19, int(sys.argv[5]) if len(sys.argv) > 5 else 24))
if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    from bench import synth_audio
    from deepfilternet_amd.config import ModelParams
    from deepfilternet_amd.enhance import enhance, init_df
    from deepfilternet_amd.state_dict import random_state_dict

    out, clips, samples = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    p = ModelParams.deepfilternet3()
    model, df_state, _, _ = init_df(params=p, state_dict=random_state_dict(p, 0), epoch="none")
    x = synth_audio(clips, samples, 100, torch.device("cuda"))
    y = enhance(model, df_state, x)
    torch.cuda.synchronize()
    np.save(out, y.cpu().numpy())
    sys.exit(0)

import numpy as np

(la_name, la), (lb_name, lb) = [l.split("=", 1) if "=" in l else (l, l) for l in sys.argv[1:3]]
print(f"enhance(): A = {la_name}, B = {lb_name}")
clips = int(sys.argv[3]) if len(sys.argv) > 3 else 37
samples = int(sys.argv[4]) if len(sys.argv) > 4 else 100001
ys = []
for i, l in enumerate((la, lb)):
    env = dict(os.environ)
    if l != "-":
        env["DFX_LIBRARY"] = l
    f = os.path.join(tempfile.mkdtemp(prefix="lib_diff_"), f"{i}.npy")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f, str(clips), str(samples)], env=env, check=True)
    ys.append(np.load(f))
a, b = ys
d = np.abs(a.astype(np.float64) - b.astype(np.float64))
print("shape", a.shape, "rms", float(np.sqrt((a.astype(np.float64) ** 2).mean())), "max abs diff", float(d.max()), "differing samples", int((a != b).sum()), "of", a.size)
if d.max() > 0:
    r, c = np.unravel_index(np.argmax(d), d.shape)
    print("worst at clip", r, "sample", c, "frame", c // 480, "pos in hop", c % 480, a[r, c], b[r, c])
    fr = np.nonzero((a != b).any(axis=0))[0] // 480
    print("frames with differences:", len(np.unique(fr)), "first", np.unique(fr)[:12])
    pos = np.bincount(np.nonzero(a != b)[1] % 480, minlength=480)
    print("positions in the hop with most differences:", np.argsort(-pos)[:8], pos.max(), pos.min())
