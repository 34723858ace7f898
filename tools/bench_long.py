#!/usr/bin/env python3
"""Clips of any length on one MI355X (enhance_long: time-chunked stream passes with exact clip ends), DeepFilterNet3 shape, seeded weights
and inputs, device-resident clips.  One JSON line per measurement; wall-clock time around a synchronised call (the path's host work — slot
bookkeeping, one Python call per chunk — is part of what is measured), after one warm-up call:
  sweep   hops_per_call 128 / 256 / 512 / 1024 at 256 slots, 256 clips x --sweep-seconds, float and 16-bit: frames/s (enhance._LONG_HOPS is chosen from it)
  cost    the bench workload, 256 x 10 s: enhance() and enhance_long alternating, three runs each — frames/s and their ratio
  corpus  64 clips x 10 min under DFX_WORKSPACE_CAP_GB=24: enhance_batch (sub-batches of whole clips) against enhance_long — frames/s, device bytes
  single  one clip of 3 h under the same cap: enhance_long's time and device bytes (enhance() alone needs more workspace than the cap)
    python tools/bench_long.py [--only sweep,cost,corpus,single]"""
import argparse
import json
import os
import statistics
import sys
import time

if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 24:   # one hardware queue per engine stream, as bench.py
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

SR = 48000


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def noise(shape, g, dev, pcm16=False):
    """0.1 * standard_normal of that shape, made on the device row by row"""
    out = torch.empty(shape, dtype=torch.int16 if pcm16 else torch.float32, device=dev)
    for row in out.view(-1, shape[-1]):
        v = torch.randn((shape[-1],), generator=g, device=dev).mul_(0.1)
        row.copy_(v.mul_(32768).to(torch.int16) if pcm16 else v)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", default="sweep,cost,corpus,single")
    ap.add_argument("--sweep-seconds", type=int, default=60)
    ap.add_argument("--corpus-minutes", type=int, default=10)
    ap.add_argument("--single-hours", type=float, default=3.0)
    ap.add_argument("--cap-gb", type=float, default=24.0)
    args = ap.parse_args()
    only = set(args.only.split(","))
    from deepfilternet_amd import _lib
    from deepfilternet_amd import enhance as E
    from deepfilternet_amd.config import ModelParams

    torch.cuda.set_device(0)
    p = ModelParams.deepfilternet3()
    model, df_state, _, _ = E.init_df(params=p, epoch="none", seed=0)
    dev = _lib.device()
    hop, n_fft = df_state.hop_size(), df_state.fft_size()
    g = torch.Generator(device=dev).manual_seed(0)

    def frames(clips):
        return sum(c.shape[0] * ((c.shape[1] + n_fft) // hop) for c in clips)

    if "sweep" in only:
        for pcm16 in (False, True):
            x = noise((256, args.sweep_seconds * SR), g, dev, pcm16)
            clips = [x[i:i + 1] for i in range(256)]
            for hops in (128, 256, 512, 1024):
                E.enhance_long(model, df_state, clips[:16], hops_per_call=hops)   # (warm-up)
                runs = [wall(lambda: E.enhance_long(model, df_state, clips, slots=256, hops_per_call=hops))[0] for _ in range(3)]
                s = statistics.median(runs)
                print(json.dumps({"measurement": "sweep", "format": "pcm16" if pcm16 else "f32", "slots": 256, "hops_per_call": hops,
                                  "clips": 256, "seconds": args.sweep_seconds, "s_median": round(s, 4), "s": [round(r, 4) for r in runs],
                                  "frames_per_s": round(frames(clips) / s), "plan": dict(E.last_long_plan)}), flush=True)
            del x, clips
        model.check()
    if "cost" in only:
        x = noise((256, 10 * SR), g, dev)
        E.enhance(model, df_state, x), E.enhance_long(model, df_state, [x])
        a, b = [], []
        for _ in range(3):
            a.append(wall(lambda: E.enhance(model, df_state, x))[0])
            b.append(wall(lambda: E.enhance_long(model, df_state, [x]))[0])
        fa, fb = frames([x]) / statistics.median(a), frames([x]) / statistics.median(b)
        print(json.dumps({"measurement": "cost", "clips": 256, "seconds": 10, "enhance_s": [round(v, 4) for v in a],
                          "enhance_long_s": [round(v, 4) for v in b], "enhance_frames_per_s": round(fa), "enhance_long_frames_per_s": round(fb),
                          "long_over_enhance": round(fb / fa, 4), "plan": dict(E.last_long_plan)}), flush=True)
        del x
        model.check()
    if only & {"corpus", "single"}:
        os.environ["DFX_WORKSPACE_CAP_GB"] = repr(args.cap_gb)
        model._ws = None
        torch.cuda.empty_cache()
    if "corpus" in only:
        x = noise((64, args.corpus_minutes * 60 * SR), g, dev)
        clips = [x[i:i + 1] for i in range(64)]
        res = {}
        for name, fn in (("enhance_batch", E.enhance_batch), ("enhance_long", E.enhance_long)):
            fn(model, df_state, clips[:2])   # (warm-up)
            model._ws = None
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            s, out = wall(lambda: fn(model, df_state, clips))
            res[name] = {"s": round(s, 3), "frames_per_s": round(frames(clips) / s),
                         # what the call held on top of the clips: torch's peak (workspace, packed rows, results) and, for enhance_long, the handle
                         "torch_peak_bytes": int(torch.cuda.max_memory_allocated() - base),
                         "handle_bytes": int(E.last_long_plan.get("bytes", 0)) if name == "enhance_long" else 0}
            if name == "enhance_long":
                res[name]["plan"] = dict(E.last_long_plan)
            del out
        print(json.dumps({"measurement": "corpus", "clips": 64, "minutes": args.corpus_minutes, "cap_gb": args.cap_gb, **res,
                          "long_over_batch": round(res["enhance_long"]["frames_per_s"] / res["enhance_batch"]["frames_per_s"], 3)}), flush=True)
        del x, clips
        model.check()
    if "single" in only:
        x = noise((1, int(args.single_hours * 3600) * SR), g, dev)
        model._ws = None
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        E.last_long_plan.clear()
        s, out = wall(lambda: E.enhance(model, df_state, x))   # (routed: one clip's workspace is above the cap)
        assert E.last_long_plan, "the clip fitted the cap: not the long path"
        print(json.dumps({"measurement": "single", "hours": args.single_hours, "cap_gb": args.cap_gb, "s": round(s, 3),
                          "frames_per_s": round(frames([x]) / s), "realtime_factor": round(x.shape[1] / SR / s, 1),
                          "torch_peak_bytes": int(torch.cuda.max_memory_allocated() - base), "handle_bytes": int(E.last_long_plan["bytes"]),
                          "plan": dict(E.last_long_plan)}), flush=True)
        del out, x
        model.check()


if __name__ == "__main__":
    main()
