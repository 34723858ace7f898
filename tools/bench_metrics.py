#!/usr/bin/env python3
"""Time of scoring a batch on the device: STOI (df/stoi.py) plus SI-SDR of B clips x S seconds at 48 kHz, inputs resident.

    python tools/bench_metrics.py [--clips 256] [--seconds 10] [--sr 48000] [--steps 20] [--warmup 3]

Events are recorded around the two calls (workspaces allocated once, outside the timed region); the median and the spread over the steps are
reported, then the kernels' own times from one more step under dfx_prof_* (events around every launch: a separate pass, its launches do not
overlap).  The algorithmic traffic is the resampler's two reads of the inputs (2 signals x B x T x 4 bytes) plus SI-SDR's two passes over both;
achieved bytes per second are reported against each.  Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sr", type=int, default=48_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from deepfilternet_amd import _lib, metrics

    dev = _lib.device()
    B, T = args.clips, int(args.seconds * args.sr)
    g = torch.Generator(device="cpu").manual_seed(0)
    clean = torch.randn((B, T), generator=g).mul_(0.1)
    clean[:, T // 3: T // 2] *= 1e-4                     # a silent stretch, so that windows are removed
    degraded = (clean + 0.03 * torch.randn((B, T), generator=g)).to(dev)
    clean = clean.to(dev)
    lens = (C.c_int64 * B)(*([T] * B))
    need_a, need_b = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().dfx_stoi_workspace_bytes(args.sr, B, lens, C.byref(need_a)))
    _lib.check(_lib.lib().dfx_si_sdr_workspace_bytes(B, lens, C.byref(need_b)))
    ws = torch.empty(max(need_a.value, need_b.value), dtype=torch.uint8, device=dev)

    def step():
        return metrics.stoi(clean, degraded, args.sr, workspace=ws), metrics.si_sdr(clean, degraded, workspace=ws)

    for _ in range(args.warmup):
        st, sd = step()
    torch.cuda.synchronize()
    ms_all, ms_stoi = [], []
    for _ in range(args.steps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        st = metrics.stoi(clean, degraded, args.sr, workspace=ws)
        e1.record()
        sd = metrics.si_sdr(clean, degraded, workspace=ws)
        e2.record()
        torch.cuda.synchronize()
        ms_stoi.append(e0.elapsed_time(e1))
        ms_all.append(e0.elapsed_time(e2))
    _lib.prof_enable("all")
    _lib.prof_reset()
    step()
    torch.cuda.synchronize()
    kern = {k: round(v[0], 4) for k, v in _lib.prof_read().items()}
    _lib.prof_enable(None)
    med = statistics.median(ms_all)
    in_bytes = 2 * B * T * 4
    out = {
        "clips": B, "seconds": args.seconds, "sr": args.sr, "steps": args.steps,
        "ms_per_batch": round(med, 4), "ms_min": round(min(ms_all), 4), "ms_max": round(max(ms_all), 4),
        "ms_stoi": round(statistics.median(ms_stoi), 4), "ms_si_sdr": round(med - statistics.median(ms_stoi), 4),
        "kernel_ms": kern,
        "workspace_mb": round(ws.numel() / 2 ** 20, 1),
        "x_realtime": round(B * args.seconds / (med * 1e-3)),
        "stoi_input_gb_per_s": round(in_bytes / (statistics.median(ms_stoi) * 1e-3) / 1e9, 1),
        "resample_gb_per_s": round(in_bytes / (kern["dfx_k_resample"] * 1e-3) / 1e9, 1) if kern.get("dfx_k_resample") else None,
        "si_sdr_gb_per_s": round(2 * in_bytes / (kern["dfx_k_sisdr"] * 1e-3) / 1e9, 1) if kern.get("dfx_k_sisdr") else None,
        "stoi_mean": float(st.float().nanmean()), "si_sdr_mean": float(sd.mean()),
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
