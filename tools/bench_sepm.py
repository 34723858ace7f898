#!/usr/bin/env python3
"""Time of the composite measures' parts (df/sepm.py: segmental SNR, LLR, WSS, fwSNRseg) on the device: B clips x S seconds, inputs resident.

    python tools/bench_sepm.py [--clips 256] [--seconds 10] [--rates 16000,48000] [--steps 20] [--warmup 3]

Per rate: events are recorded around ``metrics.sepm`` (the workspace allocated once, outside the timed region); the median and the spread over
the steps are reported, then the kernels' own times from one more step under dfx_prof_* (events around every launch: a separate pass, its
launches do not overlap; ``dfx_k_sepm_spec`` includes the per-row reductions).  The CPU yardstick is the reference itself: 0.13 s per second of
16 kHz audio on one core (``sepm.py`` with a stub ``pesq``), which ``x_reference_core`` divides by.  Prints one JSON line per rate."""
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

REFERENCE_CORE_S_PER_S = 0.13


def run(sr: int, args) -> dict:
    from deepfilternet_amd import _lib, metrics

    dev = _lib.device()
    B, T = args.clips, int(args.seconds * sr)
    g = torch.Generator(device="cpu").manual_seed(0)
    clean = torch.randn((B, T), generator=g).mul_(0.1)
    clean[:, T // 3: T // 2] *= 1e-4
    processed = (clean + 0.03 * torch.randn((B, T), generator=g)).to(dev)
    clean = clean.to(dev)
    lens = (C.c_int64 * B)(*([T] * B))
    need = C.c_int64()
    _lib.check(_lib.lib().dfx_sepm_workspace_bytes(sr, B, lens, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    for _ in range(args.warmup):
        m = metrics.sepm(clean, processed, sr, dtype=torch.float64, workspace=ws)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = metrics.sepm(clean, processed, sr, dtype=torch.float64, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    _lib.prof_enable("all")
    _lib.prof_reset()
    metrics.sepm(clean, processed, sr, dtype=torch.float64, workspace=ws)
    torch.cuda.synchronize()
    kern = {k: round(v[0], 4) for k, v in _lib.prof_read().items()}
    _lib.prof_enable(None)
    med = statistics.median(ms)
    return {"clips": B, "seconds": args.seconds, "sr": sr, "steps": args.steps, "ms_per_batch": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "kernel_ms": kern, "workspace_mb": round(ws.numel() / 2 ** 20, 1),
            "x_realtime": round(B * args.seconds / (med * 1e-3)),
            "x_reference_core": round(B * args.seconds * REFERENCE_CORE_S_PER_S / (med * 1e-3)),
            "means": {k: float(v.nanmean()) for k, v in m.items()}}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rates", default="16000,48000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for sr in (int(v) for v in args.rates.split(",")):
        print(json.dumps(run(sr, args)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
