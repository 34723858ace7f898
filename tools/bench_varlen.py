#!/usr/bin/env python3
"""Clips of different lengths on one MI355X (dfx_enhance_varlen / enhance_batch), DeepFilterNet3 shape, seeded weights and inputs.  One JSON line
per measurement, device-event timing after warm-up:
  mixed   512 clips of 1-12 s at 48 kHz (uniform lengths, seeded) resident in HBM: the per-clip enhance() loop against enhance_batch — clips/s,
          audio-seconds/s, passes, the padded share of the frames the passes run
  equal   256 x 10 s through dfx_enhance and through dfx_enhance_varlen with all lengths equal, alternated call by call: the varlen path's overhead
  budget  enhance_batch's rows per pass (enhance._BATCH_ROWS) 128 / 256 / 512 on the mixed set
    python tools/bench_varlen.py [--only mixed,equal,budget] [--reps N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 24:   # one hardware queue per engine stream, as bench.py
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

SR = 48000


def timed(fn, reps, warm=1):
    """ms per call of fn: device events around reps calls, after warm calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def padded_share(E, model, df_state, lens, hop, n_fft):
    """(passes, share of the frames the passes run that lie behind a row's own end) for enhance_batch's plan of these rows"""
    lens = sorted(lens, reverse=True)
    passes = E._plan_passes(model, df_state, lens, True)
    run = own = 0
    for r0, n, _ in passes:
        tf = [(t + n_fft) // hop for t in lens[r0:r0 + n]]
        run += max(tf) * n
        own += sum(tf)
    return len(passes), 1.0 - own / run


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", default="mixed,equal,budget")
    ap.add_argument("--reps", type=int, default=5)
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
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(SR, 12 * SR + 1, (512,), generator=g).tolist()
    if only & {"mixed", "budget"}:
        clips = [(0.1 * torch.randn((1, n), generator=g)).to(dev) for n in lens]
        audio_s = sum(lens) / SR
    if "mixed" in only:
        for c in clips[:8]:
            E.enhance(model, df_state, c)   # (warm-up: every kernel of the small-pass path)
        ms_loop = timed(lambda: [E.enhance(model, df_state, c) for c in clips], 1, warm=0)
        ms_batch = timed(lambda: E.enhance_batch(model, df_state, clips), args.reps)
        model.check()
        npass, pad = padded_share(E, model, df_state, lens, hop, n_fft)
        print(json.dumps({"measurement": "mixed", "clips": len(clips), "audio_s": round(audio_s, 1), "rows_per_pass": E._BATCH_ROWS,
                          "per_clip_loop": {"ms": round(ms_loop, 1), "clips_per_s": round(len(clips) / ms_loop * 1e3, 1),
                                            "audio_s_per_s": round(audio_s / ms_loop * 1e3, 1)},
                          "enhance_batch": {"ms": round(ms_batch, 2), "clips_per_s": round(len(clips) / ms_batch * 1e3, 1),
                                            "audio_s_per_s": round(audio_s / ms_batch * 1e3, 1), "passes": npass, "padded_frame_share": round(pad, 4)},
                          "speedup_clips_per_s": round(ms_loop / ms_batch, 2)}), flush=True)
    if "equal" in only:
        B, T = 256, 10 * SR
        x = (0.1 * torch.randn((B, T), generator=g)).to(dev)
        y = torch.empty_like(x)
        L = _lib.lib()
        arr = (C.c_int64 * B)(*([T] * B))
        n1, n2 = C.c_int64(), C.c_int64()
        _lib.check(L.dfx_enhance_workspace_bytes(model.handle, df_state.handle, B, T, 1, C.byref(n1)))
        _lib.check(L.dfx_enhance_varlen_workspace_bytes(model.handle, df_state.handle, B, arr, 1, C.byref(n2)))
        ws = torch.empty(max(n1.value, n2.value), dtype=torch.uint8, device=dev)

        def uni():
            _lib.check(L.dfx_enhance(model.handle, df_state.handle, _lib.ptr(x), B, T, 1, 0.0, _lib.ptr(y), _lib.ptr(ws), ws.numel(), _lib.stream()))

        def var():
            _lib.check(L.dfx_enhance_varlen(model.handle, df_state.handle, _lib.ptr(x), B, T, arr, 1, 0.0, _lib.ptr(y), T, _lib.ptr(ws), ws.numel(),
                                            _lib.stream()))

        for _ in range(3):
            uni(), var()
        a, b = [], []
        for _ in range(max(args.reps, 5) * 2):
            a.append(timed(uni, 1, warm=0))
            b.append(timed(var, 1, warm=0))
        model.check()
        ma, mb = statistics.median(a), statistics.median(b)
        print(json.dumps({"measurement": "equal", "clips": B, "seconds": 10, "dfx_enhance_ms_median": round(ma, 3),
                          "dfx_enhance_varlen_ms_median": round(mb, 3), "varlen_over_uniform": round(mb / ma, 4),
                          "dfx_enhance_ms": [round(v, 3) for v in a], "dfx_enhance_varlen_ms": [round(v, 3) for v in b]}), flush=True)
    if "budget" in only:
        keep = E._BATCH_ROWS
        for rows in (128, 256, 512):
            E._BATCH_ROWS = rows
            ms = timed(lambda: E.enhance_batch(model, df_state, clips), args.reps)
            npass, pad = padded_share(E, model, df_state, lens, hop, n_fft)
            print(json.dumps({"measurement": "budget", "rows_per_pass": rows, "ms": round(ms, 2), "clips_per_s": round(len(clips) / ms * 1e3, 1),
                              "passes": npass, "padded_frame_share": round(pad, 4)}), flush=True)
        E._BATCH_ROWS = keep
        model.check()


if __name__ == "__main__":
    main()
