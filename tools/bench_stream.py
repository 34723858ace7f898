#!/usr/bin/env python3
"""Streaming throughput (BASELINE.json configs[3]-style: many concurrent real-time streams, frame by frame) on one MI355X.

    python tools/bench_stream.py [--streams 4096] [--frames-per-call 1 4 16] [--calls 200] [--gating] [--churn K] [--exact] [--paused FRACTION]
                                  [--per-stream-settings] [--sr 16000] [--pcm16 | --g711 {ulaw,alaw}] [--move]

--churn K: K streams start over before every call (DfStream.reset(ids)), rotating through the pool: the hop time of a service whose
callers come and go.
--paused FRACTION: a pausable handle (DfStream(pausable=True)); every call pauses that share of the streams, a block that rotates through
the pool (0: a pausable handle on which nobody pauses).
--per-stream-settings: every stream gets its own attenuation limit and post-filter beta (and, with --gating, thresholds) before the first call
(DfStream.set_*(..., streams=ids)); the JSON line also carries the host time of one setter call over all ids (setter_host_ms).
--sr RATE: the handle takes and returns hops at RATE (DfStream(sr=RATE): an up-sampler in front of the 48 kHz pass, a down-sampler behind it);
--pcm16: the hops are int16 PCM in both directions; --g711 LAW: uint8 G.711 codes of that law (DfStream(law=LAW): an RTP payload's bytes).  The JSON
line carries all three; without them the call is the plain 48 kHz float one.
--move: after the steady hops, 256 streams and then all of them are exported from the handle and imported into a second one of the same size
(DfStream.export_streams / import_streams); a further JSON line carries the device time of each (hipEvents on the caller's stream, median of
5), the record size and the bytes/s they reach against the 8 TB/s HBM peak, next to the steady hop time of the same run.  Each is timed twice:
into an empty queue (`*_ms`: what a caller that waits sees, host enqueue of the launches included) and behind a queued hop of the other handle's
size (`*_queued_ms`: the launches are already enqueued when the device reaches them — the device time of the copy kernels alone).
--exact: the model is created under DFX_EXACT_FP32=1 (every contraction in fp32: the one-hop GRU layers on dfx_k_gru_step_x32).

Prints one JSON line per frames-per-call setting: hops/s over all streams, ms per call, and the number of real-time 48 kHz streams
one GPU sustains at that call size (a stream needs 100 hops/s)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--frames-per-call", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--model", default="df3", choices=["df3", "df3_ll", "defaults"],
                    help="df3_ll: DeepFilterNet3 without lookahead (the reference's low-latency LADSPA model, ladspa/README.md:3)")
    ap.add_argument("--gating", action="store_true", help="per-stream stage gating + silent-input shortcut (tract.rs:513-525,658-672)")
    ap.add_argument("--churn", type=int, default=0, help="reset this many streams before every call, rotating through the pool")
    ap.add_argument("--paused", type=float, default=None, metavar="FRACTION",
                    help="pausable handle; this share of the streams (a rotating block) sits every call out")
    ap.add_argument("--per-stream-settings", action="store_true",
                    help="a distinct attenuation limit and post-filter beta per stream (with --gating also thresholds), set per stream")
    ap.add_argument("--sr", type=int, default=None, help="the callers' sample rate (hops of hop * sr / 48000 samples; default: the model's 48 kHz)")
    ap.add_argument("--pcm16", action="store_true", help="int16 PCM hops in and out")
    ap.add_argument("--g711", choices=["ulaw", "alaw"], default=None, help="uint8 G.711 hops in and out, of this law")
    ap.add_argument("--move", action="store_true", help="also time export_streams / import_streams of 256 and of all streams into a second handle")
    ap.add_argument("--exact", action="store_true", help="exact fp32 arithmetic (DFX_EXACT_FP32=1) instead of the fp16-split default")
    args = ap.parse_args()
    if args.pcm16 and args.g711:
        ap.error("--pcm16 and --g711 exclude each other")
    if args.exact:
        os.environ["DFX_EXACT_FP32"] = "1"   # read when the model is created
    from deepfilternet_amd import _lib
    from deepfilternet_amd.config import ModelParams
    from deepfilternet_amd.enhance import init_df
    from deepfilternet_amd.state_dict import random_state_dict
    from deepfilternet_amd.streaming import DfStream

    p = ModelParams.defaults() if args.model == "defaults" else ModelParams.deepfilternet3()
    if args.model == "df3_ll":
        p.conv_lookahead = p.df_lookahead = 0
    model, df_state, _, _ = init_df(params=p, state_dict=random_state_dict(p, 0), epoch="none")
    exact = bool(model.query(model.Q_EXACT_FP32))
    dev = _lib.device()
    for n in args.frames_per_call:
        rt = DfStream(model, df_state, streams=args.streams, max_frames=n, gating=args.gating, pausable=args.paused is not None, sr=args.sr, law=args.g711)
        hop = rt.frame_length
        x = 0.1 * torch.randn((args.streams, n * hop), device=dev)
        if args.pcm16:
            x = (x * 32768.0).to(torch.int16)
        if args.g711:
            from deepfilternet_amd.io import float_to_g711

            x = float_to_g711(x, args.g711)
        nslots, churn_pos = args.streams, 0

        def churn():   # the next K slots of the pool get a new caller
            nonlocal churn_pos
            if args.churn > 0:
                rt.reset([(churn_pos + k) % nslots for k in range(args.churn)])
                churn_pos = (churn_pos + args.churn) % nslots

        setter_ms = None
        if args.per_stream_settings:   # streams distinct values each; the host time of a setter call over all ids = median of 5 calls
            ids = torch.arange(args.streams)
            lims = (6.0 + 24.0 * torch.arange(args.streams) / args.streams).tolist()
            betas = (0.01 + 0.04 * torch.arange(args.streams) / args.streams).tolist()
            times = []
            for _ in range(5):
                t = time.perf_counter()
                rt.set_atten_lim(lims, streams=ids)
                times.append((time.perf_counter() - t) * 1e3)
            setter_ms = sorted(times)[2]
            rt.set_post_filter_beta(betas, streams=ids)
            if args.gating:
                k = torch.arange(args.streams) / args.streams
                rt.set_thresholds((-12.0 + 4.0 * k).tolist(), (28.0 + 4.0 * k).tolist(), (18.0 + 4.0 * k).tolist(), streams=ids)
        n_paused, pause_pos = int(round((args.paused or 0.0) * args.streams)), 0

        def mask():   # the next block of the pool sits this call out (a host array: the mask travels as kernel arguments)
            nonlocal pause_pos
            if args.paused is None:
                return None
            m = torch.ones(args.streams, dtype=torch.bool)
            idx = (pause_pos + torch.arange(n_paused)) % nslots
            m[idx] = False
            pause_pos = (pause_pos + n_paused) % nslots
            return m

        for _ in range(10):
            churn()
            rt.process(x, active=mask())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev_sync = int(os.environ.get("DFX_BENCH_DEV_SYNC", "0"))   # dev: the host waits after every n-th call (enqueue depth experiment)
        for i in range(args.calls):
            churn()
            y = rt.process(x, active=mask())
            if dev_sync and (i + 1) % dev_sync == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert y.dtype == x.dtype and (not y.is_floating_point() or torch.isfinite(y).all())
        # host cost of a call: 32 calls enqueued into empty queues, no wait in between (what bounds the rate on a box with a slow host)
        t1 = time.perf_counter()
        for i in range(32):
            y = rt.process(x, active=mask())
        host_ms = (time.perf_counter() - t1) / 32 * 1e3
        torch.cuda.synchronize()
        hops = args.streams * n * args.calls
        ms_call = dt / args.calls * 1e3
        print(json.dumps({"metric": "streaming 48 kHz hops/s over all streams", "value": hops / dt, "unit": "frames/s", "streams": args.streams,
                          "frames_per_call": n, "ms_per_call": ms_call, "host_ms_per_call": host_ms, "call_budget_ms": 10.0 * n,
                          "realtime_streams_per_gpu": int(hops / dt / 100.0), "model": args.model, "gating": bool(args.gating), "churn": args.churn, "paused": args.paused, "exact_fp32": exact,
                          "per_stream_settings": bool(args.per_stream_settings), "setter_host_ms": setter_ms, "sr": rt.sr, "pcm16": bool(args.pcm16), "g711": args.g711,
                          "resample_delay_ms": rt.resample_delay / rt.sr * 1e3,
                          "algorithmic_latency_ms": (p.fft_size - p.hop_size + rt.delay_frames * p.hop_size) / p.sr * 1e3}), flush=True)
        if args.move:
            other = DfStream(model, df_state, streams=args.streams, max_frames=n, gating=args.gating, pausable=args.paused is not None, sr=args.sr, law=args.g711)
            other.process(x)
            rec = rt.snapshot_bytes
            move = {"metric": "moving streams between handles", "streams": args.streams, "frames_per_call": n, "model": args.model, "record_bytes": rec,
                    "steady_ms_per_call": ms_call, "hbm_peak_bytes_per_s": 8e12}

            def dev_ms(fn, behind=None):   # median of 5, hipEvents on the caller's stream; behind: a handle whose hop is enqueued first
                times = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    if behind is not None:
                        behind.process(x)
                    e0.record()
                    r = fn()
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
                return sorted(times)[2], r

            for count in sorted({min(256, args.streams), args.streams}):
                ids = torch.arange(count)
                ex_ms, snap = dev_ms(lambda: rt.export_streams(ids))
                im_ms, _ = dev_ms(lambda: other.import_streams(ids, snap, settings=False))
                exq_ms, _ = dev_ms(lambda: rt.export_streams(ids), behind=other)
                imq_ms, _ = dev_ms(lambda: other.import_streams(ids, snap, settings=False), behind=rt)
                move[f"export_{count}_queued_ms"], move[f"import_{count}_queued_ms"] = exq_ms, imq_ms
                move[f"export_{count}_queued_bytes_per_s"], move[f"import_{count}_queued_bytes_per_s"] = 2 * count * rec / (exq_ms * 1e-3), 2 * count * rec / (imq_ms * 1e-3)
                # a record is read once and written once in either direction
                move[f"export_{count}_ms"], move[f"import_{count}_ms"] = ex_ms, im_ms
                move[f"export_{count}_bytes_per_s"], move[f"import_{count}_bytes_per_s"] = 2 * count * rec / (ex_ms * 1e-3), 2 * count * rec / (im_ms * 1e-3)
                del snap
            y = other.process(x)
            torch.cuda.synchronize()
            assert not y.is_floating_point() or torch.isfinite(y).all()
            print(json.dumps(move), flush=True)
            del other
        del rt


if __name__ == "__main__":
    main()
