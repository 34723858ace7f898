#!/usr/bin/env python3
"""Throughput of the steps either side of enhance() (csrc/dfx_io.hip) on one MI355X: PCM16 -> float, 44.1 kHz -> 48 kHz sinc
resampling (df.io.resample, "sinc_fast"), float -> PCM16, on a batch of 256 clips x 10 s.  One JSON line per step.

``bench_io.py flac``: loading FLAC instead.  tests/golden/flac_noise_mono.flac (4.94 s, 48 kHz, 16 bits, mono) x 512 copies in one
``dfx_flac_decode`` call (2 528 s of audio: bench.py's 2 560 s within 1 %): the decode alone with the bytes resident, the upload of the
compressed bytes against the upload of the same audio as int16 (page-locked host memory), and the resident ``dfx_enhance_pcm16`` pass over
the decoded batch in the same process."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 24:   # one hardware queue per engine stream, as bench.py (the flac entry times enhance())
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio
    import ctypes as C

    dev = _lib.device()
    B, sr, new = 256, 44100, 48000
    T = sr * 10
    pcm = torch.randint(-20000, 20000, (B, T), dtype=torch.int16, device=dev)
    ms = timed(lambda: dio.pcm16_to_float(pcm))
    print(json.dumps({"step": "pcm16_to_f32", "ms": ms, "GB/s": B * T * 6 / ms / 1e6}))
    x = dio.pcm16_to_float(pcm)
    ph, taps = C.c_int(), C.c_int()
    _lib.check(_lib.lib().dfx_resampler_kernel(sr, new, 16, 0.99, 0, 0.0, C.byref(ph), C.byref(taps), None, None, 0))   # sinc_fast
    n, ntaps = ph.value, taps.value
    y = dio.resample(x, sr, new)
    ms = timed(lambda: dio.resample(x, sr, new))
    flops = 2.0 * y.numel() * ntaps
    print(json.dumps({"step": "resample 44100->48000 sinc_fast", "ms": ms, "taps": ntaps, "phases": n,
                      "TFLOP/s_fp32_valu": flops / ms / 1e9, "GB/s_algorithmic": (x.numel() + y.numel()) * 4 / ms / 1e6,
                      "audio_seconds_per_second": B * 10 / (ms / 1e3)}))
    ms = timed(lambda: dio.float_to_pcm16(y))
    print(json.dumps({"step": "f32_to_pcm16", "ms": ms, "GB/s": y.numel() * 6 / ms / 1e6}))


def flac(copies=512):
    import ctypes as C

    from deepfilternet_amd import _lib
    from deepfilternet_amd import io as dio
    from deepfilternet_amd.config import ModelParams
    from deepfilternet_amd.enhance import enhance, init_df

    with open(os.path.join(REPO, "tests", "golden", "flac_noise_mono.flac"), "rb") as f:
        one = f.read()
    dev = _lib.device()
    info = dio.flac_probe(one)
    n, T = copies, int(info.total_samples)
    stride = (len(one) + 15) // 16 * 16
    host = torch.zeros(n * stride, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for i in range(n):
        hv[i * stride: i * stride + len(one)] = np.frombuffer(one, np.uint8)
    blob = host.to(dev)
    Tp = (T + 7) // 8 * 8                                  # every stream's block at a multiple of 16 bytes
    buf = torch.empty((n, Tp), dtype=torch.int16, device=dev)
    out = buf[:, :T]
    status = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    i64 = C.c_int64 * n
    offs, lens, oo = i64(*[i * stride for i in range(n)]), i64(*[len(one)] * n), i64(*[i * Tp * 2 for i in range(n)])
    infos = (_lib.FlacInfo * n)(*[info] * n)
    need = C.c_int64()
    L = _lib.lib()
    _lib.check(L.dfx_flac_workspace_bytes(n, lens, C.cast(infos, C.c_void_p), C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def decode():
        _lib.check(L.dfx_flac_decode(_lib.ptr(blob), blob.numel(), n, offs, lens, C.cast(infos, C.c_void_p), oo, _lib.ptr(buf), buf.numel() * 2,
                                     _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream()))

    ms = timed(decode, iters=10)
    st = status.cpu().numpy()
    assert (st[:, 0] == 58).all() and (st[:, 1] == 0).all() and (st[:, 2] == T).all(), st[:2]
    (ref,) = dio.decode_flac([one], pcm16=True)
    assert torch.equal(out[0:1], ref) and torch.equal(out[-1:], ref)
    secs = n * T / info.sample_rate
    print(json.dumps({"step": "flac decode (resident bytes)", "streams": n, "frames": int(st[:, 0].sum()), "audio_s": secs, "ms": ms,
                      "x_realtime": secs / (ms / 1e3), "compressed_MB": n * len(one) / 1e6, "pcm16_MB": n * T * 2 / 1e6}))
    ms_c = timed(lambda: blob.copy_(host, non_blocking=True), iters=10)
    pcm_host = torch.empty((n, T), dtype=torch.int16, pin_memory=True)
    pcm_host.copy_(out)
    pcm = torch.empty((n, T), dtype=torch.int16, device=dev)
    ms_p = timed(lambda: pcm.copy_(pcm_host, non_blocking=True), iters=10)
    print(json.dumps({"step": "upload, page-locked", "compressed_ms": ms_c, "pcm16_ms": ms_p, "compressed_GB/s": host.numel() / ms_c / 1e6,
                      "pcm16_GB/s": n * T * 2 / ms_p / 1e6}))
    model, df_state, _, _ = init_df(params=ModelParams(), epoch="none", seed=0)
    ms_e = timed(lambda: enhance(model, df_state, pcm), iters=5)
    print(json.dumps({"step": "enhance, int16 resident (dfx_enhance_pcm16)", "clips": n, "audio_s": secs, "ms": ms_e,
                      "x_realtime": secs / (ms_e / 1e3), "decode_over_enhance": ms / ms_e}))


if __name__ == "__main__":
    flac() if sys.argv[1:2] == ["flac"] else main()
