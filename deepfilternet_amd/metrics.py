"""Scores of enhanced audio, computed on the MI355X: what the reference pins its released models with (``df/scripts/test_df.py:18-21,44-78``)
and what ``df/evaluation_utils.py`` (``SiSDRMetric``, ``StoiMetric``, ``evaluation_loop_dir_only``) computes clip by clip on a CPU process pool.

    si_sdr(reference, estimate, lengths=None) -> Tensor[B]      evaluation_utils.py:599-619 (si_sdr_speechmetrics), dB
    stoi(clean, degraded, sr, lengths=None, return_info=False)  df/stoi.py:163-231
    sepm(clean, processed, sr, lengths=None)                    df/sepm.py: {"ssnr", "llr", "wss", "fwsnr"} from one pass;
    seg_snr / llr / wss / fw_seg_snr(clean, processed, sr)      one of them (SNRseg :28-51, llr :241-277, wss :299-487, fwSNRseg :54-182)
    composite(clean, processed, sr, pesq=None)                  sepm.py:490-510: {"pesq", "csig", "cbak", "covl", "ssnr", "llr", "wss"}
    score_files([(clean, enhanced), ...], sr=None)              [{"sisdr", "stoi"}] per pair of files (composite=True: + ssnr, llr, wss, fwsnr)
    python -m deepfilternet_amd.metrics CLEAN_DIR ENHANCED_DIR [--csv FILE] [--composite]

Inputs: ``[T]``, ``[B, T]`` or a list of 1-D tensors of different lengths (what ``enhance_batch`` returns), on the CPU or the device, float32 or
int16 PCM (scaled with ``pcm16_to_float``).  ``lengths`` gives each row's sample count inside a padded ``[B, T]``.  Row ``i`` of a batch is
DEFINED as the result for that clip alone, ``stoi(clean[i:i+1, :lengths[i]], ...)``: the same bits whatever the batch (the reference pads a
batch to one length, which moves its ``pad_front``; that is not copied).  Results are float32 tensors on the device; nothing is copied to the
host and nothing waits.

STOI resamples from ``sr`` to 10 kHz with the library's resampler and the reference's default parameter set (``sinc_fast``, df/io.py:114-116); any
rate the resampler takes is accepted, rates below 10 kHz included (they are up-sampled, as the reference does); ``sr == 10000`` resamples nothing.
Rows the reference skips (fewer than 512 samples left after silent-frame removal, stoi.py:195-197, where it leaves ``out[i]`` uninitialised)
are NaN.  ``return_info=True`` adds an int32 ``[B, 4]`` tensor: windows examined, windows kept, STFT frames L, segments J (L = J = 0 when skipped).

The composite measures' parts are computed at 16 kHz in float64, as ``sepm.py`` computes them; other rates are resampled first with the same
resampler (``sinc_fast``, evaluation_utils.py:32,583-584), every row with its own length.  Clips of fewer than 600 samples at 16 kHz have no
frame (the reference raises, or averages nothing): NaN.  LLR's two quadratic forms are taken in float64 from the float32-rounded LPC
coefficients and lags; the reference takes them in float32 (2e-8 .. 3e-7 apart for noise-like clips, up to 4e-3 for strongly tonal ones, where
the float32 value is the inexact one).  PESQ (ITU-T P.862) is not computed here: it is not in the reference's own code either (it calls the
third-party ``pesq`` package); ``composite`` takes the caller's values.

NOTE: test_df.py's STOI pins were produced by pystoi, not by ``df/stoi.py`` (whose docstring says "use pystoi for reporting test results");
this module implements ``df/stoi.py``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .io import _resampler, load_audio, pcm16_to_float

STOI_FS = 10_000
SEPM_FS = 16_000
Audio = Union[torch.Tensor, Sequence[torch.Tensor]]


def _rows(x: Audio, who: str) -> Tuple[torch.Tensor, Optional[List[int]]]:
    """-> (float32 [B, T] on the device, the rows' lengths when ``x`` was a list)"""
    dev = _lib.device()

    def one(t):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: audio is given as tensors, not {type(t).__name__}")
        if t.dtype == torch.int16:
            return pcm16_to_float(t)
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: samples are float32 or int16 PCM, not {t.dtype}")
        return t.to(dev)

    if isinstance(x, (list, tuple)):
        rows = [one(t) for t in x]
        if any(r.dim() != 1 for r in rows):
            raise ValueError(f"{who}: a list holds 1-D tensors")
        lens = [int(r.shape[0]) for r in rows]
        out = torch.zeros((len(rows), max(lens, default=0)), dtype=torch.float32, device=dev)
        for i, r in enumerate(rows):
            out[i, :lens[i]] = r
        return out, lens
    t = one(x)
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2:
        raise ValueError(f"{who}: audio is [T], [B, T] or a list of 1-D tensors, not {tuple(t.shape)}")
    return t.contiguous(), None


def _pair(a: Audio, b: Audio, lengths, who: str):
    x, lx = _rows(a, who)
    y, ly = _rows(b, who)
    if x.shape != y.shape or lx != ly:
        raise ValueError(f"{who}: the two signals differ in shape ({tuple(x.shape)} and {tuple(y.shape)}" + (", or in their rows' lengths)" if lx != ly else ")"))
    B, T = x.shape
    if lengths is not None:
        if lx is not None:
            raise ValueError(f"{who}: lengths goes with a padded [B, T] tensor, not with a list")
        ln = torch.as_tensor(lengths).reshape(-1)
        if ln.is_floating_point() or ln.is_complex() or ln.dtype == torch.bool:
            raise TypeError(f"{who}: lengths holds integers")
        lens = [int(v) for v in ln.cpu().tolist()]
        if len(lens) != B:
            raise ValueError(f"{who}: lengths has {len(lens)} entries for {B} rows")
        if any(v < 0 or v > T for v in lens):
            raise ValueError(f"{who}: lengths outside [0, {T}]")
    else:
        lens = lx if lx is not None else [T] * B
    return x, y, (C.c_int64 * max(B, 1))(*lens), B, T


def _workspace(nbytes: int) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=_lib.device())


def si_sdr(reference: Audio, estimate: Audio, lengths=None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Scale-invariant SDR in dB of every row (evaluation_utils.py:599-619), float32 ``[B]`` on the device.  ``workspace``: a uint8 device tensor
    to use instead of allocating one (``dfx_si_sdr_workspace_bytes``)."""
    x, y, lens, B, T = _pair(reference, estimate, lengths, "si_sdr")
    L = _lib.lib()
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    if workspace is None:
        need = C.c_int64()
        _check(L.dfx_si_sdr_workspace_bytes(B, lens, C.byref(need)))
        workspace = _workspace(need.value)
    _check(L.dfx_si_sdr(_lib.ptr(x), _lib.ptr(y), B, T, lens, _lib.ptr(out), _lib.ptr(workspace), int(workspace.numel()), _lib.stream()))
    return out


def stoi(clean: Audio, degraded: Audio, sr: int, lengths=None, return_info: bool = False, workspace: Optional[torch.Tensor] = None):
    """STOI of every row as ``df.stoi.stoi`` defines it (stoi.py:163-231), float32 ``[B]`` on the device; with ``return_info`` also int32 ``[B, 4]``."""
    sr = int(sr)
    if sr <= 0:
        raise ValueError("stoi: sr must be positive")
    x, y, lens, B, T = _pair(clean, degraded, lengths, "stoi")
    L = _lib.lib()
    r = _resampler(sr, STOI_FS, "sinc_fast", _lib.library_path()) if sr != STOI_FS else None
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    info = torch.zeros((B, 4), dtype=torch.int32, device=x.device) if return_info else None
    if workspace is None:
        need = C.c_int64()
        _check(L.dfx_stoi_workspace_bytes(sr, B, lens, C.byref(need)))
        workspace = _workspace(need.value)
    _check(L.dfx_stoi(r.h if r is not None else None, _lib.ptr(x), _lib.ptr(y), B, T, lens, _lib.ptr(out), _lib.ptr(info), _lib.ptr(workspace),
                      int(workspace.numel()), _lib.stream()))
    return (out, info) if return_info else out


def sepm(clean: Audio, processed: Audio, sr: int, lengths=None, dtype: torch.dtype = torch.float32, return_info: bool = False,
         workspace: Optional[torch.Tensor] = None):
    """Segmental SNR, LLR, WSS and frequency-weighted segmental SNR of every row as ``df/sepm.py`` defines them, from one pass:
    ``{"ssnr", "llr", "wss", "fwsnr"}``, each ``[B]`` on the device.  The values are computed in float64; ``dtype=torch.float64`` hands them out
    unrounded.  With ``return_info`` also int32 ``[B, 2]``: frames F, and the K = round(0.95 F) smallest per-frame values LLR and WSS average."""
    sr = int(sr)
    if sr <= 0:
        raise ValueError("sepm: sr must be positive")
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"sepm: results are float32 or float64, not {dtype}")
    x, y, lens, B, T = _pair(clean, processed, lengths, "sepm")
    L = _lib.lib()
    r = _resampler(sr, SEPM_FS, "sinc_fast", _lib.library_path()) if sr != SEPM_FS else None
    out = torch.empty((B, 4), dtype=torch.float64, device=x.device)
    info = torch.zeros((B, 2), dtype=torch.int32, device=x.device) if return_info else None
    if workspace is None:
        need = C.c_int64()
        _check(L.dfx_sepm_workspace_bytes(sr, B, lens, C.byref(need)))
        workspace = _workspace(need.value)
    _check(L.dfx_sepm(r.h if r is not None else None, _lib.ptr(x), _lib.ptr(y), B, T, lens, _lib.ptr(out), _lib.ptr(info), _lib.ptr(workspace),
                      int(workspace.numel()), _lib.stream()))
    res = {k: out[:, i].to(dtype) for i, k in enumerate(("ssnr", "llr", "wss", "fwsnr"))}
    return (res, info) if return_info else res


def seg_snr(clean: Audio, processed: Audio, sr: int, **kw) -> torch.Tensor:
    """Segmental SNR in dB (sepm.py:28-51) of every row; ``sepm``'s ``"ssnr"``."""
    return sepm(clean, processed, sr, **kw)["ssnr"]


def llr(clean: Audio, processed: Audio, sr: int, **kw) -> torch.Tensor:
    """Log-likelihood ratio (sepm.py:200-277) of every row; ``sepm``'s ``"llr"``."""
    return sepm(clean, processed, sr, **kw)["llr"]


def wss(clean: Audio, processed: Audio, sr: int, **kw) -> torch.Tensor:
    """Weighted spectral slope (sepm.py:280-487) of every row; ``sepm``'s ``"wss"``."""
    return sepm(clean, processed, sr, **kw)["wss"]


def fw_seg_snr(clean: Audio, processed: Audio, sr: int, **kw) -> torch.Tensor:
    """Frequency-weighted segmental SNR in dB (sepm.py:54-182) of every row; ``sepm``'s ``"fwsnr"``."""
    return sepm(clean, processed, sr, **kw)["fwsnr"]


def composite(clean: Audio, processed: Audio, sr: int, pesq=None, lengths=None, dtype: torch.dtype = torch.float32,
              workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The composite measures (sepm.py:490-510) of every row: ``{"pesq", "csig", "cbak", "covl", "ssnr", "llr", "wss"}``, each ``[B]`` on the
    device; CSIG / CBAK / COVL limited to [1, 5].  ``pesq``: a ``[B]`` tensor or sequence of wide-band PESQ MOS values computed elsewhere —
    P.862 is not in the reference's own code (it calls the third-party ``pesq`` package), so it is not computed here.  With ``pesq=None``,
    ``pesq``, ``csig``, ``cbak`` and ``covl`` are NaN and the rest is filled."""
    m = sepm(clean, processed, sr, lengths=lengths, dtype=torch.float64, workspace=workspace)
    B = int(m["ssnr"].shape[0])
    dev = m["ssnr"].device
    if pesq is None:
        p = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    else:
        p = torch.as_tensor(pesq, dtype=torch.float64).reshape(-1).to(dev)
        if int(p.shape[0]) != B:
            raise ValueError(f"composite: pesq has {int(p.shape[0])} entries for {B} rows")

    def lim(v):   # np.min((5, np.max((1, v)))): a NaN stays
        return torch.where(torch.isnan(v), v, v.clamp(1.0, 5.0))

    res = {"pesq": p,
           "csig": lim(3.093 - 1.029 * m["llr"] + 0.603 * p - 0.009 * m["wss"]),
           "cbak": lim(1.634 + 0.478 * p - 0.007 * m["wss"] + 0.063 * m["ssnr"]),
           "covl": lim(1.594 + 0.805 * p - 0.512 * m["llr"] - 0.007 * m["wss"]),
           "ssnr": m["ssnr"], "llr": m["llr"], "wss": m["wss"]}
    return {k: v.to(dtype) for k, v in res.items()}


def _check(rc: int) -> None:
    """Argument errors of the C calls are ValueErrors here; everything else stays a DfxError."""
    if rc == _lib.DFX_ERR_INVALID_ARG:
        raise ValueError(_lib.lib().dfx_last_error().decode())
    _lib.check(rc)


SEPM_KEYS = ("ssnr", "llr", "wss", "fwsnr")


def score_files(pairs: Sequence[Tuple[str, str]], sr: Optional[int] = None, batch_seconds: float = 600.0, composite: bool = False) -> List[Dict[str, float]]:
    """``[(clean file, enhanced file)]`` -> ``[{"sisdr": dB, "stoi": value}]`` in input order.  Both files of a pair are loaded with ``load_audio`` at
    ``sr`` (default: the clean file's own rate), their first channel cut to the shorter of the two; pairs of equal rate are sorted by length
    and scored in batches of at most ``batch_seconds`` of padded audio, so that clips of similar length share a pass.  ``composite=True`` adds
    ``ssnr``, ``llr``, ``wss`` and ``fwsnr`` (``sepm``; computed at 16 kHz, as ``evaluation_loop_dir_only`` does)."""
    items = []
    for i, (cf, ef) in enumerate(pairs):
        c, meta = load_audio(cf, sr, verbose=False)
        rate = int(sr) if sr is not None else int(meta.sample_rate)
        e, _ = load_audio(ef, rate, verbose=False)
        n = min(c.shape[-1], e.shape[-1])
        items.append((rate, n, i, c[0, :n], e[0, :n]))
    res: List[Optional[Dict[str, float]]] = [None] * len(items)
    items.sort(key=lambda t: (t[0], t[1]))
    at = 0
    while at < len(items):
        rate, end = items[at][0], at + 1
        while end < len(items) and items[end][0] == rate and (end + 1 - at) * items[end][1] <= batch_seconds * rate:
            end += 1
        batch = items[at:end]
        cs, es = [b[3] for b in batch], [b[4] for b in batch]
        sd, st = si_sdr(cs, es).cpu().tolist(), stoi(cs, es, rate).cpu().tolist()
        for b, u, v in zip(batch, sd, st):
            res[b[2]] = {"sisdr": float(u), "stoi": float(v)}
        if composite:
            m = {k: v.cpu().tolist() for k, v in sepm(cs, es, rate, dtype=torch.float64).items()}
            for j, b in enumerate(batch):
                res[b[2]].update({k: float(m[k][j]) for k in SEPM_KEYS})
        at = end
    return res  # type: ignore[return-value]


def pair_directories(clean_dir: str, enhanced_dir: str) -> List[Tuple[str, str]]:
    """The file pairs of two directories: a clean file goes with the enhanced file of the same name, or — as the reference's test-set layout has
    it, where ``evaluation_loop_dir_only`` walks two sorted lists — with the one whose name starts with the clean file's stem."""
    exts = (".wav", ".flac")
    clean = sorted(f for f in os.listdir(clean_dir) if f.lower().endswith(exts))
    enh = sorted(f for f in os.listdir(enhanced_dir) if f.lower().endswith(exts))
    pairs = []
    for c in clean:
        stem = os.path.splitext(c)[0]
        m = c if c in enh else next((f for f in enh if f.startswith(stem)), None)
        if m is None:
            raise FileNotFoundError(f"{enhanced_dir}: no file for {c}")
        pairs.append((os.path.join(clean_dir, c), os.path.join(enhanced_dir, m)))
    return pairs


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(prog="python -m deepfilternet_amd.metrics", description="SI-SDR and STOI (df/stoi.py) of enhanced files against clean ones, on the GPU")
    ap.add_argument("clean_dir")
    ap.add_argument("enhanced_dir")
    ap.add_argument("--sr", type=int, default=None, help="score at this rate (default: each clean file's own; evaluation_loop_dir_only uses 16000)")
    ap.add_argument("--csv", default=None, help="write one line per file here")
    ap.add_argument("--composite", action="store_true", help="add segmental SNR, LLR, WSS and frequency-weighted segmental SNR (df/sepm.py)")
    args = ap.parse_args(argv)
    pairs = pair_directories(args.clean_dir, args.enhanced_dir)
    scores = score_files(pairs, sr=args.sr, composite=args.composite)
    cols = ("sisdr", "stoi") + (SEPM_KEYS if args.composite else ())
    lines = ["file," + ",".join(cols)] + [os.path.basename(c) + "".join(f",{s[k]:.6f}" for k in cols) for (c, _), s in zip(pairs, scores)]
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines))
    good = [s for s in scores if s["stoi"] == s["stoi"]]
    if scores:
        print(f"mean over {len(scores)} files: SI-SDR {sum(s['sisdr'] for s in scores) / len(scores):.4f} dB, "
              f"STOI {sum(s['stoi'] for s in good) / max(len(good), 1):.6f} ({len(scores) - len(good)} skipped: too short after silent-frame removal)")
    return 0


if __name__ == "__main__":
    import sys

    sys.exit(main())
