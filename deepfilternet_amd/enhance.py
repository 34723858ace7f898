"""``init_df`` / ``df_features`` / ``enhance`` with the reference's signatures (DeepFilterNet/df/enhance.py:101-250),
running entirely on the MI355X through libdfx.so.

* ``df_features`` and ``enhance`` accept the same arguments and return tensors of the same shape/dtype as the reference.
* ``enhance`` keeps everything on the device: audio -> (pad) -> STFT + ERB/complex features -> DeepFilterNet3 ->
  deep filter + ERB gains (+ post filter, + attenuation limit) -> ISTFT -> slice, one C call (``dfx_enhance``).
* The batch dimension is the channel dimension C of the ``[C, T]`` input, exactly as in the reference.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .config import ModelParams
from .libdf import DF, erb, erb_norm, unit_norm
from .model import DfNet, read_cp
from .state_dict import random_state_dict

PRETRAINED_MODELS = ("DeepFilterNet", "DeepFilterNet2", "DeepFilterNet3")
DEFAULT_MODEL = "DeepFilterNet3"


def get_device() -> torch.device:
    """utils.py:20-29 get_device(); here always the HIP device libdfx runs on."""
    return _lib.device()


def init_df(
    model_base_dir: Optional[str] = None,
    post_filter: bool = False,
    log_level: str = "INFO",
    log_file: Optional[str] = "enhance.log",
    config_allow_defaults: bool = True,
    epoch: Union[str, int, None] = "best",
    default_model: str = DEFAULT_MODEL,
    mask_only: bool = False,
    *,
    params: Optional[ModelParams] = None,
    state_dict: Optional[Dict[str, "np.ndarray | torch.Tensor"]] = None,
    seed: int = 0,
) -> Tuple[DfNet, DF, str, int]:
    """enhance.py:101-187.  ``model_base_dir`` must contain ``config.ini`` and ``checkpoints/model_*.ckpt[.best]``.

    The pretrained models cannot be downloaded here (no network, enhance.py:253-273); passing one of their names raises.
    Extensions (keyword-only): ``params`` + ``state_dict`` build the model from memory; ``epoch="none"`` (or None) with no
    checkpoint initialises seeded synthetic weights (``seed``), which is what the benchmarks use.
    """
    load_cp = epoch is not None and not (isinstance(epoch, str) and epoch.lower() == "none")
    if params is None:
        if model_base_dir is None or model_base_dir in PRETRAINED_MODELS:
            raise FileNotFoundError(
                f"pretrained model '{model_base_dir or default_model}' is not available offline; pass a model directory "
                "with config.ini + checkpoints/, or params=/state_dict=")
        if os.path.isfile(model_base_dir) and model_base_dir.endswith(".tar.gz"):
            # extension: the reference's exported artefact (<model>_onnx.tar.gz, tract.rs:29-70) in place of a model directory
            from .model import read_onnx_targz

            p, state_dict = read_onnx_targz(model_base_dir)
        elif os.path.isfile(model_base_dir) and model_base_dir.endswith(".dfx"):
            # extension: a .dfx model file (export_dfx; what the C API's df_create reads)
            from .model import read_dfx

            p, state_dict = read_dfx(model_base_dir)
        elif not os.path.isdir(model_base_dir):
            raise NotADirectoryError("Base directory not found at {}".format(model_base_dir))
        else:
            p = ModelParams.from_ini(os.path.join(model_base_dir, "config.ini"), must_exist=True)
    else:
        p = params
    if post_filter:
        p.mask_pf = True  # enhance.py:152-159
    df_state = DF(sr=p.sr, fft_size=p.fft_size, hop_size=p.hop_size, nb_bands=p.nb_erb, min_nb_erb_freqs=p.min_nb_freqs)
    ep = 0
    from_checkpoint = False
    if state_dict is None and load_cp and model_base_dir is not None and os.path.isdir(model_base_dir):
        state_dict, ep = read_cp(os.path.join(model_base_dir, "checkpoints"), epoch)
        if state_dict is None:
            raise FileNotFoundError("Could not find a checkpoint")  # reference: logger.error + exit(1)
        from_checkpoint = True
    if state_dict is None:
        state_dict = random_state_dict(p, seed)
    # enhance.py:172-175: init_model(df_state, run_df=not mask_only); checkpoints load like read_cp (non-strict, size mismatches dropped)
    model = DfNet(p, state_dict, df_state, run_df=not mask_only, strict=not from_checkpoint)
    suffix = os.path.basename(os.path.abspath(model_base_dir)) if model_base_dir else p.model
    if post_filter:
        suffix += "_pf"
    return model, df_state, suffix, ep


def df_features(audio: torch.Tensor, df: DF, nb_df: int, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """enhance.py:190-203: -> spec [C,1,T',F,2], erb_feat [C,1,T',E], spec_feat [C,1,T',nb_df,2] (on the HIP device)."""
    p_alpha = _norm_alpha(df)
    x = audio.to(_lib.device(), torch.float32).contiguous()
    Cn, T = x.shape
    Tf, F, E = T // df.hop_size(), df.fft_size() // 2 + 1, df.nb_erb()
    spec = torch.empty((Cn, Tf, F, 2), dtype=torch.float32, device=x.device)
    fe = torch.empty((Cn, Tf, E), dtype=torch.float32, device=x.device)
    fs = torch.empty((Cn, Tf, nb_df, 2), dtype=torch.float32, device=x.device)
    if Cn and Tf:
        _lib.check(_lib.lib().dfx_features(df.handle, _lib.ptr(x), Cn, T, x.stride(0), int(nb_df), float(p_alpha),
                                           _lib.ptr(spec), _lib.ptr(fe), _lib.ptr(fs), _lib.stream()))
    return spec.unsqueeze(1), fe.unsqueeze(1), fs.unsqueeze(1)


def _norm_alpha(df: DF, tau: float = 1.0) -> float:
    p = ModelParams(sr=df.sr(), hop_size=df.hop_size(), norm_tau=tau)
    return p.norm_alpha()


def _workspace_cap(model: DfNet, need: int) -> Optional[int]:
    """Bytes the enhance() workspace may take: DFX_WORKSPACE_CAP_GB if set, else 90 % of what the device has free plus the workspace this
    model already holds (None when that cannot be asked, e.g. on the CPU interpreter build; ``model`` None: a buffer of its own, nothing held).  The device is only asked when the answer can
    matter: a request that fits into the workspace the model already holds needs no allocation at all."""
    env = os.environ.get("DFX_WORKSPACE_CAP_GB")
    if env:
        return int(float(env) * (1 << 30))
    if _lib.device().type != "cuda":
        return None
    # the workspace this model already holds counts as available: DfNet.workspace() releases it before it allocates a larger one
    held = model._ws.numel() if getattr(model, "_ws", None) is not None else 0
    if need <= held:
        return held
    free, _ = torch.cuda.mem_get_info(_lib.device())
    return int(0.9 * (free + held))


@torch.no_grad()
def enhance(model: DfNet, df_state: DF, audio: torch.Tensor, pad: bool = True, atten_lim_db: Optional[float] = None
            ) -> torch.Tensor:
    """enhance.py:206-250.  audio [C, T] float32 (host or device) -> enhanced audio, same shape when ``pad``.

    The result lives on the device the input came from (a CPU tensor in -> CPU tensor out, like the reference).

    Extension: an ``int16`` tensor is taken as 16-bit PCM — the sample format the reference's file loop decodes and encodes around this
    call (enhance.py:73-89 -> io.py:25-84) — and comes back as ``int16``: torchaudio's ``x / 32768`` and save_audio's
    ``(audio * (1 << 15)).to(torch.int16)`` run inside the STFT kernel's loads and the ISTFT kernel's stores (``dfx_enhance_pcm16``): the same
    samples as ``float_to_pcm16(enhance(pcm16_to_float(audio)))``, half the bytes over PCIe and no conversion passes."""
    if not isinstance(model, DfNet):
        raise TypeError("enhance() of deepfilternet_amd needs a deepfilternet_amd.DfNet (see init_df)")
    src_dev = audio.device
    pcm16 = audio.dtype == torch.int16
    # a page-locked host batch moves by DMA without the driver's staging copies (and comes back into page-locked memory): the
    # transfer is then asynchronous on the launch stream, ~55 GB/s over PCIe Gen5 instead of ~10 for pageable memory
    pinned = src_dev.type == "cpu" and audio.is_pinned() and _lib.device().type == "cuda"
    if audio.dim() != 2:
        raise ValueError("audio must have shape [C, T]")
    B, T = audio.shape
    hop = df_state.hop_size()
    n_fft = df_state.fft_size()
    out_len = T if pad else ((T // hop) * hop)
    dt = torch.int16 if pcm16 else torch.float32
    if B == 0 or out_len == 0:
        return torch.empty((B, out_len), dtype=dt, device=_lib.device()).to(src_dev)
    nbytes = C.c_int64()
    L = _lib.lib()
    lim_db = float(atten_lim_db) if atten_lim_db is not None else 0.0

    def ws_bytes(b: int) -> int:
        _lib.check(L.dfx_enhance_workspace_bytes(model.handle, df_state.handle, b, T, int(bool(pad)), C.byref(nbytes)))
        return int(nbytes.value)

    # The engine's scratch is ~82 MB per 10 s clip: a batch whose workspace does not fit what the device has free is
    # enhanced in sub-batches of whole clips, one after the other in the same workspace (clips are independent: same samples).
    # DFX_WORKSPACE_CAP_GB bounds the workspace explicitly (tests; shared devices).
    need = ws_bytes(B)
    cap = _workspace_cap(model, need)
    sub = B
    if cap is not None and need > cap:
        lo, hi = 1, B                      # largest sub-batch whose workspace fits (the requirement grows with the batch)
        if ws_bytes(1) > cap:
            # one clip alone does not fit: its rows go through time-chunked stream passes in bounded memory (enhance_long) — decided before
            # anything of the clip is on the device: a host clip is then staged chunk by chunk and never uploaded whole
            err = MemoryError(f"enhance(): a single clip of {T} samples needs {ws_bytes(1)} bytes of workspace, {cap} available")
            if not _long_serves(model, df_state):
                raise err
            return enhance_long(model, df_state, [audio], pad=pad, atten_lim_db=atten_lim_db)[0]
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if ws_bytes(mid) <= cap:
                lo = mid
            else:
                hi = mid - 1
        sub = lo if lo < 16 else lo - lo % 16   # whole groups of 16 clips (one GRU workgroup each) when there are that many
    x = audio.to(_lib.device(), dt, non_blocking=pinned).contiguous()
    y = torch.empty((B, out_len), dtype=dt, device=x.device)
    ws = model.workspace(need if sub == B else ws_bytes(sub))
    for b0 in range(0, B, sub):
        n = min(sub, B - b0)
        _lib.check((L.dfx_enhance_pcm16 if pcm16 else L.dfx_enhance)(model.handle, df_state.handle, _lib.ptr(x[b0:b0 + n]), n, T, int(bool(pad)), lim_db,
                                                                     _lib.ptr(y[b0:b0 + n]), _lib.ptr(ws), ws.numel(), _lib.stream()))
    # No silent garbage: a kernel that found a fault (fp16-split range, flag-wait timeout) raised an error word of the model.  A host
    # result is only handed back after the device has finished, so its own pass is checked; a device result is asynchronous, and the
    # words are looked at without waiting — the C entry points do the same before they start the next pass, so a fault surfaces in the
    # next call at the latest (DFX_CHECK_EVERY_PASS=1: in dfx_enhance itself).
    if pinned:
        out = torch.empty(y.shape, dtype=y.dtype, pin_memory=True)
        out.copy_(y, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        model.poll()
        return out
    out = y.to(src_dev)
    model.poll()
    return out


# Rows (clip channels) per pass of enhance_batch: tools/bench_varlen.py's sweep of 128 / 256 / 512 on its mixed set (profiles/r07_varlen.txt).
_BATCH_ROWS = 256
# Rows enhance_files gathers before it enhances them: enough for several passes of similar lengths once the window is sorted.
_FILE_WINDOW_ROWS = 4 * _BATCH_ROWS


def _varlen_ws_bytes(model: DfNet, df_state: DF, lens, pad: bool) -> int:
    arr = (C.c_int64 * len(lens))(*lens)
    nbytes = C.c_int64()
    _lib.check(_lib.lib().dfx_enhance_varlen_workspace_bytes(model.handle, df_state.handle, len(lens), arr, int(bool(pad)), C.byref(nbytes)))
    return int(nbytes.value)


def _plan_passes(model: DfNet, df_state: DF, lens, pad: bool, long_rows: Optional[list] = None):
    """[(first row, rows, workspace bytes)] over rows sorted longest first: at most _BATCH_ROWS rows per pass, and — the rule of enhance() — a
    workspace within _workspace_cap (fewer rows, whole groups of 16, when the cap says so).  A row whose workspace does not fit the cap even
    alone is appended to ``long_rows`` — the caller takes it through enhance_long's stream passes — where that list is given and the stream
    runtime serves the model; else MemoryError."""
    passes, r = [], 0
    while r < len(lens):
        n = min(_BATCH_ROWS, len(lens) - r)
        need = _varlen_ws_bytes(model, df_state, lens[r:r + n], pad)
        cap = _workspace_cap(model, need)
        if cap is not None and need > cap:
            if _varlen_ws_bytes(model, df_state, lens[r:r + 1], pad) > cap:
                if long_rows is None or not _long_serves(model, df_state):
                    raise MemoryError(f"enhance_batch(): a clip of {lens[r]} samples needs more workspace than the {cap} bytes available")
                long_rows.append(r)
                r += 1
                continue
            lo, hi = 1, n
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if _varlen_ws_bytes(model, df_state, lens[r:r + mid], pad) <= cap:
                    lo = mid
                else:
                    hi = mid - 1
            n = lo if lo < 16 else lo - lo % 16
            need = _varlen_ws_bytes(model, df_state, lens[r:r + n], pad)
        passes.append((r, n, need))
        r += n
    return passes


def _copy_rows(dst, src) -> None:
    """dst[i].copy_(src[i]) for every i, on one device: one multi-tensor launch instead of one per row."""
    if dst:
        torch._foreach_copy_(dst, src)


@torch.no_grad()
def enhance_batch(model: DfNet, df_state: DF, clips, pad: bool = True, atten_lim_db: Optional[float] = None) -> list:
    """``enhance()`` of many clips of different lengths, batched.  ``clips``: a sequence of ``[C_i, T_i]`` (or ``[T_i]``) float32 / int16
    tensors, on the host (page-locked or not) or on the device.  Result i is what ``enhance(model, df_state, clips[i], pad, atten_lim_db)``
    returns — shape, dtype, device and samples, bit for bit — and a 1-D clip gives a 1-D result.

    The channels of every clip become consecutive rows; the rows are sorted longest first and cut into passes of at most _BATCH_ROWS rows
    (fewer under the workspace cap of enhance()), one ``dfx_enhance_varlen[_pcm16]`` call each (include/dfx.h).  Every row of a pass runs the
    frames of its longest row, so similar lengths share a pass.  16-bit and float clips go into separate passes."""
    if not isinstance(model, DfNet):
        raise TypeError("enhance_batch() of deepfilternet_amd needs a deepfilternet_amd.DfNet (see init_df)")
    clips = list(clips)
    dev = _lib.device()
    cuda = dev.type == "cuda"
    hop = df_state.hop_size()
    lim_db = float(atten_lim_db) if atten_lim_db is not None else 0.0
    L = _lib.lib()
    views, results = [], []
    for a in clips:
        if a.dim() not in (1, 2):
            raise ValueError("enhance_batch(): every clip must have shape [C, T] or [T]")
        v = a.unsqueeze(0) if a.dim() == 1 else a
        T = v.shape[1]
        dt = torch.int16 if a.dtype == torch.int16 else torch.float32
        pinned = cuda and a.device.type == "cpu" and a.is_pinned()
        views.append(v)
        results.append(torch.empty((v.shape[0], T if pad else T // hop * hop), dtype=dt, device=a.device, pin_memory=pinned))
    for pcm16 in (True, False):
        dt = torch.int16 if pcm16 else torch.float32
        order = sorted((i for i in range(len(views)) if (results[i].dtype == torch.int16) == pcm16), key=lambda i: -views[i].shape[1])
        rows = [(i, ch) for i in order for ch in range(views[i].shape[0])]
        if not rows:
            continue
        lens = [views[i].shape[1] for i, _ in rows]
        long_rows = []
        passes = _plan_passes(model, df_state, lens, pad, long_rows)
        if long_rows:
            _long_rows(model, df_state, [(views[rows[r][0]][rows[r][1]], results[rows[r][0]][rows[r][1]]) for r in long_rows], pad, atten_lim_db)
        if not passes:
            continue
        ws = model.workspace(max(p[2] for p in passes))
        pending = None
        for r0, n, _ in passes:
            prow, plen = rows[r0:r0 + n], lens[r0:r0 + n]
            outs = [t if pad else t // hop * hop for t in plen]
            x = _pack_rows(views, prow, plen, dt, dev, cuda)
            y = torch.empty((n, max(max(outs), 1)), dtype=dt, device=dev)
            arr = (C.c_int64 * n)(*plen)
            _lib.check((L.dfx_enhance_varlen_pcm16 if pcm16 else L.dfx_enhance_varlen)(
                model.handle, df_state.handle, _lib.ptr(x), n, x.shape[1], arr, int(bool(pad)), lim_db, _lib.ptr(y), y.shape[1], _lib.ptr(ws),
                ws.numel(), _lib.stream()))
            # rows of device clips are copied out on the device; rows of host clips come back in one copy, unpacked once the next pass is enqueued
            on_dev = [j for j, (i, _) in enumerate(prow) if _lib.on_device(results[i])]
            _copy_rows([results[prow[j][0]][prow[j][1]] for j in on_dev], [y[j, : outs[j]] for j in on_dev])
            if pending is not None:
                _unpack_host(*pending)
                pending = None
            if len(on_dev) < n:
                yh = torch.empty(y.shape, dtype=dt, pin_memory=cuda)
                yh.copy_(y, non_blocking=cuda)
                ev = torch.cuda.Event() if cuda else None
                if ev is not None:
                    ev.record()
                pending = (results, prow, outs, yh, ev, set(on_dev))
            model.poll()
        if pending is not None:
            _unpack_host(*pending)
    model.poll()
    return [r[0] if a.dim() == 1 else r for r, a in zip(results, clips)]


def _pack_rows(views, prow, plen, dt, dev, cuda):
    """The rows of a pass as one [rows, longest] array on the device (what lies behind a row's own samples is never read): rows of host
    clips through one page-locked buffer and one copy, rows of device clips copied on the device."""
    n, T = len(prow), max(plen[0], 1)
    on_dev = [_lib.on_device(views[i]) for i, _ in prow]
    if all(on_dev):
        x = torch.empty((n, T), dtype=dt, device=dev)
    else:
        h = torch.empty((n, T), dtype=dt, pin_memory=cuda)
        for j, (i, ch) in enumerate(prow):
            if not on_dev[j]:
                h[j, : plen[j]].copy_(views[i][ch])
        x = h.to(dev, non_blocking=cuda)
    d = [j for j in range(n) if on_dev[j]]
    _copy_rows([x[j, : plen[j]] for j in d], [views[prow[j][0]][prow[j][1]] for j in d])
    return x


def _unpack_host(results, prow, outs, yh, ev, done):
    if ev is not None:
        ev.synchronize()
    for j, (i, ch) in enumerate(prow):
        if j not in done:
            results[i][ch].copy_(yh[j, : outs[j]])


# Hops per call of enhance_long.  tools/bench_long.py's sweep over 128 / 256 / 512 / 1024 is nearly flat (9.0 to 9.5 M frames/s): 256 is the last
# step that buys more than 2 %, at 7.8 GB for 256 slots (docs/measurements.md, "Clips of any length").
_LONG_HOPS = 256
# What the last enhance_long call ran with: slots, hops_per_call, the handle's device bytes (dfx_stream_memory_bytes), stream calls made.
last_long_plan: dict = {}


def _stream_bytes(model: DfNet, df_state: DF, slots: int, hops: int) -> int:
    nbytes = C.c_int64()
    _lib.check(_lib.lib().dfx_stream_memory_bytes(model.handle, df_state.handle, int(slots), int(hops), C.byref(nbytes)))
    return int(nbytes.value)


def _long_serves(model: DfNet, df_state: DF) -> bool:
    """Does the stream runtime take this model (dfx_stream_create's refusals: include/dfx.h, "Engine configurations")?"""
    try:
        _stream_bytes(model, df_state, 1, 16)
    except RuntimeError:
        return False
    return True


def _plan_long(model: DfNet, df_state: DF, rows: int, most_hops: int, slots: Optional[int], hops_per_call: Optional[int]):
    """(slots, hops_per_call, device bytes) of enhance_long's stream handle: the defaults or the caller's values, no more hops per call than
    the longest row takes, and under the cap of enhance() (DFX_WORKSPACE_CAP_GB, else 90 % of the free device memory) — slots halve first, down
    to 16, then hops down to 16, then the last slots.  MemoryError when one slot of 16 hops does not fit."""
    if slots is None:
        slots = min(rows, _BATCH_ROWS)
        slots = slots if slots < 16 else slots - slots % 16   # whole groups of 16 rows (one GRU workgroup each) when there are that many
    s = max(1, min(int(slots), rows))
    h = max(1, min(int(hops_per_call) if hops_per_call is not None else _LONG_HOPS, most_hops))
    h_min = min(16, h)
    need = _stream_bytes(model, df_state, s, h)
    cap = _workspace_cap(None, need)
    while cap is not None and need > cap:
        if s > 16:
            s = max(16, s // 2 // 16 * 16)
        elif h > h_min:
            h = max(h_min, h // 2)
        elif s > 1:
            s //= 2
        else:
            raise MemoryError(f"enhance_long(): a stream handle of one slot and {h} hops needs {need} bytes, {cap} available")
        need = _stream_bytes(model, df_state, s, h)
    return s, h, need


@torch.no_grad()
def enhance_long(model: DfNet, df_state: DF, clips, pad: bool = True, atten_lim_db: Optional[float] = None, slots: Optional[int] = None,
                 hops_per_call: Optional[int] = None) -> list:
    """``enhance()`` of clips of any length in bounded device memory.  ``clips`` is what ``enhance_batch`` accepts — ``[C_i, T_i]`` or ``[T_i]``,
    float32 or int16, host (page-locked or not) or device — and result i has the shape, dtype and device of
    ``enhance(model, df_state, clips[i], pad, atten_lim_db)``.

    Every channel of every clip is a row; the rows run, longest first, through the ``slots`` streams of one
    ``DfStream(streams=slots, max_frames=hops_per_call)``: a call feeds every busy slot its row's next ``hops_per_call`` hops (zeros behind
    the row's own samples), a row's frame count ``(T + (n_fft if pad else 0)) // hop`` gives the call's ``valid_hops`` — behind its last frame
    the row sees the batch path's zero padding (``dfx_stream_process_ends``) — and a slot whose row has put out its last sample is reset and
    takes the next row at the following call.  The device holds the handle (``dfx_stream_memory_bytes``; ``last_long_plan`` reports it) and two
    calls' worth of samples, whatever the clips' lengths; ``slots`` and ``hops_per_call`` shrink until the handle fits the cap of ``enhance()``
    (``DFX_WORKSPACE_CAP_GB``, else 90 % of the free memory), and MemoryError is raised only when one slot of 16 hops does not fit.

    The samples are those of ``enhance()`` to rounding, not bit for bit: a stream's chunks take the windowed forward pass and, on one-hop
    passes, kernels of their own, whose sums run in another order than the whole-clip pass (include/dfx.h: "the results do not depend on the
    cut beyond rounding") — about 1e-6 RMS at a signal of 0.1 RMS, and 16-bit results may differ by one LSB where that rounding crosses a
    truncation boundary.  ``atten_lim_db`` follows ``enhance()``'s rule for every value (``dfx_stream_set_atten_lim_enhance``).  A model with
    ``mask_pf`` is served by the stream runtime's post filter, libDF's, which leaves the last ``(ch * F) % 4`` bins of a frame alone where
    ``enhance()`` filters every bin: there the results agree to 1e-4.

    ``enhance()``, ``enhance_batch()`` and ``enhance_files()`` come here by themselves with the rows of a clip whose workspace does not fit the
    cap alone — where they used to raise MemoryError — and with nothing else."""
    if not isinstance(model, DfNet):
        raise TypeError("enhance_long() of deepfilternet_amd needs a deepfilternet_amd.DfNet (see init_df)")
    clips = list(clips)
    cuda = _lib.device().type == "cuda"
    hop = df_state.hop_size()
    results, pairs = [], []
    for a in clips:
        if a.dim() not in (1, 2):
            raise ValueError("enhance_long(): every clip must have shape [C, T] or [T]")
        v = a.unsqueeze(0) if a.dim() == 1 else a
        T = v.shape[1]
        dt = torch.int16 if a.dtype == torch.int16 else torch.float32
        pinned = cuda and a.device.type == "cpu" and a.is_pinned()
        r = torch.empty((v.shape[0], T if pad else T // hop * hop), dtype=dt, device=a.device, pin_memory=pinned)
        results.append(r)
        pairs += [(v[ch] if v.dtype == dt else v[ch].to(dt), r[ch]) for ch in range(v.shape[0])]
    _long_rows(model, df_state, pairs, pad, atten_lim_db, slots, hops_per_call)
    return [r[0] if a.dim() == 1 else r for r, a in zip(results, clips)]


def _long_rows(model: DfNet, df_state: DF, pairs, pad: bool, atten_lim_db: Optional[float], slots: Optional[int] = None,
               hops_per_call: Optional[int] = None) -> None:
    """enhance_long over rows: ``pairs`` = (samples [T], result [out_len]) of every row, 1-D tensors of one dtype per pair."""
    from .streaming import DfStream

    pairs = [(s, d) for s, d in pairs if d.numel() > 0]   # (a row without output — shorter than a hop without pad, or empty — is done)
    if not pairs:
        return
    hop, n_fft = df_state.hop_size(), df_state.fft_size()
    look = int(model.p.df_lookahead)
    o0 = look * hop + (n_fft - hop if pad else 0)         # a row's output starts at this stream sample (enhance.py:248-249 behind the lookahead)
    most = max(-(-(o0 + d.shape[0]) // hop) for _, d in pairs)
    slots, hops, nbytes = _plan_long(model, df_state, len(pairs), most, slots, hops_per_call)
    rt = DfStream(model, df_state, streams=slots, max_frames=hops)
    rt.set_atten_lim_enhance(atten_lim_db)
    assert rt.delay_frames == look
    calls = 0
    for dt in (torch.int16, torch.float32):   # the sample format belongs to the call: 16-bit rows first, then float rows, on the same handle
        group = sorted((p for p in pairs if p[1].dtype == dt), key=lambda p: -p[0].shape[0])
        if group:
            rt.reset()   # (every slot free and none behind an end)
            calls += _long_group(rt, group, dt, hop, (n_fft if pad else 0), o0)
    model.poll()
    last_long_plan.clear()
    last_long_plan.update(slots=slots, hops_per_call=hops, bytes=nbytes, calls=calls)


class _Slot:
    __slots__ = ("src", "dst", "T", "frames", "fed", "need")

    def __init__(self, src, dst, hop, pad_n, o0):
        self.src, self.dst, self.T = src, dst, int(src.shape[0])
        self.frames = (self.T + pad_n) // hop          # enhance.py:230-235
        self.fed = 0                                   # hops fed so far
        self.need = -(-(o0 + dst.shape[0]) // hop)     # hops until the row's last output sample is out (<= frames + lookahead)


def _long_group(rt, group, dt, hop: int, pad_n: int, o0: int) -> int:
    """The rows of one sample format through the handle's slots; returns the number of stream calls."""
    dev = _lib.device()
    cuda = dev.type == "cuda"
    S, nmax = rt.streams, rt.max_frames
    queue = list(reversed(group))                # (pop() takes the longest row left)
    slot = [None] * S
    stale = [False] * S                          # the slot's row is finished and no new one has taken it: behind its end until the next reset
    stage_in, stage_out, ev_in = [None, None], [None, None], [None, None]
    pending, calls = None, 0
    while queue or any(s is not None for s in slot):
        new = []
        for j in range(S):
            if slot[j] is None and queue:
                slot[j] = _Slot(*queue.pop(), hop, pad_n, o0)
                new.append(j)
        if new:   # a new row takes a slot at a call boundary: the slot starts over
            rt.reset(new)
            for j in new:
                stale[j] = False
        busy = [j for j in range(S) if slot[j] is not None]
        n = min(nmax, max(slot[j].need - slot[j].fed for j in busy))
        W = n * hop
        b = calls & 1
        # ---- this call's samples [S, n * hop]: host rows through a page-locked staging buffer (two of them, in turn) and one asynchronous copy,
        # device rows with the multi-tensor copy; zeros behind a row's own samples and in the slots without a row
        host = [j for j in busy if not _lib.on_device(slot[j].src)]
        took = {j: max(0, min(slot[j].T, slot[j].fed * hop + W) - slot[j].fed * hop) for j in busy}
        if host:
            if ev_in[b] is not None:
                ev_in[b].synchronize()   # (the copy that last read this buffer)
            if stage_in[b] is None:
                stage_in[b] = torch.empty((S * nmax * hop,), dtype=dt, pin_memory=cuda)
            h = stage_in[b][: S * W].view(S, W)
            for j in host:
                a, m = slot[j].fed * hop, took[j]
                h[j, :m].copy_(slot[j].src[a:a + m])
                if m < W:
                    h[j, m:].zero_()
            x = h.to(dev, non_blocking=cuda)
            if cuda:
                ev_in[b] = torch.cuda.Event()
                ev_in[b].record()
            elif x.data_ptr() == h.data_ptr():
                x = x.clone()
        else:
            x = torch.empty((S, W), dtype=dt, device=dev)
        on_dev = [j for j in busy if j not in set(host)]
        _copy_rows([x[j, : took[j]] for j in on_dev if took[j]], [slot[j].src[slot[j].fed * hop: slot[j].fed * hop + took[j]] for j in on_dev if took[j]])
        for j in range(S):
            if slot[j] is None:
                x[j].zero_()
            elif j in on_dev and took[j] < W:
                x[j, took[j]:].zero_()
        # ---- the hops of this call inside every row's clip; a slot without a row: all of them before its first row, none behind a finished one
        valid = [min(n, max(0, slot[j].frames - slot[j].fed)) if slot[j] is not None else (0 if stale[j] else n) for j in range(S)]
        y = rt.process(x, valid_hops=None if all(v == n for v in valid) else valid)   # (polls the model's error words)
        calls += 1
        # ---- the part of every row's output window that came out in this call
        d_dst, d_src, h_items = [], [], []
        for j in busy:
            s = slot[j]
            a = s.fed * hop
            lo, hi = max(a, o0), min(a + W, o0 + s.dst.shape[0])
            if hi > lo:
                if _lib.on_device(s.dst):
                    d_dst.append(s.dst[lo - o0: hi - o0])
                    d_src.append(y[j, lo - a: hi - a])
                else:
                    h_items.append((s.dst[lo - o0: hi - o0], j, lo - a, hi - a))
            s.fed += n
            if s.fed >= s.need:
                slot[j], stale[j] = None, True
        _copy_rows(d_dst, d_src)
        if pending is not None:   # the previous call's host rows are unpacked while this call runs
            _unpack_long(*pending)
            pending = None
        if h_items:
            if stage_out[b] is None:
                stage_out[b] = torch.empty((S * nmax * hop,), dtype=dt, pin_memory=cuda)
            yh = stage_out[b][: S * W].view(S, W)
            yh.copy_(y, non_blocking=cuda)
            ev = torch.cuda.Event() if cuda else None
            if ev is not None:
                ev.record()
            pending = (yh, ev, h_items)
    if pending is not None:
        _unpack_long(*pending)
    return calls


def _unpack_long(yh, ev, items) -> None:
    if ev is not None:
        ev.synchronize()
    for dst, j, lo, hi in items:
        dst.copy_(yh[j, lo:hi])


# FLAC files decoded per io.decode_flac call (and bytes: their compressed size), consecutive FLAC inputs only
_FLAC_GROUP_FILES = 512
_FLAC_GROUP_BYTES = 1 << 30


def _load_inputs(files, sr: int, method: str):
    """(file, audio, meta) of every input in order, loaded as enhance_files wants them (int16 when no resampling is needed); consecutive FLAC
    files are decoded together."""
    from .io import is_flac, load_audio, load_flac_files

    i = 0
    while i < len(files):
        if not is_flac(files[i]):
            audio, meta = load_audio(files[i], sr=sr, verbose=False, method=method, pcm16=True)
            yield files[i], audio, meta
            i += 1
            continue
        group, size = [], 0
        while i < len(files) and len(group) < _FLAC_GROUP_FILES and is_flac(files[i]):
            size += os.path.getsize(files[i])
            if group and size > _FLAC_GROUP_BYTES:
                break
            group.append(files[i])
            i += 1
        for file, (audio, meta) in zip(group, load_flac_files(group, sr=sr, verbose=False, method=method, pcm16=True)):
            yield file, audio, meta


def enhance_files(model: DfNet, df_state: DF, input_files, output_dir: Optional[str] = None, suffix: Optional[str] = None,
                  compensate_delay: bool = True, atten_lim_db: Optional[float] = None, method: str = "sinc_fast"):
    """The body of the reference's file loop, ``df.enhance.main`` (enhance.py:73-89), without its argument parser: every file is
    decoded, brought to the model's sampling rate, enhanced, brought back to its own rate and written next to the input (or into
    ``output_dir``) as ``<name>_<suffix>.wav``.  A file that already has the model's rate moves as 16-bit PCM all the way (the two
    conversions of df/io.py run inside the STFT / ISTFT kernels: ``enhance()`` on an int16 tensor); one that has to be resampled takes the
    float path (int16 -> float, resample, enhance, resample, float -> int16, all on the device).  Returns the written paths, in input order.

    The files are read in order and gathered into windows of at most _FILE_WINDOW_ROWS channels whose workspace, as one pass, fits the cap of
    ``enhance()``; a window is enhanced with ``enhance_batch`` — every file gets the samples ``enhance()`` gives it alone, so the files written
    are byte for byte those of one ``enhance()`` per file — and written before the next window is read."""
    from .io import resample, save_audio

    sr = df_state.sr()
    out, win, lens = [], [], []

    def flush():
        enhanced = enhance_batch(model, df_state, [a for _, a, _ in win], pad=compensate_delay, atten_lim_db=atten_lim_db)
        for (file, _, meta), e in zip(win, enhanced):
            if e.dtype != torch.int16:
                e = resample(e, sr, meta.sample_rate, method=method)
            if meta.encoding == "FLAC":   # the outputs are WAVE files, as in the reference: a FLAC input's name gets the extension of what is written
                file = os.path.splitext(file)[0] + ".wav"
            out.append(save_audio(file, e, sr=meta.sample_rate, output_dir=output_dir, suffix=suffix))
        win.clear()
        lens.clear()

    for file, audio, meta in _load_inputs(list(input_files), sr, method):
        more = lens + [audio.shape[-1]] * audio.shape[0]
        if win and len(more) > _FILE_WINDOW_ROWS:
            flush()
        elif win:
            need = _varlen_ws_bytes(model, df_state, more, compensate_delay)
            cap = _workspace_cap(model, need)
            if cap is not None and need > cap:
                flush()
        win.append((file, audio, meta))
        lens.extend([audio.shape[-1]] * audio.shape[0])
    if win:
        flush()
    return out


def _parse_epoch(value: str):
    """df/enhance.py parse_epoch_type: 'best', 'latest' or an epoch number."""
    try:
        return int(value)
    except ValueError:
        if value not in ("best", "latest"):
            raise ValueError(f"epoch must be 'best', 'latest' or a number, not {value!r}") from None
        return value


def main(argv=None):
    """``python -m deepfilternet_amd.enhance``: the reference's ``deepFilter`` command (df/enhance.py:299-379) — arguments, then ``init_df``
    and ``enhance_files``.  Returns the written paths."""
    import argparse
    import glob

    ap = argparse.ArgumentParser(prog="python -m deepfilternet_amd.enhance", description="Enhance noisy audio files with DeepFilterNet on the GPU.")
    ap.add_argument("--model-base-dir", "-m", type=str, default=None,
                    help="model directory (config.ini + checkpoints/), a .dfx model file or the reference's <model>_onnx.tar.gz")
    ap.add_argument("--pf", action="store_true", help="post-filter that slightly over-attenuates very noisy sections")
    ap.add_argument("--output-dir", "-o", type=str, default=None, help="directory for the enhanced files (default: the current one)")
    ap.add_argument("--epoch", "-e", default="best", type=_parse_epoch, help="checkpoint to load: 'best', 'latest' or an epoch number")
    ap.add_argument("--no-delay-compensation", dest="compensate_delay", action="store_false",
                    help="do not pad to compensate the delay of the real-time STFT / ISTFT")
    ap.add_argument("--atten-lim", "-a", type=int, default=None, help="attenuation limit in dB (mixes the noisy signal back in)")
    ap.add_argument("noisy_audio_files", type=str, nargs="*", help="noisy audio files")
    ap.add_argument("--noisy-dir", "-i", type=str, default=None, help="directory of noisy audio files, instead of noisy_audio_files")
    ap.add_argument("--no-suffix", action="store_false", dest="suffix", help="do not add the model suffix to the enhanced files")
    ap.add_argument("--no-df-stage", action="store_true", help="mask only: no deep-filter stage")
    args = ap.parse_args(argv)
    if args.noisy_dir is not None:
        if args.noisy_audio_files:
            ap.error("only one of noisy_audio_files or --noisy-dir can be given")
        files = sorted(glob.glob(os.path.join(args.noisy_dir, "*")))
    elif not args.noisy_audio_files:
        ap.error("no audio files given")
    else:
        files = args.noisy_audio_files
    model, df_state, suffix, _ = init_df(args.model_base_dir, post_filter=args.pf, epoch=args.epoch, mask_only=args.no_df_stage)
    out_dir = args.output_dir or "."
    os.makedirs(out_dir, exist_ok=True)
    return enhance_files(model, df_state, files, output_dir=out_dir, suffix=suffix if args.suffix else None,
                         compensate_delay=args.compensate_delay, atten_lim_db=args.atten_lim)


if __name__ == "__main__":
    main()
