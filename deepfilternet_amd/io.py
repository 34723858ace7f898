"""Host-side mirror of ``df/io.py`` (load_audio :25-57, save_audio :60-84, get_resample_params :92-111, resample :114-116) with
the sample work on the MI355X: the file is parsed on the host (a RIFF/WAVE reader / writer of its own, below — the reference goes
through torchaudio, which is not a dependency here; 8 / 16 / 24 / 32-bit integer PCM, 32 / 64-bit IEEE float and 8-bit G.711 A-law /
mu-law, plain or WAVE_FORMAT_EXTENSIBLE; FLAC files are not parsed on the host at all: their bytes go up as they are and ``decode_flac`` decodes them on
the device, csrc/dfx_flac.h), the int16 -> float scaling, the G.711 codec, the sample-rate conversion and the float -> int16 encoding run as HIP kernels
(csrc/dfx_io.hip), so a file -> file loop like ``enhance.main`` (enhance.py:73-89) keeps its audio on the device between decode and
encode (the rarer sample formats are scaled with torch ops on the device):

    audio, meta = load_audio("noisy.wav", sr=48000)          # [C, T] float32 on the GPU, resampled if the file is not 48 kHz
    enhanced = enhance(model, df_state, audio)
    save_audio("noisy.wav", resample(enhanced, 48000, meta.sample_rate), meta.sample_rate, suffix="DeepFilterNet3")
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from dataclasses import dataclass
from functools import lru_cache
from typing import Any, Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib

TA_RESAMPLE_SINC = "sinc_interp_hann"      # io.py:13-14
TA_RESAMPLE_KAISER = "sinc_interp_kaiser"


@dataclass
class AudioMetaData:
    """The fields of torchaudio's AudioMetaData that the reference reads (enhance.py:80-88)."""
    sample_rate: int
    num_frames: int
    num_channels: int
    bits_per_sample: int = 16
    encoding: str = "PCM_S"


def get_resample_params(method: str) -> Dict[str, Any]:
    """io.py:92-111, verbatim parameter sets."""
    params = {
        "sinc_fast": {"resampling_method": TA_RESAMPLE_SINC, "lowpass_filter_width": 16},
        "sinc_best": {"resampling_method": TA_RESAMPLE_SINC, "lowpass_filter_width": 64},
        "kaiser_fast": {"resampling_method": TA_RESAMPLE_KAISER, "lowpass_filter_width": 16, "rolloff": 0.85,
                        "beta": 8.555504641634386},
        "kaiser_best": {"resampling_method": TA_RESAMPLE_KAISER, "lowpass_filter_width": 16, "rolloff": 0.9475937167399596,
                        "beta": 14.769656459379492},
    }
    assert method in params.keys(), f"method must be one of {list(params.keys())}"
    return params[method]


class _Resampler:
    def __init__(self, orig_sr: int, new_sr: int, method: str):
        p = get_resample_params(method)
        h = C.c_void_p()
        kaiser = p["resampling_method"] == TA_RESAMPLE_KAISER
        _lib.check(_lib.lib().dfx_resampler_create(int(orig_sr), int(new_sr), int(p["lowpass_filter_width"]), float(p.get("rolloff", 0.99)),
                                                   int(kaiser), float(p.get("beta", 14.769656459379492)), C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                _lib.lib().dfx_resampler_free(h)
            except Exception:  # noqa: BLE001
                pass


@lru_cache(maxsize=16)
def _resampler(orig_sr: int, new_sr: int, method: str, lib_path: str) -> _Resampler:
    return _Resampler(orig_sr, new_sr, method)


def resample(audio: torch.Tensor, orig_sr: int, new_sr: int, method: str = "sinc_fast") -> torch.Tensor:
    """io.py:114-116.  audio [..., T] float32 -> [..., ceil(new_sr * T / orig_sr)] on the device."""
    if int(orig_sr) == int(new_sr):
        return audio                                      # torchaudio.functional.resample returns its input here
    r = _resampler(int(orig_sr), int(new_sr), method, _lib.library_path())
    x = audio.to(_lib.device(), torch.float32)
    shape = x.shape
    x = x.reshape(-1, shape[-1]).contiguous()
    B, T = x.shape
    out_len = int(_lib.lib().dfx_resampler_out_len(r.h, T))
    y = torch.empty((B, out_len), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dfx_resample(r.h, _lib.ptr(x), B, T, T, _lib.ptr(y), out_len, _lib.stream()))
    return y.reshape(*shape[:-1], out_len)


class StreamResampler:
    """``resample`` call by call: ``rows`` independent signals, each call a piece ``[rows, m * block]`` (float32, or int16 PCM) ->
    ``[rows, m * block * new_sr / orig_sr]`` in the input's dtype, with the filter's memory carried on the device.  Whatever the cut, a row's
    concatenated output is ``resample(cat(zeros(P), x), orig_sr, new_sr, method)`` cut to whole frames: the output lags by ``delay``
    samples (``P = ceil(width / block) * block`` input samples — whole frames, so that the samples land on the offline grid), and is
    bit-identical between cuts.  ``process(x, active=mask)``: rows whose entry is false sit the call out (zeros, no state moves);
    ``reset(rows)`` makes rows start over.  Parameter sets as in ``resample`` (``get_resample_params``)."""

    def __init__(self, orig_sr: int, new_sr: int, rows: int, method: str = "sinc_fast", max_samples: Optional[int] = None):
        if int(orig_sr) == int(new_sr):
            raise ValueError("StreamResampler: the two rates are equal")
        self._r = _resampler(int(orig_sr), int(new_sr), method, _lib.library_path())   # (kept alive: the handle points into it)
        self.orig_sr, self.new_sr, self.rows = int(orig_sr), int(new_sr), int(rows)
        g = int(np.gcd(self.orig_sr, self.new_sr))
        self.block, self._nw = self.orig_sr // g, self.new_sr // g
        if max_samples is None:
            max_samples = -(-self.orig_sr // self.block) * self.block      # one second
        self.max_samples = int(max_samples)
        h = C.c_void_p()
        _lib.check(_lib.lib().dfx_stream_resampler_create(self._r.h, self.rows, self.max_samples, C.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().dfx_stream_resampler_free(h)
            except Exception:  # noqa: BLE001
                pass

    def _delays(self) -> Tuple[int, int]:
        a, b = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().dfx_stream_resampler_delay(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def delay(self) -> int:
        """Output samples by which the output lags the input."""
        return self._delays()[1]

    @property
    def delay_in(self) -> int:
        """The same delay in input samples (``P``)."""
        return self._delays()[0]

    def reset(self, rows=None) -> None:
        if rows is None:
            _lib.check(_lib.lib().dfx_stream_resampler_reset(self._h, None, 0, _lib.stream()))
            return
        ids = torch.as_tensor(rows).reshape(-1)
        if ids.numel() and (ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool):
            raise TypeError("row indices must be integers")
        ids = ids.to("cpu", torch.int64).contiguous()
        _lib.check(_lib.lib().dfx_stream_resampler_reset(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int64)), int(ids.numel()), _lib.stream()))

    def process(self, x: torch.Tensor, active=None, law: Optional[str] = None) -> torch.Tensor:
        """``x`` float32, int16 PCM, or uint8 G.711 codes of ``law`` ("ulaw" / "alaw": decoded in the kernel's loads, the output encoded
        in its stores with ``float_to_g711``'s saturating rule; an inactive row comes back as the law's silence code)."""
        src_dev = x.device
        fmt = _sample_format(x, law, "StreamResampler.process")
        x = x.to(_lib.device(), _FMT_DTYPES[fmt]).contiguous()
        if x.dim() != 2 or x.shape[0] != self.rows:
            raise ValueError(f"x must have shape [{self.rows}, m*{self.block}]")
        mask = None
        if active is not None:
            mask = torch.as_tensor(active).reshape(-1)
            if mask.is_floating_point() or mask.is_complex():
                raise TypeError("active must hold bools or integers")
            if mask.numel() != self.rows:
                raise ValueError(f"active must have one entry per row ({self.rows})")
            mask = (mask.to("cpu") != 0).to(torch.uint8).contiguous()
        T = x.shape[1]
        out_len = T // self.block * self._nw
        y = torch.empty((self.rows, out_len), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().dfx_stream_resampler_process(self._h, _lib.ptr(x), fmt, T, T, _lib.ptr(y), fmt, out_len,
                                                           C.c_void_p(mask.data_ptr()) if mask is not None else None, _lib.stream()))
        return y.to(src_dev)


def pcm16_to_float(pcm: torch.Tensor) -> torch.Tensor:
    """int16 samples -> float32 in [-1, 1) (what torchaudio.load(normalize=True) returns)."""
    x = pcm.to(_lib.device()).contiguous()
    assert x.dtype == torch.int16
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dfx_pcm16_to_f32(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.stream()))
    return out


def float_to_pcm16(audio: torch.Tensor) -> torch.Tensor:
    """save_audio's ``(audio * (1 << 15)).to(torch.int16)`` (io.py:79-80)."""
    x = audio.to(_lib.device(), torch.float32).contiguous()
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    _lib.check(_lib.lib().dfx_f32_to_pcm16(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.stream()))
    return out


G711_LAWS = {"ulaw": 1, "alaw": 2}                # DFX_G711_ULAW, DFX_G711_ALAW (include/dfx.h)
G711_SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}
_FMT_DTYPES = {0: torch.float32, 1: torch.int16, 2: torch.uint8, 3: torch.uint8}   # DFX_FMT_*


def _law(law) -> int:
    try:
        return G711_LAWS[law]
    except (KeyError, TypeError):
        raise ValueError(f'law must be "ulaw" or "alaw", not {law!r}') from None


def _sample_format(x: torch.Tensor, law, who: str) -> int:
    """DFX_FMT_* of a tensor of samples: uint8 are G.711 codes and need a law; everything but int16 and uint8 is taken as float32."""
    if x.dtype == torch.uint8:
        if law is None:
            raise ValueError(f'{who}: uint8 samples are G.711 codes and need law="ulaw" or law="alaw"')
        return _law(law) + 1
    return 1 if x.dtype == torch.int16 else 0


def _g711_decode(codes: torch.Tensor, law: str, to_pcm16: bool) -> torch.Tensor:
    if codes.dtype != torch.uint8:
        raise TypeError("G.711 codes are uint8")
    k = _law(law)
    x = codes.to(_lib.device())
    if not x.is_contiguous():
        x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.int16 if to_pcm16 else torch.float32, device=x.device)
    _lib.check(_lib.lib().dfx_g711_decode(_lib.ptr(x), k, x.numel(), _lib.ptr(out), int(to_pcm16), _lib.stream()))
    return out


def _g711_encode(x: torch.Tensor, law: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    k = _law(law)
    pcm16 = x.dtype == torch.int16
    x = x.to(_lib.device(), torch.int16 if pcm16 else torch.float32).contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.numel() != x.numel() or not out.is_contiguous() or not _lib.on_device(out):
        raise ValueError("out must be a contiguous uint8 tensor of the input's size on the library's device")
    _lib.check(_lib.lib().dfx_g711_encode(_lib.ptr(x), int(pcm16), k, x.numel(), _lib.ptr(out), _lib.stream()))
    return out


def g711_to_float(codes: torch.Tensor, law: str) -> torch.Tensor:
    """uint8 G.711 codes (``law`` "ulaw" / "alaw") -> float32, the 16-bit linear value / 32768: what torchaudio.load(normalize=True)
    returns for a mu-law / A-law WAVE file.  A contiguous view is read where it lies, whatever its byte offset."""
    return _g711_decode(codes, law, False)


def g711_to_pcm16(codes: torch.Tensor, law: str) -> torch.Tensor:
    """uint8 G.711 codes -> their 16-bit linear values (int16)."""
    return _g711_decode(codes, law, True)


def float_to_g711(audio: torch.Tensor, law: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 -> uint8 G.711 codes: ``trunc(clamp(x * 32768, -32768, 32767))`` (NaN -> 0), then the sign-magnitude encoder.  Unlike
    ``float_to_pcm16`` this SATURATES.  ``out``: a contiguous uint8 tensor (or view, at any byte offset) to write into."""
    return _g711_encode(audio if audio.dtype != torch.int16 else audio.to(torch.float32) / 32768.0, law, out)


def pcm16_to_g711(pcm: torch.Tensor, law: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int16 -> uint8 G.711 codes."""
    if pcm.dtype != torch.int16:
        raise TypeError("pcm16_to_g711 takes int16 samples")
    return _g711_encode(pcm, law, out)


_WAVE_PCM, _WAVE_FLOAT, _WAVE_ALAW, _WAVE_ULAW, _WAVE_EXTENSIBLE = 1, 3, 6, 7, 0xFFFE
_WAVE_G711 = {_WAVE_ALAW: "alaw", _WAVE_ULAW: "ulaw"}


def _read_riff(file: str, frame_offset: int = 0, num_frames: int = -1):
    """-> (samples [T, C] numpy array in the file's own sample type (24-bit: int32, sign-extended; G.711: the uint8 codes), sample_rate,
    total frames, bits, float?, G.711 law or None).
    RIFF/WAVE with a 'fmt ' chunk of tag 1 (integer PCM), 3 (IEEE float), 6 (A-law), 7 (mu-law) or 0xFFFE (extensible: the sub-format's
    first two bytes); the two G.711 tags only in the extended chunk (18 bytes or more) the WAVE format prescribes for non-PCM data."""
    with open(file, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise RuntimeError(f"{file}: not a RIFF/WAVE file")
        fmt = None
        while True:
            ch = f.read(8)
            if len(ch) < 8:
                raise RuntimeError(f"{file}: no 'data' chunk")
            cid, size = ch[:4], struct.unpack("<I", ch[4:])[0]
            if cid == b"fmt ":
                body = f.read(size + (size & 1))
                if size < 16 or len(body) < 16:
                    raise RuntimeError(f"{file}: 'fmt ' chunk of {size} bytes (16 at least)")
                tag, nch, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == _WAVE_EXTENSIBLE and size >= 26:
                    valid = struct.unpack("<H", body[18:20])[0]   # wValidBitsPerSample: fewer than the container (24 in 32) would need their own scale
                    if valid not in (0, bits):
                        raise RuntimeError(f"{file}: extensible WAVE with {valid} valid bits in {bits}-bit containers is not decoded")
                    tag = struct.unpack("<H", body[24:26])[0]
                fmt = (tag, nch, rate, align, bits, size)
            elif cid == b"data":
                if fmt is None:
                    raise RuntimeError(f"{file}: 'data' chunk before 'fmt '")
                tag, nch, rate, align, bits, fmt_size = fmt
                if (tag not in (_WAVE_PCM, _WAVE_FLOAT, _WAVE_ALAW, _WAVE_ULAW) or (tag == _WAVE_PCM and bits not in (8, 16, 24, 32))
                        or (tag == _WAVE_FLOAT and bits not in (32, 64)) or (tag in _WAVE_G711 and bits != 8)):
                    raise RuntimeError(f"{file}: unsupported WAVE sample format (tag {tag}, {bits} bits); integer PCM 8/16/24/32, IEEE float 32/64 "
                                       "and 8-bit G.711 (A-law, mu-law) are decoded")
                if tag in _WAVE_G711 and fmt_size < 18:
                    # A non-PCM format carries the extended 'fmt ' chunk (cbSize: 18 bytes at least, which is what every writer of G.711 files
                    # emits, save_audio included); a 16-byte PCM header with a G.711 tag stays refused, as it has always been.
                    raise RuntimeError(f"{file}: unsupported WAVE sample format (tag {tag}, {bits} bits, in a 'fmt ' chunk of {fmt_size} bytes); "
                                       "G.711 is decoded from the 18-byte or extensible 'fmt ' chunk that non-PCM formats carry")
                bps = bits // 8
                if align != nch * bps or nch < 1:
                    raise RuntimeError(f"{file}: inconsistent 'fmt ' chunk (block align {align}, {nch} channels x {bps} bytes)")
                here = f.tell()
                f.seek(0, 2)
                size = min(size, f.tell() - here)      # (a streamed file may carry 0xFFFFFFFF / a stale size)
                total = size // align
                off = min(max(int(frame_offset or 0), 0), total)
                n = total - off if num_frames is None or num_frames <= 0 else min(int(num_frames), total - off)
                f.seek(here + off * align)
                raw = f.read(n * align)
                n = len(raw) // align
                raw = raw[: n * align]
                if tag == _WAVE_FLOAT:
                    x = np.frombuffer(raw, dtype="<f4" if bits == 32 else "<f8")
                elif bits == 8:
                    x = np.frombuffer(raw, dtype=np.uint8)
                elif bits == 16:
                    x = np.frombuffer(raw, dtype="<i2")
                elif bits == 32:
                    x = np.frombuffer(raw, dtype="<i4")
                else:   # 24-bit little endian -> int32 with the sign extended
                    b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
                    x = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
                    x = (x ^ 0x800000) - 0x800000
                return x.reshape(n, nch), rate, total, bits, tag == _WAVE_FLOAT, _WAVE_G711.get(tag)
            else:
                f.seek(size + (size & 1), 1)


def _write_riff(file: str, data: np.ndarray, sr: int, is_float: bool, law: Optional[str] = None) -> None:
    """data [T, C]: int16 -> 16-bit PCM (tag 1), float32 -> 32-bit IEEE float (tag 3, with the 'fact' chunk non-PCM formats carry);
    ``law``: uint8 G.711 codes -> tag 7 (mu-law) / 6 (A-law): an 18-byte 'fmt ' chunk (cbSize 0), a 'fact' chunk, one byte per sample."""
    T, nch = data.shape
    bps = 1 if law else (4 if is_float else 2)
    payload = np.ascontiguousarray(data.astype(np.uint8 if law else ("<f4" if is_float else "<i2"), copy=False)).tobytes()
    pad = b"\x00" if len(payload) & 1 else b""
    if law:
        fmt = struct.pack("<HHIIHHH", _WAVE_ULAW if law == "ulaw" else _WAVE_ALAW, nch, int(sr), int(sr) * nch, nch, 8, 0)
        extra = b"fact" + struct.pack("<II", 4, T)
    elif is_float:
        fmt = struct.pack("<HHIIHHH", _WAVE_FLOAT, nch, int(sr), int(sr) * nch * bps, nch * bps, 8 * bps, 0)
        extra = b"fact" + struct.pack("<II", 4, T)
    else:
        fmt = struct.pack("<HHIIHH", _WAVE_PCM, nch, int(sr), int(sr) * nch * bps, nch * bps, 8 * bps)
        extra = b""
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra + b"data" + struct.pack("<I", len(payload)) + payload + pad
    with open(file, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def is_flac(file: str) -> bool:
    """Does the file start with the ``fLaC`` marker, or with an ID3v2 tag (which no RIFF file starts with: what follows it is left to the probe)?"""
    with open(file, "rb") as f:
        head = f.read(4)
    return head == b"fLaC" or head[:3] == b"ID3"


def _as_bytes(blob) -> np.ndarray:
    if isinstance(blob, torch.Tensor):
        if blob.dtype != torch.uint8:
            raise TypeError("a FLAC stream is given as bytes or as a uint8 array")
        return blob.detach().cpu().contiguous().reshape(-1).numpy()
    if isinstance(blob, np.ndarray):
        if blob.dtype != np.uint8:
            raise TypeError("a FLAC stream is given as bytes or as a uint8 array")
        return np.ascontiguousarray(blob).reshape(-1)
    return np.frombuffer(blob, dtype=np.uint8)


def flac_probe(blob, name: str = "stream") -> "_lib.FlacInfo":
    """STREAMINFO of a FLAC stream (``dfx_flac_probe``: host arithmetic): sample_rate, channels, bits_per_sample, min_block, max_block,
    first_frame (byte offset), total_samples, md5.  RuntimeError for what is not decoded: Ogg-FLAC, no STREAMINFO, more than 8 channels,
    bit depths outside 8 .. 24."""
    b = _as_bytes(blob)
    info = _lib.FlacInfo()
    rc = _lib.lib().dfx_flac_probe(C.c_void_p(b.ctypes.data), int(b.size), C.byref(info))
    if rc != _lib.DFX_OK:
        raise RuntimeError(f"{name}: {_lib.lib().dfx_last_error().decode()}")
    return info


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


def decode_flac(blobs, pcm16: bool = False, names=None, infos_out: Optional[list] = None) -> list:
    """The bytes of many FLAC files through ONE ``dfx_flac_decode`` call: the compressed bytes go up as they are (one buffer, one copy), the
    decoder runs on the device, frames and channels of every stream side by side.  ``blobs``: ``bytes`` / uint8 arrays, one per stream.
    Returns one ``[C, T]`` tensor per stream, on the device: float32 = sample / 2^(bits - 1) — what ``load_audio`` returns for a WAVE file of
    the same samples —, or with ``pcm16=True`` int16 for the streams of at most 16 bits (a stream below 16 bits fills the int16 from the top).
    A stream with a frame that was lost (CRC-16, cut short, damaged header) raises RuntimeError naming it (``names``) and the count.
    ``infos_out``: a list that receives every stream's ``flac_probe`` result."""
    arrs = [_as_bytes(b) for b in blobs]
    n = len(arrs)
    names = list(names) if names is not None else [f"stream {i}" for i in range(n)]
    infos = [flac_probe(a, nm) for a, nm in zip(arrs, names)]
    if infos_out is not None:
        infos_out.extend(infos)
    if n == 0:
        return []
    for I, a, nm in zip(infos, arrs, names):
        if I.total_samples == 0 and a.size > I.first_frame:
            raise RuntimeError(f"{nm}: a FLAC stream whose STREAMINFO does not state its length (total samples 0) is not decoded")
    dev = _lib.device()
    cuda = dev.type == "cuda"
    offs, at = [], 0
    for a in arrs:
        offs.append(at)
        at = _align16(at + int(a.size))
    host = torch.zeros(max(at, 16), dtype=torch.uint8, pin_memory=cuda)
    hv = host.numpy()
    for a, o in zip(arrs, offs):
        hv[o:o + a.size] = a
    blob = host.to(dev, non_blocking=cuda)
    if blob.data_ptr() == host.data_ptr():
        blob = host
    out_offs, oat = [], 0
    for I in infos:
        out_offs.append(oat)
        oat = _align16(oat + (2 if I.bits_per_sample <= 16 else 4) * I.channels * I.total_samples)
    out = torch.empty(max(oat, 16), dtype=torch.uint8, device=dev)
    status = torch.zeros((n, 4), dtype=torch.int64, device=dev)
    i64 = C.c_int64 * n
    lens = i64(*[int(a.size) for a in arrs])
    info_arr = (_lib.FlacInfo * n)(*infos)
    need = C.c_int64()
    L = _lib.lib()
    _lib.check(L.dfx_flac_workspace_bytes(n, lens, C.cast(info_arr, C.c_void_p), C.byref(need)))
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
    _lib.check(L.dfx_flac_decode(_lib.ptr(blob), int(blob.numel()), n, i64(*offs), lens, C.cast(info_arr, C.c_void_p), i64(*out_offs), _lib.ptr(out),
                                 int(out.numel()), _lib.ptr(status), _lib.ptr(ws), int(ws.numel()), _lib.stream()))
    st = status.cpu().numpy()
    res = []
    for i, I in enumerate(infos):
        good, lost, written, flags = (int(v) for v in st[i])
        if lost or flags or written != I.total_samples:
            raise RuntimeError(f"{names[i]}: {lost} FLAC frame(s) lost (CRC-16 failed, stream cut short or header damaged); {good} decoded, "
                               f"{written} of {I.total_samples} samples" + ("; more sync-code look-alikes than the decoder lists" if flags else ""))
        i16 = I.bits_per_sample <= 16
        nb = (2 if i16 else 4) * I.channels * I.total_samples
        x = out[out_offs[i]:out_offs[i] + nb].view(torch.int16 if i16 else torch.float32).reshape(I.channels, I.total_samples)
        res.append(x if (not i16 or pcm16) else pcm16_to_float(x))
    return res


def flac_md5(audio: torch.Tensor, bits: int) -> bytes:
    """The MD5 STREAMINFO carries: over the interleaved samples, little endian, ceil(bits / 8) bytes each.  ``audio``: what ``decode_flac``
    returned for the stream (a device -> host copy)."""
    import hashlib

    a = audio.detach().cpu()
    if a.dtype == torch.int16:
        v = a.numpy().astype(np.int64) >> max(0, 16 - bits)
    else:
        v = np.round(a.numpy().astype(np.float64) * float(1 << (bits - 1))).astype(np.int64)
    nb = (bits + 7) // 8
    raw = np.ascontiguousarray(v.T).astype("<i8").view(np.uint8).reshape(-1, 8)[:, :nb]
    return hashlib.md5(np.ascontiguousarray(raw).tobytes()).digest()


def load_flac_files(files, sr: Optional[int] = None, verbose: bool = True, method: str = "sinc_fast", pcm16: bool = False,
                    frame_offset: int = 0, num_frames: int = -1, verify_md5: bool = False) -> list:
    """``load_audio`` of several FLAC files, decoded together (one ``decode_flac`` call): [(audio, meta)] in input order."""
    blobs = []
    for f in files:
        with open(f, "rb") as fh:
            blobs.append(fh.read())
    infos: list = []
    native = decode_flac(blobs, pcm16=True, names=files, infos_out=infos)
    res = []
    for file, x, I in zip(files, native, infos):
        if verify_md5 and any(I.md5) and flac_md5(x, I.bits_per_sample) != bytes(I.md5):
            raise RuntimeError(f"{file}: the decoded samples do not have the MD5 that STREAMINFO states")
        total, rate = int(I.total_samples), int(I.sample_rate)
        frames = num_frames
        if frames is not None and frames > 0 and sr is not None:
            if rate < sr:
                raise RuntimeError(f"{file}: num_frames with a file rate ({rate}) below the requested rate ({sr}) selects no frames (df/io.py:46-47)")
            frames *= rate // sr
        off = min(max(int(frame_offset or 0), 0), total)
        n = total - off if frames is None or frames <= 0 else min(int(frames), total - off)
        x = x[:, off:off + n]
        meta = AudioMetaData(sample_rate=rate, num_frames=total, num_channels=int(I.channels), bits_per_sample=int(I.bits_per_sample),
                             encoding="FLAC")
        if x.dtype == torch.int16:
            if pcm16 and (sr is None or rate == sr):
                res.append((x.contiguous(), meta))
                continue
            x = pcm16_to_float(x)
        if sr is not None and rate != sr:
            if verbose:
                import warnings

                warnings.warn(f"Audio sampling rate does not match model sampling rate ({rate}, {sr}). Resampling...")
            x = resample(x, rate, sr, method=method)
        res.append((x.contiguous(), meta))
    return res


def load_audio(file: str, sr: Optional[int] = None, verbose: bool = True, **kwargs) -> Tuple[torch.Tensor, AudioMetaData]:
    """io.py:25-57: audio [C, T] float32 (on the device), resampled to ``sr`` when given; ``method=`` selects the resampler set.
    Sample formats as torchaudio.load(normalize=True) scales them: int16 / 32768 (a HIP kernel), 24-bit / 2^23, int32 / 2^31,
    uint8 (x - 128) / 128, float32 as stored, float64 rounded to float32.
    ``pcm16=True`` (extension): a 16-bit file that needs no resampling is handed back as its int16 samples (on the device) — ``enhance()``
    takes them as they are.
    A-law / mu-law files (``meta.encoding`` "ALAW" / "ULAW", 8 bits): the codes' 16-bit linear values / 32768 (``g711_to_float``);
    read from the extended 'fmt ' chunk (18 bytes or more, or extensible) that non-PCM formats carry — a G.711 tag in a 16-byte PCM header is
    refused as before.
    FLAC files (recognised by their ``fLaC`` marker, or an ID3v2 tag in front of it, not by their name; native FLAC of 8 to 24 bits and up to 8
    channels; ``meta.encoding`` "FLAC", ``bits_per_sample`` / ``num_frames`` / ``sample_rate`` from STREAMINFO): the file's bytes go up as they
    are and are decoded on the device (``decode_flac``); the result is that of a WAVE file of the same samples, ``pcm16=True`` hands back
    int16 for streams of at most 16 bits.  A frame that fails its CRC raises RuntimeError with the file's name and the count;
    ``verify_md5=True`` also checks a non-zero STREAMINFO MD5 (a device -> host copy).  Ogg-FLAC and 32-bit FLAC are refused; FLAC is not written.
    ``g711=True`` (extension): the call returns ``(audio, meta, law)``; a G.711 file that needs no resampling comes back as its uint8
    codes (on the device) with ``law`` "ulaw" / "alaw" — what ``DfStream.process(..., law=law)`` takes —, anything else as usual with
    ``law`` None."""
    method = kwargs.pop("method", "sinc_fast")
    want_pcm = bool(kwargs.pop("pcm16", False))
    want_g711 = bool(kwargs.pop("g711", False))
    verify_md5 = bool(kwargs.pop("verify_md5", False))
    frames = kwargs.get("num_frames", -1)
    off = kwargs.get("frame_offset", 0)
    if is_flac(file):
        ((audio, info),) = load_flac_files([file], sr=sr, verbose=verbose, method=method, pcm16=want_pcm, frame_offset=off, num_frames=frames,
                                           verify_md5=verify_md5)
        return (audio, info, None) if want_g711 else (audio, info)
    if frames is not None and frames > 0 and sr is not None:
        rate0 = _read_riff(file, 0, 1)[1]        # io.py:46-47 scales num_frames by the file's own rate: read it first
        if rate0 < sr:   # (the reference's `num_frames *= rate0 // sr` is 0 there, which torchaudio reads as "nothing": say so instead of loading the whole file)
            raise RuntimeError(f"{file}: num_frames with a file rate ({rate0}) below the requested rate ({sr}) selects no frames (df/io.py:46-47)")
        frames *= rate0 // sr
    x, orig_sr, n, bits, is_float, law = _read_riff(file, off, frames)
    ch = x.shape[1]
    info = AudioMetaData(sample_rate=orig_sr, num_frames=n, num_channels=ch, bits_per_sample=bits,
                         encoding=law.upper() if law else ("PCM_F" if is_float else ("PCM_U" if bits == 8 else "PCM_S")))
    xt = torch.from_numpy(np.array(x.T, order="C"))       # interleaved -> [C, T] (a writable copy)
    if law:                                               # the bytes go up, the decoder runs on the device
        if want_g711 and (sr is None or orig_sr == sr):
            return xt.to(_lib.device()).contiguous(), info, law
        audio = g711_to_float(xt, law)
    elif x.dtype == np.dtype("<i2"):
        if want_pcm and (sr is None or orig_sr == sr):
            return xt.to(_lib.device()).contiguous(), info
        audio = pcm16_to_float(xt)
    else:
        xd = xt.to(_lib.device())
        if is_float:
            audio = xd.to(torch.float32)
        elif bits == 8:
            audio = (xd.to(torch.float32) - 128.0) / 128.0
        else:
            audio = xd.to(torch.float32) / float(1 << (bits - 1))
    if sr is not None and orig_sr != sr:
        if verbose:
            import warnings

            warnings.warn(f"Audio sampling rate does not match model sampling rate ({orig_sr}, {sr}). Resampling...")
        audio = resample(audio, orig_sr, sr, method=method)
    return (audio.contiguous(), info, None) if want_g711 else (audio.contiguous(), info)


def save_audio(file: str, audio: Union[torch.Tensor, np.ndarray], sr: int, output_dir: Optional[str] = None,
               suffix: Optional[str] = None, log: bool = False, dtype=torch.int16, encoding: Optional[str] = None) -> str:
    """io.py:60-84: ``dtype=torch.int16`` (default) writes 16-bit PCM (float input scaled by 2^15 and truncated, io.py:79-80, on the
    device), ``dtype=torch.float32`` a 32-bit IEEE-float WAVE (int16 input divided by 2^15, io.py:81-82) — the two files torchaudio.save
    writes for an int16 / a float32 tensor.
    ``encoding="ULAW"`` / ``"ALAW"`` (extension): an 8-bit G.711 WAVE (format tag 7 / 6) instead; float or int16 input is encoded on the
    device (``float_to_g711``: saturating; ``pcm16_to_g711``), uint8 input is taken as codes of that law.  ``dtype`` is not used then."""
    outpath = file
    if suffix is not None:
        base, ext = os.path.splitext(file)
        outpath = base + f"_{suffix}" + ext
    if output_dir is not None:
        outpath = os.path.join(output_dir, os.path.basename(outpath))
    if dtype not in (torch.int16, torch.float32):
        raise ValueError(f"save_audio: dtype must be torch.int16 or torch.float32, not {dtype}")
    if encoding not in (None, "ULAW", "ALAW"):
        raise ValueError(f'save_audio: encoding must be None, "ULAW" or "ALAW", not {encoding!r}')
    audio = torch.as_tensor(audio)
    if audio.ndim == 1:
        audio = audio.unsqueeze(0)
    if encoding is not None:
        law = encoding.lower()
        if audio.dtype != torch.uint8:
            audio = pcm16_to_g711(audio, law) if audio.dtype == torch.int16 else float_to_g711(audio, law)
        _write_riff(outpath, audio.cpu().numpy().T, int(sr), False, law)
        return outpath
    if dtype == torch.int16 and audio.dtype != torch.int16:
        audio = float_to_pcm16(audio)
    if dtype == torch.float32 and audio.dtype != torch.float32:
        audio = audio.to(torch.float32) / (1 << 15)
    if audio.dtype not in (torch.int16, torch.float32):   # (torchaudio.save takes what it is given: only these two reach it from the branches above)
        audio = audio.to(torch.float32)
    _write_riff(outpath, audio.cpu().numpy().T, int(sr), audio.dtype == torch.float32)
    return outpath
