"""Frame-by-frame (streaming) enhancement: the host-side mirror of the reference's real-time runtime ``DfTract``
(libDF/src/tract.rs:509-642) and its C API ``df_create / df_process_frame / df_set_atten_lim / df_set_post_filter_beta / df_free``
(libDF/src/capi.rs:83-253), for many independent mono streams advanced in lockstep on one MI355X.

    rt = DfStream(model, df_state, streams=4096)           # df_create, once
    for hop in audio.split(rt.frame_length, dim=1):        # [streams, 480] per call
        out = rt.process(hop)                              # df_process_frame: the enhanced hop of `lookahead` calls ago

``process`` also accepts several hops per call (``[streams, n * hop]``, ``n <= max_frames``); the concatenated output does not depend
on how the signal is cut.  It equals ``enhance(model, df_state, audio, pad=False)`` delayed by ``delay_frames`` hops (the first
``delay_frames`` output hops are silence, like the reference's rolling buffers).

``gating=True`` switches on the reference runtime's per-frame decisions (tract.rs:513-525,658-672), taken independently by every
stream: stages are skipped according to the local SNR (``thresholds`` = min_db, max_db_erb, max_db_df; reference defaults
-10 / 30 / 20 dB), skipped decoders keep their state, and a stream that has been silent for more than five hops is answered with
zeros without being processed.

``channels=k`` makes every k consecutive rows the channels of one stream (``RuntimeParams::n_ch``): per-channel STFT / network state,
one ERB mask per stream (``reduce_mask`` = "mean" (reference default) | "max" | "none", tract.rs:96-118,868-902), one stage decision
per stream (taken from its first channel's local SNR).

The handle takes the model's engine configuration: a model created under ``DFX_EXACT_FP32=1`` streams in exact fp32 arithmetic (equal to
its own ``enhance(pad=False)`` delayed; one launch per GRU layer on a one-hop call, like the fp16-split default), and a mask-only model
(``init_df(mask_only=True)``) streams without the DF stage: gated, it never takes stage 2, and ``process_raw`` reports gains only.

``rt.reset([3, 17])`` makes single streams start over (a new caller in a used slot) while all others run on; ``rt.frames`` are the per-stream ages in hops.

``rt.process(hops, valid_hops=[...])`` ends clips inside a call: entry ``v`` of a stream says that the call's first ``v`` hops are the last frames
of its clip; what follows (feed zeros) is the batch path's zero padding behind a clip — spectrum and normalised features — so the stream's
output is ``enhance(pad=False)`` of exactly its own frames, delayed, its last ``delay_frames`` frames included.  An ended stream takes 0 until
``reset([i])`` gives the slot to the next clip.  ``deepfilternet_amd.enhance.enhance_long`` drives a handle this way for clips of any length.

``pausable=True`` lets single streams sit calls out: ``rt.process(hop, active=mask)`` with one bool per stream.  A stream whose entry is
false is paused for that call — none of its state moves and its age stands still, its rows of the output are exact zeros and its lsnr
NaN, and its next active hop is processed as if the paused calls had not happened (every caller keeps its own clock, as with one
reference handle each).  Its input rows are still read and computed, then discarded: fill them with finite samples (zeros are fine).
A pause is not silence: on a gated handle the stream's silent-input counter neither rises nor clears.  ``reset([i])`` followed by
paused calls reserves a slot.  A paused row still costs its lane; a pausable handle runs one hop per pass in the per-stream state forms
of a gated handle, so declare it only where it is needed.

Settings per stream: in the reference the attenuation limit, the post-filter beta and the thresholds belong to one ``DfTract``, i.e. to one
caller (capi.rs:136-156, tract.rs:160-170).  ``rt.set_atten_lim(12, streams=[3])``, ``rt.set_post_filter_beta([0.02, 0.05], streams=[3, 17])``
and ``rt.set_thresholds(-10, 30, 20, streams=ids)`` set them for single streams of a running handle; ``rt.settings`` reports every stream's
values.  A setter takes effect with the next ``process`` call and does not wait for the device; resets leave settings alone (a new caller
sets its own after ``reset([i])``), and a paused stream's settings can be changed.  Without ``streams`` the setters are handle-wide, as
before: they set every stream's value and make the handle uniform in that setting again.  The undelayed pass-through (``set_atten_lim(0)``)
is a handle-wide mode; ``set_atten_lim(0, streams=[i])`` mixes with a limit just below 1 instead: stream i's noisy input comes back delayed
like every other stream's output, and its state keeps advancing.  The steady hop costs no extra launch on a handle with per-stream settings.

``sr=16000`` (8, 12, 16, 24, 32, 44.1, 88.2 or 96 kHz at a 48 kHz model) makes the handle take and return hops at the caller's own rate:
``frame_length`` is then ``hop * sr / 48000`` samples, an up-sampler in front of the pass and a down-sampler behind it (stateful forms of
``io.resample``'s filters, ``resample_method`` picks the parameter set) run on the device with the rest of the hop, and ``process`` also
takes int16 PCM and returns int16 (at any rate, 48 kHz included).  The output equals ``io.resample`` -> a 48 kHz ``DfStream`` ->
``io.resample`` with each resampler fed its whole-frame delay of zeros first; together they add ``resample_delay`` samples at the caller's
rate (34 at 16 kHz, 294 at 44.1 kHz with ``sinc_fast``) to the latency.  Rates at which the hop is no whole number of resampler frames
(22.05 kHz, 11.025 kHz) are refused.

``snap = rt.export_streams([17, 42])`` copies live streams out of a handle and ``other.import_streams([3, 4], snap)`` continues them in
another one — to drain a handle, merge two, grow one (create a bigger handle, ``big.import_streams(range(n), rt.export_streams())``, drop
the old one) or checkpoint calls.  A ``StreamSnapshot`` is two tensors: ``payload`` (uint8 ``[n, snapshot_bytes]`` on the device: every
state row of the streams in a layout that does not depend on the handle) and ``meta`` (uint8 on the host: format version, a fingerprint of
the kind of handle, the stream's age and settings); ``.cpu()`` / ``.to(device)`` move it, ``torch.save(snap.state_dict(), f)`` and
``StreamSnapshot.from_state_dict(torch.load(f))`` take it through files and pipes.  The two handles must be of the same kind (model
configuration, channels, gating, pausable, ``sr``; weights are not checked); streams, ``max_frames`` and hop count may differ.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from .libdf import DF
from .model import DfNet


class StreamSnapshot:
    """Streams taken out of a ``DfStream`` (``export_streams``): ``payload`` uint8 [n, bytes per stream] — position-independent bytes, on the
    device they were exported on until moved — and ``meta`` uint8 [n, META_BYTES] on the host (one ``dfx_stream_meta`` per stream)."""
    META_BYTES = 48

    def __init__(self, payload: torch.Tensor, meta: torch.Tensor):
        if payload.dtype != torch.uint8 or meta.dtype != torch.uint8 or payload.dim() != 2 or meta.dim() != 2:
            raise TypeError("StreamSnapshot: payload and meta are 2-d uint8 tensors")
        if meta.shape[1] != self.META_BYTES or meta.shape[0] != payload.shape[0]:
            raise ValueError(f"StreamSnapshot: meta must be [{payload.shape[0]}, {self.META_BYTES}]")
        self.payload, self.meta = payload, meta.to("cpu").contiguous()

    def __len__(self) -> int:
        return int(self.payload.shape[0])

    @property
    def ages(self) -> torch.Tensor:
        """Hops of network time every stream had consumed when it was exported: int64 [n]."""
        return self.meta[:, 16:24].contiguous().view(torch.int64).reshape(-1).clone()

    def to(self, device) -> "StreamSnapshot":
        return StreamSnapshot(self.payload.to(device), self.meta)

    def cpu(self) -> "StreamSnapshot":
        return self.to("cpu")

    def state_dict(self) -> dict:
        return {"payload": self.payload, "meta": self.meta}

    @classmethod
    def from_state_dict(cls, sd: dict) -> "StreamSnapshot":
        return cls(sd["payload"], sd["meta"])


class DfStream:
    def __init__(self, model: DfNet, df_state: DF, streams: int = 1, max_frames: int = 1, atten_lim_db: Optional[float] = None,
                 gating: bool = False, thresholds: Optional[Tuple[float, float, float]] = None, channels: int = 1,
                 reduce_mask: str = "mean", pausable: bool = False, sr: Optional[int] = None, resample_method: str = "sinc_fast",
                 law: Optional[str] = None):
        if not isinstance(model, DfNet):
            raise TypeError("DfStream needs a deepfilternet_amd.DfNet (see init_df)")
        h = C.c_void_p()
        _lib.check(_lib.lib().dfx_stream_create(model.handle, df_state.handle, int(streams), int(max_frames), C.byref(h)))
        self._h = h
        if law is not None:
            from .io import _law

            _law(law)   # ("ulaw" / "alaw": the G.711 law of uint8 frames, unless a call names its own)
        self.law = law
        self._model, self._df = model, df_state  # keep the handles the runtime points into alive
        self.streams, self.max_frames = int(streams), int(max_frames)
        if atten_lim_db is not None:
            self.set_atten_lim(atten_lim_db)
        if channels != 1:
            _lib.check(_lib.lib().dfx_stream_set_channels(self._h, int(channels), {"none": 0, "max": 1, "mean": 2}[reduce_mask]))
        self.channels = int(channels)
        if thresholds is not None:
            self.set_thresholds(*thresholds)
        if gating:
            self.set_gating(True)
        if pausable:
            _lib.check(_lib.lib().dfx_stream_set_pausable(self._h, 1))
        if sr is not None:
            from .io import TA_RESAMPLE_KAISER, get_resample_params

            rp = get_resample_params(resample_method)
            _lib.check(_lib.lib().dfx_stream_set_sample_rate(self._h, int(sr), int(rp["lowpass_filter_width"]), float(rp.get("rolloff", 0.99)),
                                                             int(rp["resampling_method"] == TA_RESAMPLE_KAISER),
                                                             float(rp.get("beta", 14.769656459379492))))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().dfx_stream_free(h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass

    @property
    def frame_length(self) -> int:
        """df_get_frame_length (capi.rs:108): samples per hop, at the caller's rate (``sr``)."""
        return int(_lib.lib().dfx_stream_frame_length(self._h))

    @property
    def sr(self) -> int:
        """The rate of the hops ``process`` takes and returns (the model's unless ``sr=`` was given)."""
        return int(_lib.lib().dfx_stream_sample_rate(self._h))

    @property
    def resample_delay(self) -> int:
        """Samples at the caller's rate by which the two sample-rate converters delay the output, on top of the STFT's and the lookahead's
        latency (0 without ``sr=``)."""
        return int(_lib.lib().dfx_stream_resample_delay(self._h))

    @property
    def delay_frames(self) -> int:
        """Hops by which the output lags the input (the model's lookahead), on top of the STFT's fft-hop samples."""
        return int(_lib.lib().dfx_stream_delay_frames(self._h))

    def _stream_ids(self, streams) -> torch.Tensor:
        ids = torch.as_tensor(streams).reshape(-1)
        if ids.numel() and (ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool):
            raise TypeError("stream indices must be integers")
        return ids.to("cpu", torch.int64).contiguous()

    def _set_streams(self, fn, streams, values, width: int) -> None:
        """One per-stream setter call: ``values`` are ``width`` scalars (broadcast over the ids) or sequences with one entry per id."""
        ids = self._stream_ids(streams)
        cols = []
        for v in values:
            v = torch.as_tensor(v, dtype=torch.float32).to("cpu")
            if v.dim() == 0:
                v = v.expand(ids.numel())
            v = v.reshape(-1)
            if v.numel() != ids.numel():
                raise ValueError(f"{ids.numel()} stream indices but {v.numel()} values")
            cols.append(v)
        vals = torch.stack(cols, 1).contiguous()   # [count, width]
        assert vals.shape == (ids.numel(), width)
        _lib.check(fn(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int64)), int(ids.numel()), C.cast(vals.data_ptr(), C.POINTER(C.c_float)),
                      _lib.stream()))

    def set_atten_lim(self, lim_db, streams=None) -> None:
        """df_set_atten_lim (capi.rs:136, tract.rs:387-398): |dB| >= 100 = no limit.  ``streams=None``: the whole handle, and |dB| < 0.01 =
        pass the input through undelayed (a handle-wide mode: the network idles).  ``streams`` = a sequence or integer tensor of stream
        indices: those streams alone, ``lim_db`` a scalar or one value per index; there |dB| < 0.01 mixes with a limit just below 1 (the
        stream's input comes back delayed like everybody's output).  Does not wait for the device."""
        if streams is None:
            _lib.check(_lib.lib().dfx_stream_set_atten_lim(self._h, float(lim_db)))
        else:
            self._set_streams(_lib.lib().dfx_stream_set_atten_lim_streams, streams, [lim_db], 1)

    def set_atten_lim_enhance(self, atten_lim_db: Optional[float]) -> None:
        """The handle-wide limit by ``enhance()``'s rule (df/enhance.py:238-240) instead of the runtime's: ``None`` or 0 = no limit, every other
        value mixes with ``10 ** (-abs(dB) / 20)`` kept below 1 — no undelayed pass-through below 0.01 dB, no "off" from 100 dB on.  For handles
        whose streams are the clips of an ``enhance()`` call (``enhance_long``).  ``settings`` then reports ``abs(dB)`` as given."""
        _lib.check(_lib.lib().dfx_stream_set_atten_lim_enhance(self._h, float(atten_lim_db) if atten_lim_db is not None else 0.0))

    def set_post_filter_beta(self, beta, streams=None) -> None:
        """df_set_post_filter_beta (capi.rs:146): 0 disables the post filter.  ``streams`` as in ``set_atten_lim``."""
        if streams is None:
            _lib.check(_lib.lib().dfx_stream_set_post_filter_beta(self._h, float(beta)))
        else:
            self._set_streams(_lib.lib().dfx_stream_set_post_filter_beta_streams, streams, [beta], 1)

    def set_gating(self, enable: bool) -> None:
        """DfTract::process's stage skipping and silent-input shortcut (tract.rs:513-525,658-672), per stream."""
        _lib.check(_lib.lib().dfx_stream_set_gating(self._h, int(bool(enable))))

    def set_thresholds(self, min_db_thresh, max_db_erb_thresh, max_db_df_thresh, streams=None) -> None:
        """RuntimeParams::with_thresholds (tract.rs:160-170).  ``streams`` as in ``set_atten_lim`` (stored on a handle without gating,
        in force once gating is on)."""
        if streams is None:
            _lib.check(_lib.lib().dfx_stream_set_thresholds(self._h, float(min_db_thresh), float(max_db_erb_thresh),
                                                            float(max_db_df_thresh)))
        else:
            self._set_streams(_lib.lib().dfx_stream_set_thresholds_streams, streams, [min_db_thresh, max_db_erb_thresh, max_db_df_thresh], 3)

    @property
    def settings(self) -> dict:
        """Every stream's settings as they were set (CPU tensors, n = streams // channels): ``atten_lim_db`` [n] (|dB|, 100 = off),
        ``post_filter_beta`` [n] (the model's value where none was set), ``thresholds`` [n, 3] (min_db, max_db_erb, max_db_df)."""
        out = torch.zeros(self.streams // self.channels, 5, dtype=torch.float32)
        _lib.check(_lib.lib().dfx_stream_get_settings(self._h, C.cast(out.data_ptr(), C.POINTER(C.c_float))))
        return {"atten_lim_db": out[:, 0].clone(), "post_filter_beta": out[:, 1].clone(), "thresholds": out[:, 2:].clone()}

    def reset(self, streams=None) -> None:
        """``None``: the whole handle goes back to the state after creation.  A sequence or integer tensor of stream indices: those
        streams start over like the streams of a fresh handle (``delay_frames`` hops of silence, then their own signal since the reset,
        enhanced and delayed), every other stream is untouched.  Settings stay, in both forms — the handle's and every stream's own
        (``set_atten_lim(..., streams=...)`` and its neighbours): a new caller sets its own after the reset.  Does not wait for the device."""
        if streams is None:
            _lib.check(_lib.lib().dfx_stream_reset(self._h, _lib.stream()))
            return
        ids = self._stream_ids(streams)
        _lib.check(_lib.lib().dfx_stream_reset_streams(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int64)), int(ids.numel()), _lib.stream()))

    @property
    def snapshot_bytes(self) -> int:
        """Bytes of one stream's record in a ``StreamSnapshot`` of this handle."""
        n = C.c_int64(0)
        _lib.check(_lib.lib().dfx_stream_snapshot_bytes(self._h, C.byref(n)))
        return int(n.value)

    def export_streams(self, streams=None) -> "StreamSnapshot":
        """A copy of the named streams' state (``None``: every stream, in order) as a ``StreamSnapshot`` on the device; the streams run on.
        Does not wait for the device."""
        ids = torch.arange(self.streams // self.channels, dtype=torch.int64) if streams is None else self._stream_ids(streams)
        n = int(ids.numel())
        payload = torch.empty((n, self.snapshot_bytes), dtype=torch.uint8, device=_lib.device())
        meta = torch.zeros((n, StreamSnapshot.META_BYTES), dtype=torch.uint8)
        _lib.check(_lib.lib().dfx_stream_export_streams(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int64)), n, _lib.ptr(payload),
                                                        C.c_void_p(meta.data_ptr()), _lib.stream()))
        return StreamSnapshot(payload, meta)

    def import_streams(self, streams, snap: "StreamSnapshot", settings: bool = True) -> None:
        """The streams of ``snap`` continue in the slots ``streams`` of this handle (one index per snapshot entry, no index twice): the
        slots are overwritten completely, every other stream is untouched, the streams keep their ages.  ``settings``: their attenuation
        limit, post-filter beta and thresholds arrive too; ``False``: the slots keep their own.  The snapshot must come from the same kind
        of handle (model configuration, channels, gating, pausable, ``sr``); the number of streams, ``max_frames`` and the hop count may
        differ.  A handle in the undelayed pass-through (``set_atten_lim(0)``) neither exports nor imports.  A snapshot on the host is
        copied to the device first; otherwise nothing waits."""
        ids = self._stream_ids(streams)
        n = int(ids.numel())
        if not isinstance(snap, StreamSnapshot):
            raise TypeError("import_streams needs a StreamSnapshot")
        if len(snap) != n:
            raise ValueError(f"{n} stream indices but {len(snap)} snapshot entries")
        if snap.payload.shape[1] != self.snapshot_bytes:
            raise ValueError(f"snapshot records have {snap.payload.shape[1]} bytes, this handle's have {self.snapshot_bytes}")
        payload = snap.payload.to(_lib.device()).contiguous()
        meta = snap.meta.to("cpu").contiguous()
        _lib.check(_lib.lib().dfx_stream_import_streams(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int64)), n, _lib.ptr(payload),
                                                        C.c_void_p(meta.data_ptr()), int(bool(settings)), _lib.stream()))

    @property
    def frames(self) -> torch.Tensor:
        """Hops of network time every stream has consumed since its own last reset (calls it sat out do not count): CPU int64 [streams / channels]."""
        out = torch.zeros(self.streams // self.channels, dtype=torch.int64)
        _lib.check(_lib.lib().dfx_stream_frames(self._h, C.cast(out.data_ptr(), C.POINTER(C.c_int64))))
        return out

    def process(self, frames: torch.Tensor, return_lsnr: bool = False, active=None, law: Optional[str] = None, valid_hops=None):
        """df_process_frame (capi.rs:161) for every stream: ``frames`` [streams, n*hop] float32 -> enhanced [streams, n*hop]
        (on the device the input came from); with ``return_lsnr`` also the local SNR estimates [streams, n] in dB.  int16 ``frames`` are
        16-bit PCM (x / 32768) and come back as int16 (``float_to_pcm16``'s encoding); ``hop`` is ``frame_length``, at the caller's rate.
        uint8 ``frames`` are G.711 codes — an RTP payload's bytes — of ``law`` ("ulaw" / "alaw"; default: the handle's ``law=``) and come
        back as codes (``io.g711_to_float`` in, ``io.float_to_g711``'s saturating rule out; a paused stream: the law's silence code; in the
        undelayed pass-through the very bytes).  The format belongs to the call: one handle takes any of them from call to call.

        ``active`` (pausable handles): a sequence or tensor of bools or integers, one per stream (``streams // channels``); a stream whose
        entry is false is paused for all hops of this call (zeros out, lsnr NaN, no state moves; its input rows must still be finite).
        ``None`` = all streams take part.  The mask is read on the host: a device tensor is copied there first, which waits for the device.

        ``valid_hops`` (``dfx_stream_process_ends``; float32 or int16 frames on a handle without gating, pausing, ``channels`` or ``sr``): a
        sequence or tensor of integers, one per stream, read on the host.  Entry ``v`` (0 <= v <= n) says that the first ``v`` hops of this
        call are the last frames of that stream's clip: what follows — feed zeros — is the batch path's zero padding behind a clip, so the
        stream's output is ``enhance(pad=False)`` of exactly its own frames, delayed, the last ``delay_frames`` frames included.  A stream
        that has ended takes 0 in every later call until ``reset([i])``.  ``None`` = no stream ends in this call."""
        ends = None
        if valid_hops is not None:
            ends = torch.as_tensor(valid_hops).reshape(-1)
            if ends.is_floating_point() or ends.is_complex() or ends.dtype == torch.bool:
                raise TypeError("valid_hops must hold integers")
            if ends.numel() != self.streams:
                raise ValueError(f"valid_hops must have one entry per stream ({self.streams})")
            if active is not None:
                raise ValueError("valid_hops and active cannot be combined (clip ends are not served on pausable handles)")
            ends = ends.to("cpu", torch.int64).contiguous()
        mask = None
        if active is not None:
            mask = torch.as_tensor(active).reshape(-1)
            if mask.is_floating_point() or mask.is_complex():
                raise TypeError("active must hold bools or integers")
            if mask.numel() != self.streams // self.channels:
                raise ValueError(f"active must have one entry per stream ({self.streams // self.channels})")
            mask = (mask.to("cpu") != 0).to(torch.uint8).contiguous()
        src_dev = frames.device
        from .io import _FMT_DTYPES, _sample_format

        fmt = _sample_format(frames, law if law is not None else self.law, "DfStream.process")
        pcm16 = fmt == 1
        x = frames.to(_lib.device(), _FMT_DTYPES[fmt]).contiguous()
        hop = self.frame_length
        if x.dim() != 2 or x.shape[0] != self.streams or x.shape[1] % hop or x.shape[1] == 0:
            raise ValueError(f"frames must have shape [{self.streams}, n*{hop}]")
        n = x.shape[1] // hop
        if n > self.max_frames:
            raise ValueError(f"at most max_frames={self.max_frames} hops per call")
        y = torch.empty_like(x)
        lsnr = torch.empty((self.streams, n), dtype=torch.float32, device=x.device) if return_lsnr else None
        if ends is not None:
            if fmt >= 2:
                raise ValueError("valid_hops: float32 or int16 frames")
            _lib.check(_lib.lib().dfx_stream_process_ends(self._h, _lib.ptr(x), fmt, n, _lib.ptr(y), _lib.ptr(lsnr),
                                                          C.cast(ends.data_ptr(), C.POINTER(C.c_int64)), _lib.stream()))
        elif fmt >= 2:
            _lib.check(_lib.lib().dfx_stream_process_g711(self._h, _lib.ptr(x), fmt - 1, n, _lib.ptr(y), _lib.ptr(lsnr),
                                                          C.c_void_p(mask.data_ptr()) if mask is not None else None, _lib.stream()))
        elif pcm16:
            _lib.check(_lib.lib().dfx_stream_process_pcm16(self._h, _lib.ptr(x), n, _lib.ptr(y), _lib.ptr(lsnr),
                                                           C.c_void_p(mask.data_ptr()) if mask is not None else None, _lib.stream()))
        elif mask is None:
            _lib.check(_lib.lib().dfx_stream_process(self._h, _lib.ptr(x), n, _lib.ptr(y), _lib.ptr(lsnr), _lib.stream()))
        else:
            _lib.check(_lib.lib().dfx_stream_process_active(self._h, _lib.ptr(x), n, _lib.ptr(y), _lib.ptr(lsnr), C.c_void_p(mask.data_ptr()),
                                                            _lib.stream()))
        y = y.to(src_dev)
        self._model.poll()   # faults raised by kernels (invalid results) are never silent: see DfNet.poll
        return (y, lsnr.to(src_dev)) if return_lsnr else y

    def process_raw(self, spec: torch.Tensor):
        """df_process_frame_raw (capi.rs:172-210 -> DfTract::process_raw, tract.rs:441-507) for every stream: one spectral frame
        ``spec`` [streams, F] complex64 (or [streams, F, 2] float32) -> (lsnr [streams], gains [streams, nb_erb], coefs
        [streams, df_order, nb_df] complex64, stages [streams] uint8: bit value 2 = gains present, 8 = coefficients present — where the
        reference hands back NULL pointers the arrays here hold placeholders).  Needs ``gating=True``."""
        src_dev = spec.device
        x = torch.view_as_real(spec) if spec.is_complex() else spec
        x = x.to(_lib.device(), torch.float32).contiguous()
        p = self._model.p
        if x.dim() != 3 or x.shape[0] != self.streams or x.shape[1] != p.freq_bins or x.shape[2] != 2:
            raise ValueError(f"spec must have shape [{self.streams}, {p.freq_bins}] complex")
        gains = torch.empty((self.streams, p.nb_erb), dtype=torch.float32, device=x.device)
        coefs = torch.empty((self.streams, p.df_order, p.nb_df, 2), dtype=torch.float32, device=x.device)
        stages = torch.empty((self.streams,), dtype=torch.uint8, device=x.device)
        lsnr = torch.empty((self.streams,), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().dfx_stream_process_raw(self._h, _lib.ptr(x), _lib.ptr(gains), _lib.ptr(coefs), _lib.ptr(stages), _lib.ptr(lsnr),
                                                     _lib.stream()))
        out = lsnr.to(src_dev), gains.to(src_dev), torch.view_as_complex(coefs).to(src_dev), stages.to(src_dev)
        self._model.poll()
        return out
