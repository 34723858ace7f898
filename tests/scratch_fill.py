"""Helpers of tests/test_scratch_contents.py: memory that a pass starts on holds a chosen byte pattern instead of zeros or the values of the
previous, identical pass.

Two sources of memory reach the engine.  The workspace of a pass is filled by the engine itself when the handle was created under
``DFX_WS_FILL=<byte>`` (a test hook): the fill runs on the pass's own stream before anything else of the pass.  Everything the
Python package allocates around a call — outputs, staging buffers — comes from ``torch.empty`` / ``torch.empty_like``: ``fresh_memory``
replaces the two for the duration of a call by versions that fill what they return.

The patterns:
  0x00  what a new device allocation usually holds: the baseline every other run has to equal.
  0xFF  NaN as float32 and as float16, -1 / all ones as an index or a length.
  0x4B  1.3323e7 as float32 (0x4B4B4B4B), 14.59 as float16: FINITE, so it survives the max / compare operations that swallow a NaN
        (fmaxf(NaN, 0) = 0), one stray element moves any output far outside every tolerance, and as an operand of an fp16-split matrix
        operation it is above the split's range (6e4) and raises the range guard."""
import contextlib
import os

import numpy as np
import torch

FILLS = (0x00, 0xFF, 0x4B)
SWITCH = "DFX_WS_FILL"


def _filled(t, byte):
    if isinstance(t, torch.Tensor) and t.numel() and t.layout == torch.strided and t.is_contiguous():
        (torch.view_as_real(t) if t.is_complex() else t).view(torch.uint8).fill_(byte)
    return t


@contextlib.contextmanager
def fresh_memory(byte):
    """Inside the block every tensor of ``torch.empty`` / ``torch.empty_like`` — device, pageable or page-locked host — holds ``byte`` in every
    byte.  ``None``: nothing is replaced.  Wrap the engine call only: an oracle has no business with it."""
    if byte is None:
        yield
        return
    empty, empty_like = torch.empty, torch.empty_like

    def filled_empty(*a, **k):
        return _filled(empty(*a, **k), byte)

    def filled_empty_like(*a, **k):
        return _filled(empty_like(*a, **k), byte)

    torch.empty, torch.empty_like = filled_empty, filled_empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def set_fill(monkeypatch, byte):
    """The engine's own fill for handles created from here on (the switch is read by dfx_model_create).  ``None``: unset."""
    if byte is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(int(byte)))
    assert os.environ.get(SWITCH) == (None if byte is None else str(int(byte)))


def bits(t):
    """A tensor / array as the integers of its bytes: NaNs compare like any other value (a paused stream's lsnr is NaN by contract)."""
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    return a.reshape(-1).view(np.uint8) if a.size else np.zeros(0, np.uint8)


def same_bits(a, b):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    if len(a) != len(b):
        return False
    for u, v in zip(a, b):
        if tuple(u.shape) != tuple(v.shape) or u.dtype != v.dtype or not np.array_equal(bits(u), bits(v)):
            return False
    return True


def assert_same_bits(runs, what=""):
    """runs: {fill: tensor or tuple of tensors}.  Every run has the bits of the first; the message names the fill, the output and the first
    element that differs."""
    keys = list(runs)
    base = runs[keys[0]]
    base = base if isinstance(base, (tuple, list)) else (base,)
    for k in keys[1:]:
        got = runs[k] if isinstance(runs[k], (tuple, list)) else (runs[k],)
        assert len(got) == len(base), (what, k)
        for i, (u, v) in enumerate(zip(base, got)):
            assert tuple(u.shape) == tuple(v.shape) and u.dtype == v.dtype, (what, k, i, u.shape, v.shape)
            bu, bv = bits(u), bits(v)
            if not np.array_equal(bu, bv):
                item = max(1, bu.size // max(1, int(np.prod(u.shape))))
                first = int(np.flatnonzero(bu != bv)[0]) // item
                n = int(np.count_nonzero((bu != bv).reshape(-1, item).any(1)))
                raise AssertionError(f"{what}: fill {_name(k)} differs from fill {_name(keys[0])} in output {i}: {n} of {bu.size // item} elements, "
                                     f"the first at flat index {first}")


def _name(k):
    return "unset" if k is None else f"0x{k:02X}" if isinstance(k, int) else str(k)
