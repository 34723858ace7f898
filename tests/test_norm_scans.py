"""The two norm scans (erb_norm, unit_norm) at the lengths where their loops change, against the float64 restatement oracle/dsp64.py.

Calls of 16 frames or more take dfx_k_norm_scan4 (four lanes per channel: batches of DFX_SCAN_UNROLL = 16 frames, double-buffered, then a tail in
groups of four), shorter ones dfx_k_norm_scan (one lane per channel).  LENGTHS covers the quad tail (1 ... 5 frames behind a batch), one batch and
its neighbours, the double buffer's last batch (two and three batches) and a long odd call; 3 clips by 32 bands and 5 clips by 7 bins leave the
last workgroup, and with 7 bins the last wave, partly empty.  Each length runs without a state and with a caller's; the state after T frames, fed
into a second call, must give the bits of one call over both (the second call is short where the first took the batched kernel and the other way
round).  The bound is tests/helpers.py hold_to_f64; whether the result equals the C oracle's bit for bit is printed, not asserted."""
import functools

import numpy as np
import pytest
import torch

from oracle import dsp64 as R
from oracle import libdf_oracle as L
from tests.helpers import hold_to_f64

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 130]
ALPHA = 0.99


def _second(T):
    return 5 if T >= 16 else 19


@functools.lru_cache(maxsize=None)
def reference(T):
    """Inputs of T + _second(T) frames, caller's states, and both oracles' results with the states they leave; computed once, left unchanged."""
    rng = np.random.default_rng(T)
    Tt = T + _second(T)
    e = (rng.standard_normal((3, Tt, 32)) * 8 - 50).astype(np.float32)
    X = (rng.standard_normal((5, Tt, 7)) + 1j * rng.standard_normal((5, Tt, 7))).astype(np.complex64)
    st_e = (rng.standard_normal((3, 32)) - 70).astype(np.float32)
    st_u = rng.uniform(1e-4, 1e-3, (5, 7)).astype(np.float32)
    out = {"e": e, "X": X, "st_e": st_e, "st_u": st_u}
    for n in (T, Tt):   # the first call alone, and one call over both
        ce, cs = e[:, :n].copy(), st_e.copy()
        L.lib().dfo_erb_norm(L._fp(ce), 3, n, 32, ALPHA, L._fp(cs))
        cu, cus = X[:, :n].copy(), st_u.copy()
        L.lib().dfo_unit_norm(L._fp(cu.view(np.float32)), 5, n, 7, ALPHA, L._fp(cus))
        out[n] = {"c_e": L.erb_norm(e[:, :n].copy(), ALPHA), "r_e": R.erb_norm(e[:, :n], ALPHA)[0],
                  "c_u": L.unit_norm(X[:, :n], ALPHA), "r_u": R.unit_norm(X[:, :n], ALPHA)[0],
                  "c_es": (ce, cs), "r_es": R.erb_norm(e[:, :n], ALPHA, st_e), "c_us": (cu, cus), "r_us": R.unit_norm(X[:, :n], ALPHA, st_u)}
    return out


def _erb_norm(x, st):
    """dfx_erb_norm on copies: (normed, the state it leaves)"""
    from deepfilternet_amd import _lib

    xt, stt = torch.from_numpy(x.copy()).to(_lib.device()), torch.from_numpy(st.copy()).to(_lib.device())
    _lib.check(_lib.lib().dfx_erb_norm(_lib.ptr(xt), x.shape[0], x.shape[1], x.shape[2], ALPHA, _lib.ptr(stt), _lib.stream()))
    return xt.cpu().numpy(), stt.cpu().numpy()


def _unit_norm(X, st):
    from deepfilternet_amd import _lib

    xt, stt = torch.from_numpy(X.copy()).to(_lib.device()), torch.from_numpy(st.copy()).to(_lib.device())
    out = torch.empty_like(xt)
    _lib.check(_lib.lib().dfx_unit_norm(_lib.ptr(torch.view_as_real(xt)), X.shape[2], _lib.ptr(torch.view_as_real(out)), X.shape[0], X.shape[1],
                                        X.shape[2], ALPHA, _lib.ptr(stt), _lib.stream()))
    return out.cpu().numpy(), stt.cpu().numpy()


@pytest.mark.parametrize("T", LENGTHS)
def test_norm_scans_hold_to_float64(backend, T):
    from deepfilternet_amd import libdf as D

    ref = reference(T)
    e, X, st_e, st_u, r, rt = ref["e"], ref["X"], ref["st_e"], ref["st_u"], ref[T], ref[T + _second(T)]
    tag = f"T = {T} [{backend}]"
    # without a state
    hold_to_f64(D.erb_norm(e[:, :T].copy(), ALPHA), r["c_e"], r["r_e"], f"{tag} erb_norm")
    hold_to_f64(D.unit_norm(X[:, :T].copy(), ALPHA), r["c_u"], r["r_u"], f"{tag} unit_norm")
    # with a caller's state, and the state it leaves
    a, sa = _erb_norm(e[:, :T], st_e)
    hold_to_f64(a, r["c_es"][0], r["r_es"][0], f"{tag} erb_norm from a state")
    hold_to_f64(sa, r["c_es"][1], r["r_es"][1], f"{tag} erb_norm state after")
    u, su = _unit_norm(X[:, :T], st_u)
    hold_to_f64(u, r["c_us"][0], r["r_us"][0], f"{tag} unit_norm from a state")
    hold_to_f64(su, r["c_us"][1], r["r_us"][1], f"{tag} unit_norm state after")
    assert np.array_equal(D.erb_norm(e[:, :T].copy(), ALPHA, st_e.copy()), a)          # (the libdf front end takes the same path)
    # the state after T frames continues the scan: the bits of one call over both parts
    b, sb = _erb_norm(e[:, T:], sa)
    whole, sw = _erb_norm(e, st_e)
    assert np.array_equal(np.concatenate([a, b], 1), whole) and np.array_equal(sb, sw), (tag, "erb_norm continued")
    hold_to_f64(whole, rt["c_es"][0], rt["r_es"][0], f"{tag} erb_norm over {e.shape[1]} frames")
    v, sv = _unit_norm(X[:, T:], su)
    whole, sw = _unit_norm(X, st_u)
    assert np.array_equal(np.concatenate([u, v], 1), whole) and np.array_equal(sv, sw), (tag, "unit_norm continued")
    hold_to_f64(whole, rt["c_us"][0], rt["r_us"][0], f"{tag} unit_norm over {X.shape[1]} frames")
