"""float64 restatement of the libDF half of the engine (TEST INFRASTRUCTURE ONLY): analysis, the ERB feature, the two norm scans, the finishing
steps of enhance() and the synthesis, in numpy.

It follows the semantics oracle/df_oracle.c restates (the lib.rs / transforms.rs lines are cited there and repeated here) and is the reference
both the C oracle and the kernels are measured against: |C oracle - dsp64| is float32's own error on a case (E32), and a kernel is held to a
small multiple of it (tests/helpers.py hold_to_f64).  What a DFState holds as float32 enters as those float32 values, so that the float64 result
differs from the float32 ones by rounding only: the window (lib.rs:126-133 casts it), the analysis factor (lib.rs:134), the initial norm states
(the f32 step form of ndarray's linspace), the ERB floor 1e-10f, and what the engine is handed as float32: alpha and the attenuation factor.
Everything computed from them is float64.

The keyword arguments that say "mutant" deliberately compute something else: tests/test_dsp_levels.py uses them to show that its bound sees the
defects it is for.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

F32 = np.float32
ERB_FLOOR = float(F32(1e-10))   # transforms.rs:249-251: (x + 1e-10).log10() * 10 on f32


def window(N: int) -> np.ndarray:
    """lib.rs:126-133: the Vorbis window over window_size_h = N / 2, computed in f64 and stored as f32."""
    s = np.sin(0.5 * np.pi * (np.arange(N, dtype=np.float64) + 0.5) / (N // 2))
    return np.sin(0.5 * np.pi * s * s).astype(F32).astype(np.float64)


def wnorm(N: int, hop: int) -> float:
    """lib.rs:134: 1 / (N^2 / (2 hop)) = 2 hop / N^2, in f32."""
    return float(F32(1.0) / (F32(N * N) / F32(2 * hop)))


def analysis(x: np.ndarray, N: int, hop: int, mem: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """lib.rs:356-394 frame_analysis over [C, T] samples: frame t = rfft(window * stream[t hop : t hop + N]) * wnorm with
    stream = [mem (N - hop samples, zeros when None) ; x].  Returns (spec [C, T // hop, N / 2 + 1] complex128, the memory after the last frame)."""
    x = np.asarray(x, dtype=np.float64)
    C, T = x.shape
    Tf, ML = T // hop, N - hop
    m = np.zeros((C, ML)) if mem is None else np.asarray(mem, dtype=np.float64).reshape(C, ML)
    stream = np.concatenate([m, x[:, :Tf * hop]], axis=1)
    idx = np.arange(Tf)[:, None] * hop + np.arange(N)[None, :]
    frames = stream[:, idx] * window(N)                     # [C, Tf, N]
    spec = np.fft.rfft(frames, n=N, axis=-1) * wnorm(N, hop)
    return spec, stream[:, Tf * hop: Tf * hop + ML].copy()


def synthesis(S: np.ndarray, N: int, hop: int, mem: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """lib.rs:396-427 frame_synthesis over [C, Tf, N / 2 + 1] spectra: the unnormalised C2R transform (N * irfft; it ignores the imaginary parts
    of DC and Nyquist), times the window, overlap-added.  Returns (Tf * hop samples, the N - hop tail = the memory for the next call)."""
    S = np.array(S, dtype=np.complex128)
    C, Tf, F = S.shape
    assert F == N // 2 + 1
    ML = N - hop
    S[..., 0] = S[..., 0].real
    S[..., -1] = S[..., -1].real
    x = np.fft.irfft(S, n=N, axis=-1) * N * window(N)      # [C, Tf, N]
    buf = np.zeros((C, Tf * hop + ML))
    if mem is not None:
        buf[:, :ML] = np.asarray(mem, dtype=np.float64).reshape(C, ML)
    for t in range(Tf):
        buf[:, t * hop: t * hop + N] += x[:, t]
    return buf[:, :Tf * hop].copy(), buf[:, Tf * hop:].copy()


def _starts(widths) -> np.ndarray:
    w = np.asarray(widths, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(w)[:-1]])


def erb_db(spec: np.ndarray, widths, db: bool = True, floor: float = ERB_FLOOR) -> np.ndarray:
    """lib.rs:280-295 compute_band_corr(x, x): sum over the band of |x|^2 * (1 / width), the factor inside the sum; transforms.rs:249-251:
    10 log10(e + 1e-10).  ``floor``: the 1e-10 (a mutant passes another value)."""
    w = np.asarray(widths, dtype=np.int64)
    spec = np.asarray(spec, dtype=np.complex128)
    assert spec.shape[-1] == int(w.sum())
    p = (spec.real ** 2 + spec.imag ** 2) * np.repeat(1.0 / w, w)
    e = np.add.reduceat(p, _starts(w), axis=-1)
    return 10.0 * np.log10(e + floor) if db else e


def linspace32(a: float, b: float, n: int) -> np.ndarray:
    """ndarray::Array1::linspace in f32, the step form (a + step * i), as float64 values: the initial states of the two norms."""
    step = (F32(b) - F32(a)) / F32(n - 1) if n > 1 else F32(0)
    return (F32(a) + step * np.arange(n, dtype=F32)).astype(np.float64)


def erb_norm(x: np.ndarray, alpha: float, state: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """transforms.rs:301-330 + lib.rs:244-251 over [C, T, E]: s = x (1 - alpha) + s alpha; (x - s) / 40.  Returns (normed, state after T frames);
    ``state`` [C, E], None: linspace(-60, -90, E)."""
    x = np.asarray(x, dtype=np.float64)
    C, T, E = x.shape
    a = float(F32(alpha))
    s = np.tile(linspace32(-60.0, -90.0, E), (C, 1)) if state is None else np.array(state, dtype=np.float64).reshape(C, E)
    out = np.empty_like(x)
    for t in range(T):
        s = x[:, t] * (1.0 - a) + s * a
        out[:, t] = (x[:, t] - s) / 40.0
    return out, s


def unit_norm(spec: np.ndarray, alpha: float, state: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """transforms.rs:332-361 + lib.rs:253-259 over [C, T, F] complex: s = |x| (1 - alpha) + s alpha; x / sqrt(s).  Returns (normed, state);
    ``state`` [C, F], None: linspace(1e-3, 1e-4, F)."""
    spec = np.asarray(spec, dtype=np.complex128)
    C, T, F = spec.shape
    a = float(F32(alpha))
    s = np.tile(linspace32(0.001, 0.0001, F), (C, 1)) if state is None else np.array(state, dtype=np.float64).reshape(C, F)
    out = np.empty_like(spec)
    for t in range(T):
        s = np.abs(spec[:, t]) * (1.0 - a) + s * a
        out[:, t] = spec[:, t] / np.sqrt(s)
    return out, s


def band_gain(spec: np.ndarray, gains: np.ndarray, widths, mutant_bin: Optional[int] = None) -> np.ndarray:
    """lib.rs:314-326 apply_interp_band_gain: every bin of band b times gains[..., b].  ``mutant_bin``: that one bin takes the gain of the band
    below its own."""
    w = np.asarray(widths, dtype=np.int64)
    band = np.repeat(np.arange(len(w)), w)
    if mutant_bin is not None:
        assert band[mutant_bin] > 0 and band[mutant_bin - 1] == band[mutant_bin] - 1, "the mutant bin is the first of its band"
        band = band.copy()
        band[mutant_bin] -= 1
    return np.asarray(spec, dtype=np.complex128) * np.asarray(gains, dtype=np.float64)[..., band]


def df_apply(spec: np.ndarray, coefs: np.ndarray, order: int, lookahead: int, nb_df: int, mutant_clamp: bool = False) -> np.ndarray:
    """multiframe.py:85-95,126-136,169-180: Y[b, t, f] = sum_n coefs[b, n, t, f] * spec[b, t + n - (order - 1 - lookahead), f], zero outside
    [0, T).  spec [B, T, F], coefs [B, order, T, nb_df] -> [B, T, nb_df].  ``mutant_clamp``: frames behind the last one read the last one."""
    spec = np.asarray(spec, dtype=np.complex128)
    B, T, _ = spec.shape
    out = np.zeros((B, T, nb_df), dtype=np.complex128)
    for n in range(order):
        src = np.arange(T) + n - (order - 1 - lookahead)
        ok = (src >= 0) & (src < T)
        if mutant_clamp:
            ok = src >= 0
        x = spec[:, np.clip(src, 0, T - 1), :nb_df] * ok[None, :, None]
        out += np.asarray(coefs)[:, n] * x
    return out


def post_filter(spec: np.ndarray, spec_e: np.ndarray, beta: float) -> np.ndarray:
    """deepfilternet3.py:448-454 (every bin, as enhance() applies it)."""
    eps = 1e-12
    mask = np.clip(np.abs(spec_e) / (np.abs(spec) + eps), eps, 1.0)
    mask_sin = mask * np.maximum(np.sin(np.pi * mask / 2.0), eps)
    return spec_e * ((1.0 + beta) / (1.0 + beta * (mask / mask_sin) ** 2))


def atten_factor(atten_lim_db: float) -> float:
    """enhance.py:238-239: 10 ** (-|dB| / 20), as the float32 value the engine computes (powf)."""
    return float(np.power(F32(10.0), -np.abs(F32(atten_lim_db)) / F32(20.0)))


def atten_limit(spec: np.ndarray, enhanced: np.ndarray, atten_lim_db: Optional[float]) -> np.ndarray:
    """enhance.py:236-240: spec * lim + enhanced * (1 - lim); None or 0 dB: no limit."""
    if atten_lim_db is None or abs(atten_lim_db) == 0:
        return enhanced
    lim = atten_factor(atten_lim_db)
    return spec * lim + enhanced * (1.0 - lim)


def features64(audio: np.ndarray, p, widths, erb_floor: float = ERB_FLOOR):
    """enhance.py:190-203 df_features: (spec [C, T', F], feat_erb [C, T', E], feat_spec [C, T', nb_df]) in float64."""
    alpha = float(F32(p.norm_alpha()))
    spec, _ = analysis(audio, p.fft_size, p.hop_size)
    fe, _ = erb_norm(erb_db(spec, widths, floor=erb_floor), alpha)
    fs, _ = unit_norm(spec[..., :p.nb_df], alpha)
    return spec, fe, fs


MUTANTS = ("erb_floor", "gain_bin", "df_clamp")


def enhance64(p, sd64, audio: np.ndarray, pad: bool = True, atten_lim_db: Optional[float] = None, mutant: Optional[str] = None,
              check_finish: bool = False) -> np.ndarray:
    """The steps of oracle/dfnet_oracle.py enhance() in float64: features64, dfnet_forward on a float64 state dict (to_dtype) with the manual GRU,
    then the finishing steps restated above — band gains, deep filter on the noisy spectrum below nb_df, post filter, attenuation limit —
    and the synthesis.  audio [C, T] -> float64 [C, T] (pad) or [C, T // hop * hop].

    ``mutant`` (one of MUTANTS) computes a defect on purpose: the ERB floor at 2e-10; the first bin of the first band that starts above nb_df
    with the gain of the band below; the deep filter's look-ahead taps clamped to the last frame.  ``check_finish``: assert that the finishing
    steps here equal dfnet_forward's own."""
    import torch

    from . import dfnet_oracle as O
    from . import libdf_oracle as L

    assert mutant is None or mutant in MUTANTS, mutant
    N, hop = p.fft_size, p.hop_size
    widths = L.erb_fb_widths(p.sr, N, p.nb_erb, p.min_nb_freqs)
    audio = np.asarray(audio, dtype=np.float64)
    orig_len = audio.shape[-1]
    if pad:
        audio = np.pad(audio, ((0, 0), (0, N)))
    spec, fe, fs = features64(audio, p, widths, erb_floor=2e-10 if mutant == "erb_floor" else ERB_FLOOR)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = O.dfnet_forward(p, sd64, widths, torch.view_as_real(t(spec)).unsqueeze(1), t(fe).unsqueeze(1),
                          torch.view_as_real(t(fs)).unsqueeze(1), manual_gru=True)
    assert out["spec_e"].dtype == torch.float64
    mbin = None
    if mutant == "gain_bin":
        mbin = int(next(s for s in _starts(widths)[1:] if s > p.nb_df))
    enh = band_gain(spec, out["m"].squeeze(1).numpy(), widths, mutant_bin=mbin)
    coefs = torch.view_as_complex(out["df_coefs"].contiguous()).numpy()
    enh[..., :p.nb_df] = df_apply(spec, coefs, p.df_order, p.df_lookahead, p.nb_df, mutant_clamp=mutant == "df_clamp")
    if p.mask_pf:
        enh = post_filter(spec, enh, p.pf_beta)
    if check_finish:
        own = torch.view_as_complex(out["spec_e"].squeeze(1).contiguous()).numpy()
        assert mutant is None and np.abs(enh - own).max() <= 1e-12 * max(1.0, np.abs(own).max())
    enh = atten_limit(spec, enh, atten_lim_db)
    y, _ = synthesis(enh, N, hop)
    if pad:
        d = N - hop
        y = y[:, d: orig_len + d]
    return y
