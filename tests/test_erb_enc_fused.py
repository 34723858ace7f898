"""The ERB branch of the encoder as one frame-resident kernel (dfx_k_erb_enc4: erb_conv0 -> erb_conv1 -> erb_conv2 -> erb_conv3, e1 / e2 / e3
written once from LDS strips) against the three-launch form it replaces in batch passes (dfx_k_erb_enc + dfx_k_pwconv_f x 2, selected by the
test hook DFX_ERB_ENC_SPLIT=1, read when the model handle is created): the same bits, the torch oracle within the project's bar for
enhance(), and the passes that must keep the old kernels (exact fp32, streaming) still do.

e1 / e2 / e3 have no entry point of their own: they are compared through everything that reads them — DfNet.forward's mask (the decoder
tail reads e1, e2 and e3), lsnr and DF coefficients (both behind e3), and the waveform of enhance()."""
import numpy as np
import pytest
import torch

from oracle import dfnet_oracle as O
from tests.helpers import named_params, rms, torch_sd

HOP = 480
SEED = 21
ENC_SCOPES = ["dfx_k_erb_enc", "dfx_k_pwconv"]


def _noise(shape, seed):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32))


def _init(monkeypatch, split, **kw):
    """DeepFilterNet3 with seeded weights (random_state_dict(p, SEED, widths=widths_for(p))); split: the three-launch form in batch passes."""
    from deepfilternet_amd.enhance import init_df

    if split:
        monkeypatch.setenv("DFX_ERB_ENC_SPLIT", "1")
    else:
        monkeypatch.delenv("DFX_ERB_ENC_SPLIT", raising=False)
    p = named_params("df3")
    model, df_state, _, _ = init_df(params=p, epoch="none", seed=SEED, **kw)
    monkeypatch.delenv("DFX_ERB_ENC_SPLIT", raising=False)
    return p, model, df_state


def _launches(fn):
    """fn() with the launch counters of the encoder's scopes on -> (result, {scope: launches})"""
    from deepfilternet_amd import _lib

    _lib.prof_enable(ENC_SCOPES)
    try:
        _lib.prof_reset()
        out = fn()
        r = _lib.prof_read()
    finally:
        _lib.prof_enable(None)
    return out, {k: r.get(k, (0.0, 0))[1] for k in ENC_SCOPES}


def _two_more(n_fused, n_split):
    """Both forms record their encoder launch in the dfx_k_erb_enc scope; the three-launch form adds erb_conv2 and erb_conv3 in the dfx_k_pwconv
    scope (which other layers of the pass share): two more per encoder launch shows that the two handles ran the two forms."""
    print(f"launches fused {n_fused}, split {n_split}")
    assert n_fused["dfx_k_erb_enc"] == n_split["dfx_k_erb_enc"] >= 1
    assert n_split["dfx_k_pwconv"] == n_fused["dfx_k_pwconv"] + 2 * n_split["dfx_k_erb_enc"]


@pytest.fixture
def both(backend, monkeypatch):
    """(p, fused model, its state, split model, its state) on the fixture's backend"""
    p, fused, st_f = _init(monkeypatch, False)
    _, split, st_s = _init(monkeypatch, True)
    return p, fused, st_f, split, st_s


def test_fused_equals_three_launches_and_oracle(both):
    """B = 3 clips of 480 * 13 + 5 samples: 16 frames per clip, 48 frames = four whole workgroups of 12 waves; the first two frames of a clip
    and its last two take the causal / beyond-T zero rows of erb_conv0, the others do not.  Both forms ran (launch counts), the same bits,
    and rows 0 and 1 against the torch oracle: < 2e-6 RMS, the project's bar for enhance()."""
    from deepfilternet_amd.enhance import enhance

    p, fused, st_f, split, st_s = both
    x = _noise((3, HOP * 13 + 5), 1)
    y_f, n_f = _launches(lambda: enhance(fused, st_f, x))
    fused.check()
    y_s, n_s = _launches(lambda: enhance(split, st_s, x))
    split.check()
    _two_more(n_f, n_s)
    assert float(y_f.abs().max()) > 1e-4
    assert torch.equal(y_f, y_s)
    ref = O.enhance(p, torch_sd(p, SEED), x[:2].numpy())
    err = rms(y_f[:2].cpu().numpy() - ref)
    print(f"fused enhance() vs torch oracle, rows 0-1: {err:.3e}")
    assert err < 2e-6


def test_forward_outputs_bit_equal(both):
    """DfNet.forward on 1 x 21 frames (a workgroup of 12 waves and one with three idle waves): mask (reads e1, e2, e3), lsnr and DF
    coefficients (behind e3) and the enhanced spectrum, bit for bit."""
    p, fused, _, split, _ = both
    B, T = 1, 21
    rng = np.random.default_rng(4)
    spec = torch.from_numpy((0.05 * rng.standard_normal((B, 1, T, p.freq_bins, 2))).astype(np.float32))
    fe = torch.from_numpy((0.5 * rng.standard_normal((B, 1, T, p.nb_erb))).astype(np.float32))
    fs = torch.from_numpy(rng.standard_normal((B, 1, T, p.nb_df, 2)).astype(np.float32))
    (out_f, n_f) = _launches(lambda: fused(spec, fe, fs))
    (out_s, n_s) = _launches(lambda: split(spec, fe, fs))
    fused.check(), split.check()
    _two_more(n_f, n_s)
    for name, a, b in zip(("spec_e", "mask", "lsnr", "df_coefs"), out_f, out_s):
        assert float(a.abs().max()) > 0, name
        assert torch.equal(a, b), name


def test_fewer_frames_than_the_taps_reach(both):
    """B = 1, 480 * 2 + 1 samples: three frames, fewer than the lookahead plus the two causal taps — every tap row of every frame but the
    frame's own is on the `tau < 0` or `tin >= T` zero path of erb_conv0; one workgroup with nine idle waves."""
    from deepfilternet_amd.enhance import enhance

    p, fused, st_f, split, st_s = both
    x = _noise((1, HOP * 2 + 1), 2)
    y_f, y_s = enhance(fused, st_f, x), enhance(split, st_s, x)
    fused.check(), split.check()
    assert float(y_f.abs().max()) > 1e-5
    assert torch.equal(y_f, y_s)
    assert rms(y_f.cpu().numpy() - O.enhance(p, torch_sd(p, SEED), x.numpy())) < 2e-6


def test_time_chunked_pass(both):
    """A pass cut into time chunks (the layer-pipelined GRU phase, three chunks of >= 2 frames): the front runs in front of it as before."""
    from deepfilternet_amd.enhance import enhance

    p, fused, st_f, split, st_s = both
    x = _noise((3, HOP * 9 + 7), 5)   # 11 frames with the padding
    fused.set_pipeline(time_chunks=3, min_chunk_frames=2)
    split.set_pipeline(time_chunks=3, min_chunk_frames=2)
    y_f, n_f = _launches(lambda: enhance(fused, st_f, x))
    y_s, n_s = _launches(lambda: enhance(split, st_s, x))
    fused.check(), split.check()
    _two_more(n_f, n_s)
    assert torch.equal(y_f, y_s)


def test_rows_of_different_lengths(both):
    """One enhance_batch call with rows of 480 * 5, 480 * 13 + 7 and 480 * 9 samples: one pass over the frames of the longest row, the
    feature rows past a row's end are zeros."""
    from deepfilternet_amd.enhance import enhance_batch

    p, fused, st_f, split, st_s = both
    clips = [_noise((n,), 30 + i) for i, n in enumerate((HOP * 5, HOP * 13 + 7, HOP * 9))]
    ys_f, n_f = _launches(lambda: enhance_batch(fused, st_f, clips))
    ys_s, n_s = _launches(lambda: enhance_batch(split, st_s, clips))
    fused.check(), split.check()
    _two_more(n_f, n_s)
    for c, a, b in zip(clips, ys_f, ys_s):
        assert a.shape == c.shape and float(a.abs().max()) > 1e-4
        assert torch.equal(a, b)


def test_exact_fp32_keeps_the_old_kernels(backend, monkeypatch):
    """DFX_EXACT_FP32=1: dfx_k_erb_enc + dfx_k_pwconv x 2 on fp32 matrix ops, and the oracle comparison of the exact path."""
    from deepfilternet_amd.enhance import enhance

    monkeypatch.setenv("DFX_EXACT_FP32", "1")
    p, model, df_state = _init(monkeypatch, False)
    assert model.query(model.Q_EXACT_FP32) == 1
    x = _noise((2, HOP * 5 + 3), 6)
    y, n = _launches(lambda: enhance(model, df_state, x))
    model.check()
    assert n["dfx_k_erb_enc"] >= 1 and n["dfx_k_pwconv"] >= 2 * n["dfx_k_erb_enc"]
    assert rms(y.cpu().numpy() - O.enhance(p, torch_sd(p, SEED), x.numpy())) < 2e-6


def test_streams_keep_the_old_kernels(backend, monkeypatch):
    """A DfStream of two streams (frame ranges through row maps): dfx_k_erb_enc + dfx_k_pwconv_f x 2 per call, and the stream equals the
    batch path — the fused kernel — delayed by the lookahead, itself held to the torch oracle."""
    from deepfilternet_amd.enhance import enhance
    from deepfilternet_amd.streaming import DfStream

    p, model, df_state = _init(monkeypatch, False)
    T = 7
    x = _noise((2, HOP * T), 7)
    ref = enhance(model, df_state, x, pad=False)
    assert rms(ref.cpu().numpy() - O.enhance(p, torch_sd(p, SEED), x.numpy(), pad=False)) < 2e-6
    rt = DfStream(model, df_state, streams=2, max_frames=3)
    d = rt.delay_frames
    out, pos = [], 0
    n_all = {k: 0 for k in ENC_SCOPES}
    for n in (3, 1, 2, 1):
        y, cnt = _launches(lambda: rt.process(x[:, pos * HOP:(pos + n) * HOP]).cpu())
        out.append(y)
        pos += n
        if pos > d:   # (calls that only carry warm-up hops run no network pass)
            assert cnt["dfx_k_pwconv"] >= 2 * cnt["dfx_k_erb_enc"] >= 2, cnt
        for k in ENC_SCOPES:
            n_all[k] += cnt[k]
    model.check()
    y = torch.cat(out, dim=1)
    print(f"stream launches {n_all}")
    assert float(y[:, : d * HOP].abs().max()) == 0.0
    err = rms((y[:, d * HOP:] - ref.cpu()[:, : (T - d) * HOP]).numpy())
    print(f"stream vs batch path delayed: {err:.3e}")
    assert err < 1e-6
