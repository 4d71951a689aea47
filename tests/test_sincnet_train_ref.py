"""The float64 restatement of SincNet training (tests/sincnet_train_ref.py) against torch-float64 autograd on the CPU, on the shapes the
GPU tests use: feats and every parameter gradient to 1e-10 of the tensor's max-abs, the filter-bank chain rule included, with one band
edge driven into the clamp and one low_hz_ of exactly 0.  conv1d.{1,2}.bias gradients are mathematically zero (a bias in front of an
instance norm cancels): their difference is measured against the sum of the absolute terms, sum |du|."""
import numpy as np
import pytest
import torch

import sincnet_train_ref as R

SHAPES = [(1, 991), (2, 2071), (3, 8000), (2, 4003)]


def _case(B, S, seed, edge_cases=True):
    p = R.init_params(seed)
    if edge_cases:
        p["conv1d.0.filterbank.band_hz_"][39, 0] = 9000.0      # low + 50 + band > 8000: clamped, no gradient through the clamp
        p["conv1d.0.filterbank.low_hz_"][0, 0] = 0.0           # torch.abs's sign(0) = 0
        p["conv1d.0.filterbank.band_hz_"][7, 0] *= -1.0        # a negative edge: sign -1
    g = torch.Generator().manual_seed(1000 + seed)
    wav = (0.1 * torch.randn(B, S, generator=g)).numpy().astype(np.float32)
    dfeats = torch.randn(B, R.num_frames(S), R.C3, generator=g).numpy().astype(np.float32)
    return p, wav, dfeats


@pytest.mark.parametrize("B,S", SHAPES)
def test_restatement_equals_torch_float64_autograd(B, S):
    p, wav, dfeats = _case(B, S, seed=3)
    feats, cache = R.forward(p, wav)
    grads, bias_abs = R.backward(p, cache, dfeats)
    tf, tg, _ = R.torch_forward_backward(p, wav, dfeats, torch.float64)
    assert feats.shape == tf.shape == (B, R.num_frames(S), R.C3)
    assert np.abs(feats - tf).max() <= 1e-10 * np.abs(tf).max()
    if R.num_frames(S) == 1:
        # the last norm sees one position: xhat = 0, so only norm1d.2.bias gets a gradient and everything else is exactly 0
        top = np.abs(tg["norm1d.2.bias"]).max()
        assert top > 0 and np.abs(grads["norm1d.2.bias"] - tg["norm1d.2.bias"]).max() <= 1e-10 * top
        for k, _ in R.keys():
            if k != "norm1d.2.bias":
                assert not grads[k].any(), k
                assert np.abs(tg[k]).max() <= 1e-10 * top, k
        return
    for k, shape in R.keys():
        assert grads[k].shape == tuple(shape) == tg[k].shape
        scale = bias_abs[k].max() if k in bias_abs else np.abs(tg[k]).max()
        assert scale > 0 and np.abs(grads[k] - tg[k]).max() <= 1e-10 * scale, (k, np.abs(grads[k] - tg[k]).max() / scale)
    assert grads["conv1d.0.filterbank.band_hz_"][39, 0] == 0.0 and grads["conv1d.0.filterbank.low_hz_"][0, 0] == 0.0
    assert grads["conv1d.0.filterbank.band_hz_"][7, 0] != 0.0


def test_bank_restatement_pack_and_first_stage():
    p, wav, dfeats = _case(2, 2071, seed=5)
    bank = R.filters(p["conv1d.0.filterbank.low_hz_"], p["conv1d.0.filterbank.band_hz_"])
    tb = R.torch_filters(torch.tensor(p["conv1d.0.filterbank.low_hz_"], dtype=torch.float64),
                         torch.tensor(p["conv1d.0.filterbank.band_hz_"], dtype=torch.float64), torch.float64)[:, 0].numpy()
    assert bank.shape == (80, 251) and np.abs(bank - tb).max() <= 1e-12
    # the module's own f32 filters() differs from the float64 bank by f32 rounding only
    from uvad_amd.sincnet import ParamSincFB
    fb = ParamSincFB(80, 251, stride=10)
    assert np.array_equal(fb.window_.numpy(), R.buffers()[0]) and np.array_equal(fb.n_.numpy().reshape(-1), R.buffers()[1])
    with torch.no_grad():
        fb.low_hz_.copy_(torch.from_numpy(p["conv1d.0.filterbank.low_hz_"]))
        fb.band_hz_.copy_(torch.from_numpy(p["conv1d.0.filterbank.band_hz_"]))
    assert np.abs(fb.filters()[:, 0].numpy() - bank).max() <= 1e-4
    assert [len(R.pack(p, f)) for f in (0, 1, 2)] == [42602, 42360, 18180]
    for f in (0, 1, 2):
        back = R.unpack(R.pack(p, f), f)
        assert list(back) == [k for k, _ in R.keys(f)] and all(np.array_equal(back[k], p[k]) for k in back)
    # frozen stages get no gradient; the learning stages' gradients do not depend on where the walk stops
    _, cache = R.forward(p, wav)
    g0, _ = R.backward(p, cache, dfeats, 0)
    for f in (1, 2):
        gf, _ = R.backward(p, cache, dfeats, f)
        assert list(gf) == [k for k, _ in R.keys(f)] and all(np.array_equal(gf[k], g0[k]) for k in gf)
    m = R.margins(cache)
    assert len(m) == 3 and all(v["pool"] >= 0 and v["leaky"] >= 0 for v in m) and np.isfinite(m[0]["abs"]) and np.isinf(m[1]["abs"])
