"""tests/resnet_ref.py against torch's own float64 operators (no GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as R


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@pytest.mark.parametrize("cin,h,w", [(1, 11, 13), (3, 9, 131), (4, 7, 8), (3, 1, 1)])
def test_stem7_is_torch_conv2d(cin, h, w):
    r = _rng(cin, h, w)
    x, wt = r.standard_normal((2, cin, h, w)), r.standard_normal((64, cin, 7, 7))
    sc, sh = r.standard_normal(64), r.standard_normal(64)
    want = F.conv2d(torch.from_numpy(x), torch.from_numpy(wt), None, 2, 3)
    got, bound = R.stem7(x, wt)
    assert got.shape == (2, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64)
    np.testing.assert_allclose(got, want.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    want = torch.relu(want * torch.from_numpy(sc).view(1, -1, 1, 1) + torch.from_numpy(sh).view(1, -1, 1, 1))
    got, bound = R.stem7(x, wt, sc, sh, True)
    np.testing.assert_allclose(got, want.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    mag = F.conv2d(torch.from_numpy(np.abs(x)), torch.from_numpy(np.abs(wt)), None, 2, 3).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(bound, R.gamma(49 * cin + 2) * (mag * np.abs(sc) + np.abs(sh)), rtol=1e-12)
    assert (bound > 0).all()


@pytest.mark.parametrize("k,stride,pad", [(1, 2, 0), (3, 2, 1), (3, 1, 1), (1, 1, 0)])
def test_conv_nhwc_is_torch_conv2d(k, stride, pad):
    r = _rng(k, stride)
    x, wt = r.standard_normal((2, 9, 13, 8)), r.standard_normal((12, 8, k, k))
    want = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), None, stride, pad).permute(0, 2, 3, 1).numpy()
    got, bound = R.conv_nhwc(x, wt, stride, pad)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert bound.shape == got.shape and (bound >= 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 2, 3, 8), (1, 7, 9, 64), (1, 16, 24, 12), (1, 5, 1, 4)])
def test_maxpool_is_torch_max_pool2d(shape):
    x = _rng(*shape).standard_normal(shape).astype(np.float32)
    x[0, 0, 0, 0] = -np.inf
    x[0, -1, -1, 1] = -np.inf
    want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    got = R.maxpool3s2_pad1(x)
    assert got.shape == (shape[0], R.pool3s2p1_out(shape[1]), R.pool3s2p1_out(shape[2]), shape[3])
    assert np.array_equal(got.astype(np.float64), want)


def test_a_window_of_minus_infinity_gives_minus_infinity():
    x = np.full((1, 4, 4, 4), -np.inf, np.float32)
    assert np.all(R.maxpool3s2_pad1(x) == -np.inf)


def test_gamma_and_the_order_of_the_residual_add():
    assert R.gamma(1) == pytest.approx(2.0 ** -24) and R.gamma(147 + 2) < 1e-5
    z, res = np.float32([1.5, -2.0, 0.25]), np.float32([-1.0, -3.0, 4.0])
    assert np.array_equal(R.residual_act(z, res, True), torch.relu(torch.tensor(z) + torch.tensor(res)).numpy())
    assert np.array_equal(R.residual_act(z, res, False), z + res)
    assert np.array_equal(R.fpn_order(z, res, True), (torch.relu(torch.tensor(z)) + torch.tensor(res)).numpy())
    assert not np.array_equal(R.residual_act(z, res, True), R.fpn_order(z, res, True))
