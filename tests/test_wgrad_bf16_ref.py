"""tests/wgrad_bf16_ref.py states the definition of srf_conv_wgrad_nhwc_bf16 in numpy; here that statement is held to the formula
written out as loops and to torch's float64 autograd.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bf16_ref import bf16_round
from wgrad_bf16_ref import wgrad


def _naive(g, x, k):
    N, H, W, Cin = x.shape
    Cout = g.shape[3]
    pad = k // 2
    gr, xr = bf16_round(g).astype(np.float64), bf16_round(x).astype(np.float64)
    dW = np.zeros((Cout, Cin, k, k))
    for co in range(Cout):
        for ci in range(Cin):
            for ky in range(k):
                for kx in range(k):
                    s = 0.0
                    for n in range(N):
                        for y in range(H):
                            for xx in range(W):
                                iy, ix = y + ky - pad, xx + kx - pad
                                if 0 <= iy < H and 0 <= ix < W:
                                    s += gr[n, y, xx, co] * xr[n, iy, ix, ci]
                    dW[co, ci, ky, kx] = s
    return dW


@pytest.mark.parametrize("k", [1, 3])
def test_the_definition_equals_naive_loops(k):
    r = np.random.default_rng(k)
    g = r.standard_normal((1, 3, 5, 4)).astype(np.float32)
    x = r.standard_normal((1, 3, 5, 8)).astype(np.float32)
    got, mag = wgrad(g, x, k)
    want = _naive(g, x, k)
    assert got.shape == (4, 8, k, k)
    assert np.abs(got - want).max() <= 1e-13 * mag.max()      # float64 sums of the same exact products in another order
    assert (mag >= np.abs(got) - 1e-12).all()


@pytest.mark.parametrize("k", [1, 3])
def test_it_equals_float64_autograd_on_bf16_representable_operands(k):
    r = np.random.default_rng(10 + k)
    g = bf16_round(r.standard_normal((2, 4, 6, 8)).astype(np.float32))
    x = bf16_round(r.standard_normal((2, 4, 6, 12)).astype(np.float32))
    got, mag = wgrad(g, x, k)
    unrounded, _ = wgrad(g, x, k, rounded=False)
    assert np.array_equal(got, unrounded)                      # rounding is the identity on such operands
    w = torch.zeros(8, 12, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), w, padding=k // 2)
    y.backward(torch.from_numpy(g).permute(0, 3, 1, 2).double())
    assert np.abs(got - w.grad.numpy()).max() <= 1e-13 * mag.max()


def test_a_nan_of_g_poisons_its_output_channel_and_nothing_else():
    r = np.random.default_rng(3)
    g = r.standard_normal((1, 3, 5, 4)).astype(np.float32)
    x = r.standard_normal((1, 3, 5, 8)).astype(np.float32)
    g[0, 0, 0, 2] = np.nan            # a corner pixel: some of its taps fall outside the image, NaN * 0 is still NaN
    got, _ = wgrad(g, x, 3)
    assert np.isnan(got[2]).all() and np.isfinite(np.delete(got, 2, axis=0)).all()
