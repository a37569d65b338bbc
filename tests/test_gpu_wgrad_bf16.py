"""srf_conv_wgrad_nhwc_bf16 (csrc/wgrad_bf16.hip) against its definition (tests/wgrad_bf16_ref.py): the weight gradient of a stride-1
convolution with both operands rounded to bf16 once, exact products, f32 accumulation, a fixed summation order.

Shapes: partial row / column tiles and a partial last chunk, the layer shapes of config 4 in small, several pixel ranges, and one shape
per edge of the kernel's 128 x 128 tile (Cout and Cin just above 128, a flattened (tap, channel) axis that straddles tiles, a map
narrower than the 32-pixel chunk).  Bounds: against float64 of the ROUNDED operands 1e-6 of sum |g| |x| per output, the f32 chain's
own over these pixel counts (tests/test_gpu_wgrad.py); against the UNROUNDED float64 the two roundings on top, (1 + 2^-8)^2 - 1 =
2^-7 + 2^-16 per product."""
import functools

import numpy as np
import pytest
import torch

from srfdet3d_amd import ops
from wgrad_bf16_ref import wgrad

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 37, 36, 20, 3), (1, 13, 33, 160, 224, 3), (3, 7, 50, 192, 192, 1), (2, 11, 32, 128, 128, 1), (1, 8, 33, 32, 64, 3),
          (1, 40, 64, 256, 256, 3),
          # the edges of the 128 x 128 tile and of the 32-pixel chunk
          (1, 6, 33, 64, 132, 3),     # Cout just above a row tile
          (2, 9, 35, 132, 64, 1),     # Cin just above a column tile
          (1, 9, 36, 96, 136, 3),     # 9 x 96 flattened columns: tiles that straddle taps, a last tile that is three quarters empty
          (2, 9, 5, 64, 32, 3),       # a map narrower than a chunk: the pixel walk wraps several rows per step
          (1, 3, 3, 8, 4, 3)]         # less than one chunk, less than one 32-channel group


@functools.lru_cache(maxsize=None)
def _case(shape):
    N, H, W, Cin, Cout, k = shape
    g_ = torch.Generator().manual_seed(N * 1000 + Cin + Cout + k)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g_) + 0.2)
    g = torch.randn(N, H, W, Cout, generator=g_) * 0.1
    ref, mag = wgrad(g.numpy(), x.numpy(), k)
    ref_u, mag_u = wgrad(g.numpy(), x.numpy(), k, rounded=False)
    return g, x, ref, mag, ref_u, mag_u


@pytest.mark.parametrize("shape", SHAPES)
def test_matches_the_definition_and_repeats(dev, shape):
    g, x, ref, mag, ref_u, mag_u = _case(shape)
    k = shape[5]
    assert ops.conv_wgrad_bf16_supported(g.to(dev), x.to(dev), k)
    got_t = ops.conv_wgrad_nhwc_bf16(g.to(dev), x.to(dev), k)
    got = got_t.cpu().double().numpy()
    assert got.shape == ref.shape
    err = (np.abs(got - ref) / np.maximum(mag, 1e-30)).max()
    err_u = (np.abs(got - ref_u) / np.maximum(mag_u, 1e-30)).max()
    print(f"{shape}: rounded-operand error {err:.3e} of sum |g||x|, unrounded {err_u:.3e}")
    assert err <= 1e-6, err
    assert err_u <= 2.0 ** -7 + 2.0 ** -16 + 1e-6, err_u
    again = ops.conv_wgrad_nhwc_bf16(g.to(dev), x.to(dev), k)
    assert torch.equal(again, got_t)                        # no atomics, a fixed order: the same bytes


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,lo_g,ld_g,lo_x,ld_x", [(2, 9, 40, 64, 96, 3, 8, 112, 4, 100), (1, 7, 37, 36, 20, 1, 4, 28, 12, 48),
                                                                  (1, 5, 33, 160, 132, 3, 0, 136, 32, 192)])
def test_channel_slices_and_exact_on_integer_data(dev, N, H, W, Cin, Cout, k, lo_g, ld_g, lo_x, ld_x):
    """Operands that are channel slices of wider channels-last buffers (pixel pitch != channels); integers in [-3, 3] are bf16 values,
    every product and partial sum is an integer below 2^24: the result is exact whatever the order.  The buffers' other channels hold
    large values: one of them read by mistake would show."""
    g_ = torch.Generator().manual_seed(ld_g + ld_x)
    gbuf = torch.full((N, H, W, ld_g), 1000.0)
    xbuf = torch.full((N, H, W, ld_x), -1000.0)
    gbuf[..., lo_g:lo_g + Cout] = torch.randint(-3, 4, (N, H, W, Cout), generator=g_).float()
    xbuf[..., lo_x:lo_x + Cin] = torch.randint(-3, 4, (N, H, W, Cin), generator=g_).float()
    gd, xd = gbuf.to(dev)[..., lo_g:lo_g + Cout], xbuf.to(dev)[..., lo_x:lo_x + Cin]
    assert ops.nhwc_ld(gd) == ld_g and ops.nhwc_ld(xd) == ld_x
    got = ops.conv_wgrad_nhwc_bf16(gd, xd, k).cpu().double()
    ref, _ = wgrad(gbuf[..., lo_g:lo_g + Cout].numpy(), xbuf[..., lo_x:lo_x + Cin].numpy(), k)
    assert torch.equal(got, torch.from_numpy(ref))


@pytest.mark.parametrize("k", [1, 3])
def test_one_nan_in_g_poisons_exactly_its_output_channel(dev, k):
    g, x = _case((2, 5, 37, 36, 20, 3))[:2]
    g = g.clone()
    g[1, 0, 0, 7] = float("nan")          # a corner pixel: for 3x3 some of its taps lie outside the image (NaN * 0 is NaN)
    got = ops.conv_wgrad_nhwc_bf16(g.to(dev), x.to(dev), k).cpu()
    bad = torch.isnan(got).flatten(1).all(1)
    assert bad.tolist() == [c == 7 for c in range(20)]
    assert torch.isfinite(got[~bad]).all()


def test_unsupported_operands_are_refused(dev):
    g, x = torch.zeros(1, 4, 4, 8, device=dev), torch.zeros(1, 4, 4, 6, device=dev)
    assert not ops.conv_wgrad_bf16_supported(g, x, 3)                     # Cin % 4
    assert not ops.conv_wgrad_bf16_supported(g, x[..., :4], 5)            # ksize
    assert not ops.conv_wgrad_bf16_supported(g, x[..., 1:5], 3)           # a base that is not 16-byte aligned
    with pytest.raises(ValueError):
        ops.conv_wgrad_nhwc_bf16(g, x, 3)
