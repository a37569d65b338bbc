"""tests/bf16_ref.py (the numpy definition the bf16-product kernels are held to) against torch: the rounding against
`torch.Tensor.bfloat16()` bit for bit, the convolution against `torch.nn.functional.conv2d` in float64.  No GPU."""
import numpy as np
import torch

import bf16_ref as R


def _same_bits(x):
    x = np.asarray(x, dtype=np.float32)
    want = torch.from_numpy(x.copy()).bfloat16().float().numpy()
    got = R.bf16_round(x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.all((got.view(np.uint32)[~nan] & 0xFFFF) == 0)      # a bf16 value: the low 16 bits are clear


def test_rounding_of_random_values_and_random_bit_patterns():
    rng = np.random.default_rng(0)
    _same_bits(rng.standard_normal(100000).astype(np.float32) * np.exp2(rng.integers(-40, 40, 100000)).astype(np.float32))
    _same_bits(rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32))   # every class of value, NaN payloads too


def test_ties_round_to_even():
    # exactly half way between two bf16 values: low half-word 0x8000; the kept bit decides
    hi = np.arange(0x3F80, 0x3FA0, dtype=np.uint32)
    ties = ((hi << 16) | 0x8000).view(np.float32)
    got = R.bf16_round(ties).view(np.uint32) >> 16
    assert np.array_equal(got, hi + (hi & 1))
    _same_bits(ties)
    _same_bits(-ties)
    _same_bits(((hi << 16) | 0x7FFF).view(np.float32))          # just below the tie: down
    _same_bits(((hi << 16) | 0x8001).view(np.float32))          # just above: up


def test_the_largest_bf16_and_its_f32_neighbours():
    top = np.array([R.BF16_MAX], dtype=np.float32)
    one_up = np.nextafter(top, np.float32(np.inf))
    tie = np.array([0x7F7F8000], dtype=np.uint32).view(np.float32)     # half way to 2^128: the even neighbour is "2^128" = inf
    vals = np.concatenate([top, one_up, np.nextafter(top, np.float32(0)), tie, np.nextafter(tie, np.float32(0)),
                           np.array([np.finfo(np.float32).max], dtype=np.float32)])
    got = R.bf16_round(vals)
    assert got[0] == R.BF16_MAX and got[1] == R.BF16_MAX and got[2] == R.BF16_MAX
    assert np.isinf(got[3]) and got[4] == R.BF16_MAX and np.isinf(got[5])
    _same_bits(vals)
    _same_bits(-vals)


def test_subnormals_are_rounded_on_the_subnormal_grid():
    rng = np.random.default_rng(1)
    sub = rng.integers(1, 1 << 23, 50000, dtype=np.uint64).astype(np.uint32).view(np.float32)     # f32 subnormals
    _same_bits(sub)
    _same_bits(-sub)
    near = (R.FLT_MIN * (1 + rng.random(1000))).astype(np.float32)
    _same_bits(near)
    got = R.bf16_round(np.array([2.0 ** -133, 2.0 ** -134, 2.0 ** -135, 3 * 2.0 ** -134], dtype=np.float32))
    assert got[0] == 2.0 ** -133 and got[1] == 0.0 and got[2] == 0.0 and got[3] == 2.0 ** -132      # smallest bf16 subnormal; ties to even


def test_infinities_and_nans():
    vals = np.array([np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0], dtype=np.float32)
    got = R.bf16_round(vals)
    assert got[0] == np.inf and got[1] == -np.inf and np.isnan(got[2]) and np.isnan(got[3])
    assert got[4] == 0 and got[5] == 0 and np.signbit(got[5]) and not np.signbit(got[4])
    _same_bits(vals)
    # a NaN whose payload sits only in the low half-word must not round to infinity
    snan = np.array([0x7F800001, 0xFF80FFFF], dtype=np.uint32).view(np.float32)
    assert np.isnan(R.bf16_round(snan)).all()
    # the definition's finiteness: inf x 0 inside a dot product is NaN
    x = np.array([[np.inf, 1.0], [1.0, 1.0]], dtype=np.float32)
    w = np.array([[0.0, 1.0], [1.0, 1.0]], dtype=np.float32)
    y, _ = R.gemm(x, w)
    assert np.isnan(y[0, 0]) and np.isinf(y[0, 1]) and np.isfinite(y[1]).all()


def test_gemm_and_conv_are_the_float64_products_of_the_rounded_operands():
    g = torch.Generator().manual_seed(3)
    for (N, H, W, Cin, Cout, k, stride, pad) in [(2, 9, 11, 8, 5, 3, 1, 1), (1, 10, 7, 4, 6, 3, 2, 1), (2, 5, 6, 8, 3, 1, 1, 0), (1, 8, 9, 4, 4, 1, 2, 0)]:
        x = torch.randn(N, H, W, Cin, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g)
        got, mag = R.conv(x.numpy(), w.numpy(), stride, pad)
        xr, wr = x.bfloat16().double(), w.bfloat16().double()
        want = torch.nn.functional.conv2d(xr.permute(0, 3, 1, 2), wr, stride=stride, padding=pad).permute(0, 2, 3, 1).numpy()
        wmag = torch.nn.functional.conv2d(xr.abs().permute(0, 3, 1, 2), wr.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1).numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        assert np.abs(mag - wmag).max() <= 1e-13 * wmag.max()
    x = torch.randn(37, 64, generator=g)
    w = torch.randn(19, 64, generator=g)
    y, mag = R.gemm(x.numpy(), w.numpy())
    assert np.array_equal(y, (x.bfloat16().double() @ w.bfloat16().double().t()).numpy()) or \
        np.abs(y - (x.bfloat16().double() @ w.bfloat16().double().t()).numpy()).max() <= 1e-13
    e = R.epilogue(y, scale=np.full(19, 2.0), shift=np.full(19, -1.0), relu=True)
    assert np.array_equal(e, np.maximum(2.0 * y - 1.0, 0.0))
