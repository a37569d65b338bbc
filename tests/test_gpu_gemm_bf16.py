"""srf_conv1x1_nhwc_bf16* / srf_conv_gemm_nhwc_bf16 (csrc/gemm_bf16.hip) against their definition, tests/bf16_ref.py:
y = epilogue(sum bf16(x) bf16(w)), operands rounded once (RNE), products exact, f32 accumulation, f32 epilogue.

* exact where the answer is exact (integers of <= 8 significant bits, few terms): rows / columns / taps / chunk bookkeeping;
* against float64 of the ROUNDED operands: <= 6e-7 of sum |a b| and <= 2 x the error of the f32-MFMA kernel on the same pre-rounded
  operands + 1e-7 (the tolerances of tests/test_gpu_gemm_split.py); against the unrounded float64 <= (2^-7 + 2^-16 + 6e-7) sum |a b|;
* the epilogues (scale / shift / ReLU, pooled, top-down), channel slices, bitwise repeatability;
* the domain lines of the file header: +-inf / NaN / values that round to infinity, operands whose rounding is subnormal."""
import numpy as np
import pytest
import torch

import bf16_ref as R
from srfdet3d_amd import ops

pytestmark = pytest.mark.gpu


def _bf(x, w, **kw):
    return ops.conv1x1_nhwc(x, None, w.shape[0], packed_bf16=ops.pack_conv1x1_nhwc_bf16_weights(w), **kw)


def _bfconv(x, w, stride, pad, **kw):
    k = w.shape[2]
    return ops.conv_gemm_nhwc(x, None, w.shape[0], (k, k), stride, pad, packed_bf16=ops.pack_conv_gemm_bf16_weights(w), **kw)


def _sparse_ints(g, shape, nz_of, bits=8):
    """integers of <= `bits` significant bits; about one in `nz_of` non-zero"""
    v = torch.randint(-(1 << bits) + 1, 1 << bits, shape, generator=g)
    return v * (torch.randint(0, nz_of, shape, generator=g) == 0)


@pytest.mark.parametrize("K", [32, 64, 96])
@pytest.mark.parametrize("Cout", [40, 200])
def test_1x1_is_exact_where_the_answer_is_exact(dev, K, Cout):
    """|v| < 2^8: bf16 holds every operand exactly; with ~6 non-zero terms per row every partial sum of any order is an integer below
    2^24, so the result is THE integer.  234 rows = a partial row block; K = 32 / 64 / 96 = half a block, one, one and a half (fewer than
    the pipeline is deep); Cout = 40 / 200 = a partial column tile / two tiles."""
    g = torch.Generator().manual_seed(K * 1000 + Cout)
    N, H, W = 2, 9, 13
    x = _sparse_ints(g, (N * H * W, K), max(1, K // 6))
    w = torch.randint(-255, 256, (Cout, K), generator=g)
    want = x @ w.t()
    assert (x.abs() @ w.abs().t()).max() < (1 << 24)
    got = _bf(x.float().view(N, H, W, K).to(dev), w.float().to(dev))
    assert torch.equal(got.cpu().double().view(-1, Cout), want.double())


@pytest.mark.parametrize("Cin,Cout,stride", [(32, 40, 1), (96, 200, 1), (32, 200, 2), (96, 40, 2)])
def test_conv_is_exact_where_the_answer_is_exact(dev, Cin, Cout, stride):
    """The same for the implicit im2col, 3x3 / padding 1 on an odd 9 x 13 map: borders, taps, the chunk inside the tap (Cin = 32: every
    block of 64 spans two taps; 96: blocks straddle a tap boundary in the middle)."""
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + stride)
    N, H, W = 2, 9, 13
    x = _sparse_ints(g, (N, H, W, Cin), max(1, 9 * Cin // 8))
    w = torch.randint(-255, 256, (Cout, Cin, 3, 3), generator=g)
    want = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    mag = torch.nn.functional.conv2d(x.double().abs().permute(0, 3, 1, 2), w.double().abs(), stride=stride, padding=1)
    assert mag.max() < (1 << 24) and want.abs().max() > 0
    got = _bfconv(x.float().to(dev), w.float().to(dev), stride, 1)
    assert got.shape == want.shape
    assert torch.equal(got.cpu().double(), want)


def _relu_like(g, shape):
    return torch.relu(torch.randn(shape, generator=g) * 1.5 + 0.2)          # post-ReLU activations: ~45 % zeros


def _check_against_float64(got, f32_on_rounded, f32_plain, ref, mag, ref_u, mag_u, tag):
    e = (np.abs(got - ref) / np.maximum(mag, 1e-30)).max()
    e_chain = (np.abs(f32_on_rounded - ref) / np.maximum(mag, 1e-30)).max()
    e_u = (np.abs(got - ref_u) / np.maximum(mag_u, 1e-30)).max()
    print(f"\n[{tag}] bf16 kernel err / sum|ab| = {e:.3g}, f32 kernel on the rounded operands = {e_chain:.3g}, against unrounded float64 = {e_u:.3g}")
    assert e <= 6e-7, (e, e_chain)
    assert e <= 2.0 * e_chain + 1e-7, (e, e_chain)
    assert e_u <= 2.0 ** -7 + 2.0 ** -16 + 6e-7, e_u
    assert not np.array_equal(got, f32_plain)            # the reduced-precision kernel really ran


@pytest.mark.parametrize("N,H,W,K,Cout", [(1, 31, 33, 96, 100), (1, 29, 50, 2144, 1024)])
def test_1x1_matches_float64_of_the_rounded_operands(dev, monkeypatch, N, H, W, K, Cout):
    monkeypatch.setenv("SRF_GEMM_SPLIT", "0")      # the yardstick is the f32-MFMA kernel
    g = torch.Generator().manual_seed(K + Cout)
    x = _relu_like(g, (N, H, W, K))
    w = torch.randn(Cout, K, generator=g) / K ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    xd, wd = x.to(dev), w.to(dev)
    got_t = _bf(xd, wd)
    got = got_t.cpu().double().numpy().reshape(-1, Cout)
    xr, wr = torch.from_numpy(R.bf16_round(x.numpy())).to(dev), torch.from_numpy(R.bf16_round(w.numpy())).to(dev)
    chain = ops.conv1x1_nhwc(xr, ops.pack_conv1x1_nhwc_weights(wr), Cout).cpu().double().numpy().reshape(-1, Cout)
    plain = ops.conv1x1_nhwc(xd, ops.pack_conv1x1_nhwc_weights(wd), Cout).cpu().double().numpy().reshape(-1, Cout)
    ref, mag = R.gemm(x.view(-1, K).numpy(), w.numpy())
    x2, w2 = x.view(-1, K).double().numpy(), w.double().numpy()
    _check_against_float64(got, chain, plain, ref, mag, x2 @ w2.T, np.abs(x2) @ np.abs(w2).T, f"1x1 {K}->{Cout}")
    # epilogue on the f32 accumulator: one fma rounding and the accumulation error scaled by |scale|
    got2 = _bf(xd, wd, scale=scale.to(dev), shift=shift.to(dev), relu=True).cpu().double().numpy().reshape(-1, Cout)
    want2 = R.epilogue(ref, scale.numpy(), shift.numpy(), True)
    tol = 6e-7 * mag * np.abs(scale.double().numpy()) + 2.0 ** -22 * np.maximum(np.abs(want2), np.abs(shift.double().numpy()))
    assert (np.abs(got2 - want2) <= tol).all()
    assert (got2 >= 0).all() and (got2 == 0).any()
    # two launches, the same bits
    assert torch.equal(_bf(xd, wd), got_t)


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride", [(2, 17, 19, 64, 72, 1), (1, 21, 23, 96, 136, 2)])
def test_conv_matches_float64_of_the_rounded_operands(dev, monkeypatch, N, H, W, Cin, Cout, stride):
    monkeypatch.setenv("SRF_GEMM_SPLIT", "0")
    g = torch.Generator().manual_seed(Cin + Cout + stride)
    x = _relu_like(g, (N, H, W, Cin))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    xd, wd = x.to(dev), w.to(dev)
    got_t = _bfconv(xd, wd, stride, 1)
    got = got_t.cpu().double().numpy()
    xr, wr = torch.from_numpy(R.bf16_round(x.numpy())).to(dev), torch.from_numpy(R.bf16_round(w.numpy())).to(dev)
    chain = ops.conv_gemm_nhwc(xr, ops.pack_conv_gemm_weights(wr), Cout, (3, 3), stride, 1).cpu().double().numpy()
    plain = ops.conv_gemm_nhwc(xd, ops.pack_conv_gemm_weights(wd), Cout, (3, 3), stride, 1).cpu().double().numpy()
    ref, mag = R.conv(x.numpy(), w.numpy(), stride, 1)
    ref_u = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=stride, padding=1).permute(0, 2, 3, 1).numpy()
    mag_u = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double().abs(), stride=stride, padding=1).permute(0, 2, 3, 1).numpy()
    assert got.shape == ref.shape
    _check_against_float64(got, chain, plain, ref, mag, ref_u, mag_u, f"conv {Cin}->{Cout}/s{stride}")
    got2 = _bfconv(xd, wd, stride, 1, scale=scale.to(dev), shift=shift.to(dev), relu=True).cpu().double().numpy()
    want2 = R.epilogue(ref, scale.numpy(), shift.numpy(), True)
    tol = 6e-7 * mag * np.abs(scale.double().numpy()) + 2.0 ** -22 * np.maximum(np.abs(want2), np.abs(shift.double().numpy()))
    assert (np.abs(got2 - want2) <= tol).all()
    assert torch.equal(_bfconv(xd, wd, stride, 1), got_t)


@pytest.mark.parametrize("N,H,W,K,Cout", [(3, 23, 27, 160, 96), (2, 58, 100, 1728, 768)])
def test_pooled_stores_the_plain_outputs_and_their_mean(dev, N, H, W, K, Cout):
    g = torch.Generator().manual_seed(11)
    x = torch.relu(torch.randn(N, H, W, K, generator=g)).to(dev)
    w = (torch.randn(Cout, K, generator=g) / K ** 0.5).to(dev)
    scale, shift = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.1).to(dev)
    y0 = _bf(x, w, scale=scale, shift=shift, relu=True)
    y, mean = _bf(x, w, scale=scale, shift=shift, relu=True, pool=True)
    assert torch.equal(y, y0)                                               # the pooled form stores the same outputs
    want = y.double().mean(dim=(1, 2))
    assert (mean.double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    y2, mean2 = _bf(x, w, scale=scale, shift=shift, relu=True, pool=True)
    assert torch.equal(mean2, mean) and torch.equal(y2, y)                  # fixed summation order


@pytest.mark.parametrize("N,H,W,Ht,Wt,K,Cout", [(2, 20, 30, 10, 15, 64, 128), (1, 29, 50, 15, 25, 768, 256), (2, 13, 21, 7, 11, 96, 40)])
def test_topdown_equals_conv_then_upsample_add(dev, N, H, W, Ht, Wt, K, Cout):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, K, generator=g).to(dev)
    w = (torch.randn(Cout, K, generator=g) / K ** 0.5).to(dev)
    shift = (torch.randn(Cout, generator=g) * 0.1).to(dev)
    top = torch.randn(N, Ht, Wt, Cout, generator=g).to(dev)
    plain = _bf(x, w, shift=shift)
    up = torch.nn.functional.interpolate(top.permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(_bf(x, w, shift=shift, top=top), plain + up)         # the same float is added once


def test_reads_and_writes_channel_slices(dev):
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(2, 17, 19, 160, generator=g)
    w = torch.randn(24, 64, generator=g) / 8
    dst = torch.full((2, 17, 19, 72), 7.0, device=dev)
    _bf(buf.to(dev)[..., 32:96], w.to(dev), out=dst[..., 8:32])
    ref, mag = R.gemm(buf[..., 32:96].reshape(-1, 64).numpy(), w.numpy())
    assert (np.abs(dst[..., 8:32].cpu().double().numpy().reshape(-1, 24) - ref) <= 6e-7 * mag).all()
    assert torch.all(dst[..., :8] == 7.0) and torch.all(dst[..., 32:] == 7.0)
    # the conv form: x_ld = 160 > Cin = 32 (K = 288: a half block at the end), y_ld = 72 > Cout = 24
    w3 = torch.randn(24, 32, 3, 3, generator=g) / 17
    dst.fill_(7.0)
    _bfconv(buf.to(dev)[..., 96:128], w3.to(dev), 1, 1, out=dst[..., 40:64])
    ref, mag = R.conv(buf[..., 96:128].contiguous().numpy(), w3.numpy(), 1, 1)
    assert (np.abs(dst[..., 40:64].cpu().double().numpy() - ref) <= 6e-7 * mag).all()
    assert torch.all(dst[..., :40] == 7.0) and torch.all(dst[..., 64:] == 7.0)


def _run(x, w, dev):
    rows, K = x.shape
    got = _bf(x.view(1, 1, rows, K).to(dev), w.to(dev)).cpu().double().numpy().reshape(rows, -1)
    ref, mag = R.gemm(x.numpy(), w.numpy())
    return got, ref, mag


def test_non_finite_operands_give_ieee_arithmetic_on_the_rounded_operands(dev):
    """+-inf, NaN, and finite values above the largest bf16 (they round to +-inf) in activations and weights: NaN exactly where the
    definition has NaN (inf x 0, inf - inf, NaN), +-inf of the same sign exactly where it has +-inf, every other output in tolerance."""
    g = torch.Generator().manual_seed(65)
    rows, K, Cout = 140, 96, 160
    x = torch.randn(rows, K, generator=g)
    w = torch.randn(Cout, K, generator=g) * 2.0 ** -12
    w[10:20, 7] = 0.0                                                      # inf x 0 = NaN
    x[5, 7], x[64, 33], x[139, 95] = float("inf"), float("-inf"), float("nan")
    x[20, 3], x[21, 40] = 3.40e38, -float.fromhex("0x1.FFp127")            # finite in f32, infinite after the rounding
    x[22, 64] = R.BF16_MAX                                                 # the largest bf16 itself stays finite
    x[30, 1], x[30, 2] = float("inf"), float("-inf")                       # inf - inf inside a row, whatever the order
    w[:, 1], w[:, 2] = w[:, 1].abs() + 2.0 ** -20, w[:, 2].abs() + 2.0 ** -20
    w[100, 50], w[101, 51], w[102, 52] = float("inf"), 3.40e38, float("nan")
    got, ref, mag = _run(x, w, dev)
    assert np.isnan(ref[5, 12]) and np.isinf(ref[5, 0]) and np.isinf(ref[20, 0]) and np.isfinite(ref[22, 0]) and np.isnan(ref[30, 0])
    assert np.isinf(ref[0, 100]) and np.isinf(ref[0, 101]) and np.isnan(ref[0, 102])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref))
    fin = np.isfinite(ref)
    assert fin.sum() > rows * Cout // 2
    assert (np.abs(got[fin] - ref[fin]) <= 6e-7 * mag[fin]).all()


@pytest.mark.parametrize("tiny_side", ["activations", "weights"])
def test_operands_whose_rounding_is_subnormal(dev, tiny_side):
    """|x| < 2^-126 after the rounding (f32 subnormals, and normals just under 2^-126 that do not round up to it): the conversion keeps
    them, the MFMA may flush its A / B inputs.  Held to the derivable bound only: within sum over those terms of 2^-126 |partner| of
    the definition (plus the accumulation error of the rest)."""
    g = torch.Generator().manual_seed(62)
    rows, K, Cout = 200, 128, 128
    kind = torch.randint(0, 3, (rows, K), generator=g)
    sub = torch.randint(1, 1 << 23, (rows, K), generator=g).int().view(torch.float32)            # f32 subnormals k 2^-149
    small = torch.exp2(torch.randint(-133, -126, (rows, K), generator=g).float())                # bf16 subnormals, exactly representable
    tiny = torch.where(kind == 0, sub, torch.where(kind == 1, small, torch.randn(rows, K, generator=g)))
    tiny = tiny * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1)
    other = torch.randn(rows, K, generator=g)
    x, w = (tiny, other[:Cout].contiguous()) if tiny_side == "activations" else (other, tiny[:Cout].contiguous())
    got, ref, mag = _run(x, w, dev)
    xr, wr = R.bf16_round(x.numpy()).astype(np.float64), R.bf16_round(w.numpy()).astype(np.float64)
    if tiny_side == "activations":
        partner = ((np.abs(xr) < R.FLT_MIN) & (xr != 0)).astype(np.float64) @ np.abs(wr).T
    else:
        partner = np.abs(xr) @ ((np.abs(wr) < R.FLT_MIN) & (wr != 0)).astype(np.float64).T
    assert partner.min() > 0
    tol = 6e-7 * mag + R.FLT_MIN * partner
    err = np.abs(got - ref)
    print(f"\n[{tiny_side}] max err / (2^-126 sum |partner|) = {(err / (R.FLT_MIN * partner)).max():.3g}; "
          f"max err / (6e-7 sum |a b|) = {(err / (6e-7 * mag)).max():.3g}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), (err / tol).max()
    # on record (printed with -s): a product whose tiny side holds ONLY bf16 subnormals against partners of 2^100 .. 2^110 lands in the
    # normal range if the MFMA keeps its subnormal inputs and is zero if it flushes them; both satisfy the bound
    tiny2 = torch.exp2(torch.randint(-133, -126, (rows, K), generator=g).float())
    big = torch.exp2(torch.randint(100, 111, (rows, K), generator=g).float())
    x, w = (tiny2, big[:Cout].contiguous()) if tiny_side == "activations" else (big, tiny2[:Cout].contiguous())
    got, ref, mag = _run(x, w, dev)
    partner = np.abs(w.double().numpy()).sum(1)[None, :] if tiny_side == "activations" else np.abs(x.double().numpy()).sum(1)[:, None]
    print(f"[{tiny_side}] only-subnormal operands: result / definition = {(got / ref).min():.3g} .. {(got / ref).max():.3g} "
          f"(1 = kept, 0 = flushed)")
    assert (np.abs(got - ref) <= 6e-7 * mag + R.FLT_MIN * partner).all()
