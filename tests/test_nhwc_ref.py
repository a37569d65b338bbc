"""tests/nhwc_ref.py (the numpy definition of the streaming channels-last layers) against torch's CPU operators in float64 --
no GPU.  The definitions that are exact in float32 are compared on data where float64 torch is exact too (integers), the others
within float64 rounding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nhwc_ref as R

SHAPES = [(1, 1, 1, 4), (2, 2, 3, 4), (1, 5, 4, 12), (3, 7, 9, 12), (2, 13, 18, 64)]


def _rng(*key):
    return np.random.default_rng(list(key))


def _ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _nchw(a):
    return torch.from_numpy(np.asarray(a, np.float64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def test_pool_extent_equals_torch_for_every_height():
    """H = 2 .. 69: torch's ceil_mode extent; H = 1, which torch refuses, is the one clipped window."""
    for h in range(2, 70):
        assert R.pool3s2_out(h) == F.max_pool2d(torch.zeros(1, 1, h, 2), 3, 2, ceil_mode=True).shape[2], h
    assert R.pool3s2_out(1) == 1
    with pytest.raises(RuntimeError):
        F.max_pool2d(torch.zeros(1, 1, 1, 4), 3, 2, ceil_mode=True)


def test_pool_extent_equals_the_library_rule():
    from srfdet3d_amd import ops
    assert all(R.pool3s2_out(h) == ops.pool3s2_out(h) for h in range(1, 200))


def test_nearest_index_equals_torch_for_every_size_pair():
    """in = 1 .. 64, out = 1 .. 129: F.interpolate(mode='nearest') picks the same source index."""
    for n_in in range(1, 65):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        for n_out in range(1, 130):
            got = F.interpolate(src, size=(n_out, 1), mode="nearest").view(-1).numpy().astype(np.int64)
            assert np.array_equal(R.nearest_index(n_out, n_in), got), (n_in, n_out)


@pytest.mark.parametrize("shape", SHAPES)
def test_affine(shape):
    rng = _rng(1, *shape)
    N, H, W, C = shape
    x, res = _ints(rng, shape), _ints(rng, shape)
    for ps in range(4):
        sc = _ints(rng, (N, C) if ps & 1 else (C,))
        sh = _ints(rng, (N, C) if ps & 2 else (C,))
        s64 = torch.from_numpy(sc.astype(np.float64)).view(N if ps & 1 else 1, 1, 1, C)
        t64 = torch.from_numpy(sh.astype(np.float64)).view(N if ps & 2 else 1, 1, 1, C)
        x64, r64 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(res.astype(np.float64))
        assert np.array_equal(R.affine(x, sc, sh, res, True, ps), torch.relu(x64 * s64 + t64 + r64).numpy())
        assert np.array_equal(R.affine(x, sc, None, None, False, ps), (x64 * s64).numpy())
        assert np.array_equal(R.affine(x, None, sh, None, False, ps), (x64 + t64).numpy())
    assert np.array_equal(R.affine(x), x)
    assert np.array_equal(R.affine(x, residual=res, relu_=True), np.maximum(x + res, 0))


def test_affine_rounds_once_per_step():
    x = np.full((1, 1, 1, 4), 1 + 2.0 ** -23, np.float32)
    sc = np.full(4, 1 + 2.0 ** -23, np.float32)
    sh = np.full(4, -1.0, np.float32)
    # the product 1 + 2^-22 + 2^-46 rounds to 1 + 2^-22 before the add; an fma would keep 2^-46
    assert np.all(R.affine(x, sc, sh) == np.float32(2.0 ** -22))


def test_fmaxf_drops_nan_and_orders_the_zeros():
    f = np.float32
    assert R.fmaxf(f(np.nan), f(1))[()] == 1 and R.fmaxf(f(-3), f(np.nan))[()] == -3 and np.isnan(R.fmaxf(f(np.nan), f(np.nan)))
    for a, b, neg in ((0.0, -0.0, False), (-0.0, 0.0, False), (-0.0, -0.0, True), (0.0, 0.0, False)):
        assert np.signbit(R.fmaxf(f(a), f(b))) == neg
    assert not np.signbit(R.relu(f(-0.0))) and R.relu(f(np.nan))[()] == 0 and R.relu(f(-np.inf))[()] == 0 and np.isinf(R.relu(f(np.inf)))


@pytest.mark.parametrize("shape", [(2, h, w, 4) for h, w in ((2, 2), (2, 5), (3, 3), (4, 7), (5, 4), (6, 6), (8, 9), (9, 8))] + [(1, 13, 18, 12)])
def test_maxpool(shape):
    x = _rng(2, *shape).standard_normal(shape).astype(np.float32)
    ref = _nhwc(F.max_pool2d(_nchw(x), 3, 2, ceil_mode=True))
    assert np.array_equal(R.maxpool3s2_ceil(x), ref)


def test_maxpool_one_row_and_nan():
    x = _rng(3).standard_normal((1, 1, 6, 4)).astype(np.float32)
    assert np.array_equal(R.maxpool3s2_ceil(x)[0, 0], np.stack([x[0, 0, 0:3].max(0), x[0, 0, 2:5].max(0), x[0, 0, 4:6].max(0)]))
    x = np.arange(36, dtype=np.float32).reshape(1, 3, 3, 4)
    x[0, 2, 2] = np.nan
    assert np.array_equal(R.maxpool3s2_ceil(x)[0, 0, 0], x[0, 2, 1])
    assert np.all(R.maxpool3s2_ceil(np.full((1, 2, 2, 4), np.nan, np.float32)) == -np.inf)      # clipped: the padding is a value
    assert np.isnan(R.maxpool3s2_ceil(np.full((1, 3, 3, 4), np.nan, np.float32))).all()         # nine NaN and nothing else


@pytest.mark.parametrize("H,W,Ht,Wt", [(4, 4, 4, 4), (8, 6, 4, 3), (13, 18, 7, 9), (29, 50, 15, 25), (5, 5, 1, 1), (3, 4, 7, 9)])
def test_upsample_add(H, W, Ht, Wt):
    rng = _rng(4, H, W, Ht, Wt)
    lat, top = _ints(rng, (2, H, W, 4)), _ints(rng, (2, Ht, Wt, 4))
    ref = _nchw(lat) + F.interpolate(_nchw(top), size=(H, W), mode="nearest")
    assert np.array_equal(R.upsample_add(lat, top), _nhwc(ref))


@pytest.mark.parametrize("shape", [(2, 1, 1, 4), (1, 2, 5, 4), (2, 6, 3, 4), (1, 9, 8, 12), (1, 29, 51, 12)])
def test_dwconv(shape):
    rng = _rng(5, *shape)
    N, H, W, C = shape
    x, w = rng.standard_normal(shape).astype(np.float32), rng.standard_normal((C, 1, 3, 3)).astype(np.float32)
    sc, sh = (rng.random(C) + 0.5).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    conv = F.conv2d(_nchw(x), torch.from_numpy(w.astype(np.float64)), stride=2, padding=1, groups=C)
    s64, t64 = torch.from_numpy(sc.astype(np.float64)).view(1, -1, 1, 1), torch.from_numpy(sh.astype(np.float64)).view(1, -1, 1, 1)
    for scale, shift, relu, ref in ((None, None, False, conv), (sc, None, True, torch.relu(conv * s64)), (None, sh, False, conv + t64),
                                    (sc, sh, True, torch.relu(conv * s64 + t64))):
        val, mag = R.dwconv3x3s2(x, w, scale, shift, relu)
        assert val.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
        assert np.abs(val - _nhwc(ref)).max() <= 1e-13 * max(mag.max(), 1.0)
        assert np.all(mag >= np.abs(val) * (1 - 1e-12))
    side = rng.standard_normal((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 8)).astype(np.float32)
    cat, cmag = R.dwconv3x3s2_cat(side, x, w, sc, sh, True)
    assert np.array_equal(cat[..., :8], side) and np.array_equal(cat[..., 8:], val) and not cmag[..., :8].any()


def test_dwconv_is_exact_on_integers():
    rng = _rng(6)
    x, w = _ints(rng, (2, 7, 6, 4)), _ints(rng, (4, 3, 3), -3, 3)
    val, _ = R.dwconv3x3s2(x, w, np.full(4, 0.5, np.float32), _ints(rng, (4,)), False)
    assert np.array_equal(val, val.astype(np.float32).astype(np.float64)) and np.array_equal(val * 2, np.round(val * 2))


@pytest.mark.parametrize("shape", SHAPES)
def test_column_sums(shape):
    rng = _rng(7, *shape)
    a, b = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    ta, tb = torch.from_numpy(a.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
    mean, bound = R.colmean(a)
    # the definition multiplies by f32(1 / HW): within 2^-24 (relative to the mean of |a|) of the true mean
    assert np.all(np.abs(mean - ta.mean(dim=(1, 2)).numpy()) <= 2.0 ** -24 * np.abs(a).astype(np.float64).mean(axis=(1, 2)) + 1e-15)
    assert np.all(bound >= 0)
    prod, bound = R.colsum_prod(a, b)
    assert np.allclose(prod, (ta * tb).sum(dim=(1, 2)).numpy(), rtol=1e-12, atol=1e-12)
    ia = _ints(rng, shape)
    assert np.array_equal(R.colsum_prod(ia, np.ones_like(ia))[0], ia.astype(np.float64).sum(axis=(1, 2)))


def test_depths_follow_the_kernel_structure():
    # colsum: C = 4 -> 256 lanes; HW = 64 * 256 + 1 -> per = 257, two pixels in the first lane
    assert R.colsum_depth(64 * 256 + 1, 4) == 2 + 255 + 64
    assert R.colsum_depth(1, 1024) == 1 + 0 + 64 and R.colsum_depth(1500, 12, prod=True) == 1 + 84 + 64 + 1
    assert R.colsum_depth(1500, 192, mean=True) == -(-24 // 5) + 4 + 64 + 1
    assert R.pool_sum_depth(6, 64) == 2 + 3 + 6 and R.pool_sum_depth(1, 4) == 1 + 3 + 6
    # affine_relu_bwd: C = 4 -> rpp = 256: one row per thread; C = 1024 -> rpp = 1: 256 rows in a thread
    assert R.arb_depth(1, 4) == 1 + 256 + 1 + 16 and R.arb_depth(17 * 256, 1024, fma=True) == 256 + 1 + 2 + 16 + 1
    assert R.arb_depth(257, 12) == -(-256 // 85) + 85 + 1 + 16
    assert R.gamma(100) == 100 * 2.0 ** -24 / (1 - 100 * 2.0 ** -24)


@pytest.mark.parametrize("n_cam,size,pad_to", [(1, None, 4), (6, (3, 5), 4), (2, (9, 11), 1), (3, (7, 4), 4), (1, (7, 9), 1)])
def test_pool_sum(n_cam, size, pad_to):
    rng = _rng(8, n_cam, pad_to)
    B, H, W, C = 2, 7, 6, 12
    x = rng.standard_normal((B * n_cam, H, W, C)).astype(np.float32)
    val, bound = R.pool_sum(x, n_cam, size, pad_to)
    Ho, Wo = (H, W) if size is None else size
    t = F.interpolate(_nchw(x), size=(Ho, Wo), mode="nearest").reshape(B, n_cam, C, Ho * Wo).sum(dim=(1, 2)).numpy()
    assert val.shape[1] % pad_to == 0 and 0 <= val.shape[1] - Ho * Wo < pad_to
    assert np.allclose(val[:, :Ho * Wo], t, rtol=1e-12, atol=1e-12) and not val[:, Ho * Wo:].any() and not bound[:, Ho * Wo:].any()


@pytest.mark.parametrize("M,C,relu,two", [(1, 4, True, False), (37, 12, True, True), (300, 40, False, True), (64, 12, True, False)])
def test_affine_relu_bwd(M, C, relu, two):
    rng = _rng(9, M, C)
    z = torch.from_numpy(_ints(rng, (M, C)).astype(np.float64)).requires_grad_(True)
    s = _ints(rng, (C,), 1, 4)
    gy, gy2 = _ints(rng, (M, C)), (_ints(rng, (M, C)) if two else None)
    y = z * torch.from_numpy(s.astype(np.float64)) + 1.0
    y = torch.relu(y) if relu else y                    # threshold_backward through autograd
    g = torch.from_numpy((gy + (gy2 if two else 0)).astype(np.float64))
    y.backward(g)
    gz, sums, bound = R.affine_relu_bwd(gy, y.detach().numpy().astype(np.float32), s, relu, gy2)
    assert gz.dtype == np.float32 and np.array_equal(gz, z.grad.numpy())
    gu = g.numpy() * ((y.detach().numpy() > 0) if relu else 1)
    assert np.array_equal(sums[0], gu.sum(0)) and np.array_equal(sums[1], (gu * y.detach().numpy()).sum(0)) and np.all(bound >= 0)
    gz1, _, _ = R.affine_relu_bwd(gy, y.detach().numpy().astype(np.float32), None, relu, gy2)
    assert np.array_equal(gz1, gu)


def test_affine_relu_bwd_masks_nan_and_zeros():
    f = np.float32
    y = np.array([[0.0, -0.0, 2.0 ** -149, np.nan], [1.0, 1.0, 1.0, 1.0]], f)
    gy = np.array([[np.nan, np.inf, 3.0, 5.0], [1.0, 1.0, 1.0, 1.0]], f)
    gz, sums, _ = R.affine_relu_bwd(gy, y, np.full(4, 2.0, f), True)
    assert np.array_equal(gz, np.array([[0, 0, 6, 0], [2, 2, 2, 2]], f))
    assert np.array_equal(sums[0], [1, 1, 4, 1]) and np.array_equal(sums[1][:3], [1, 1, 1 + 3 * 2.0 ** -149]) and np.isnan(sums[1][3])


@pytest.mark.parametrize("C", [1, 5, 64])
def test_bn_eval_fold_and_grads(C):
    rng = _rng(10, C)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.standard_normal(C).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.standard_normal(C).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(C).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy((rng.random(C) + 0.1).astype(np.float32)))
        bn.weight[0] = 0.0                                  # the s == 0 branch
    bn.eps = float(np.float32(1e-3))
    z = torch.from_numpy(rng.standard_normal((2, C, 3, 4))).requires_grad_(True)
    y = torch.relu(bn(z))
    gy = torch.from_numpy(rng.standard_normal(tuple(y.shape)))
    y.backward(gy)
    fold = R.bn_eval_fold(bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.running_mean.numpy(), bn.running_var.numpy(), 1e-3)
    assert np.allclose(z.detach().numpy() * fold[0].reshape(1, C, 1, 1) + fold[1].reshape(1, C, 1, 1), bn(z).detach().numpy(), rtol=1e-12, atol=1e-12)
    gu = (gy * (y > 0)).detach().numpy()
    sums = np.stack([gu.sum(axis=(0, 2, 3)), (gu * y.detach().numpy()).sum(axis=(0, 2, 3))])
    g = R.bn_eval_grads(sums, fold, bn.running_mean.numpy())
    ok = np.arange(C) != 0        # with gamma = 0 the library's d gamma drops the term it cannot recover from y (z is not stored)
    assert np.allclose(g[0][ok], bn.weight.grad.numpy()[ok], rtol=1e-9, atol=1e-10) and np.allclose(g[1], bn.bias.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert g[0][0] == -(bn.running_mean.numpy()[0] * sums[0][0]) * fold[2][0]
