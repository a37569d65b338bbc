"""The kernels the bottleneck ResNets added -- srf_stem_conv7_nchw, srf_nhwc_maxpool3s2_pad1, the residual form of the three f32-accurate
1x1 GEMM families -- and the 1x1 / stride 2 layer through srf_conv_gemm_nhwc, against tests/resnet_ref.py and torch.

Every output is a channel slice of a wider sentinel-filled buffer whose other channels must come back untouched.  Dot products are
held to gamma(K + 2) (|scale| sum |x w| + |shift|), the bound ANY order of summation satisfies (resnet_ref.py), and are exact on
small-integer data; the pool and the residual add are compared bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as R
from srfdet3d_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1.2345e30          # no kernel result comes near it


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def sl(a, off=4, extra=12):
    """numpy (..., C) -> GPU view: the channels [off, off + C) of a buffer `extra` channels wider, the rest a sentinel."""
    a = np.asarray(a, np.float32)
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + extra,), SENT, dtype=torch.float32, device=DEV)
    v = buf[..., off:off + a.shape[-1]]
    v.copy_(torch.from_numpy(a))
    return v


def out_sl(shape, off=8, extra=20):
    buf = torch.full(tuple(shape[:-1]) + (shape[-1] + extra,), SENT, dtype=torch.float32, device=DEV)
    return buf, buf[..., off:off + shape[-1]]


def untouched(buf, C, off=8):
    return bool((buf[..., :off] == SENT).all()) and bool((buf[..., off + C:] == SENT).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ---- the 7x7 stem ----------------------------------------------------------------------------------------------------
STEM_SHAPES = [(2, 11, 13), (1, 9, 131), (1, 64, 130)]      # outputs 6 x 7: below one 4 x 64 tile, odd; 5 x 66: two tile rows (the second with one row), a partial second tile column; 32 x 65: 8 x 2 tiles, one column in the second


@pytest.mark.parametrize("N,H,W", STEM_SHAPES)
@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("affine", [False, True])
def test_stem7_within_the_bound_of_any_summation_order(cin, N, H, W, affine):
    r = _rng(cin, N, H, W, affine)
    x = r.standard_normal((N, cin, H, W)).astype(np.float32)
    w = (r.standard_normal((64, cin, 7, 7)) * 0.2).astype(np.float32)
    sc = (r.standard_normal(64) + 1.5).astype(np.float32) if affine else None
    sh = r.standard_normal(64).astype(np.float32) if affine else None
    want, bound = R.stem7(x, w, sc, sh, affine)
    buf, y = out_sl(want.shape)
    got = ops.stem_conv7_nchw(dev(x), dev(w), None if sc is None else dev(sc), None if sh is None else dev(sh), affine, out=y)
    assert got.data_ptr() == y.data_ptr() and tuple(got.shape) == want.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    assert (bound > 0).all()
    print(f"stem7 cin={cin} {N}x{H}x{W} affine={affine}: worst error / bound = {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert untouched(buf, 64)
    assert torch.equal(ops.stem_conv7_nchw(dev(x), dev(w), None if sc is None else dev(sc), None if sh is None else dev(sh), affine), got)


@pytest.mark.parametrize("N,H,W", STEM_SHAPES)
@pytest.mark.parametrize("cin", [1, 3, 4])
def test_stem7_is_exact_on_small_integers(cin, N, H, W):
    r = _rng(7, cin, N, H, W)
    x = r.integers(-8, 9, (N, cin, H, W)).astype(np.float32)
    w = r.integers(-4, 5, (64, cin, 7, 7)).astype(np.float32)
    sc, sh = r.integers(-3, 4, 64).astype(np.float32), r.integers(-50, 51, 64).astype(np.float32)
    for scale, shift, relu in ((None, None, False), (sc, sh, True), (None, sh, False), (sc, None, True)):
        want, _ = R.stem7(x, w, scale, shift, relu)
        buf, y = out_sl(want.shape)
        ops.stem_conv7_nchw(dev(x), dev(w), None if scale is None else dev(scale), None if shift is None else dev(shift), relu, out=y)
        assert np.array_equal(y.cpu().numpy().astype(np.float64), want), (scale is not None, shift is not None, relu)
        assert untouched(buf, 64)


def test_stem7_refuses_what_it_does_not_take():
    x = torch.zeros(1, 5, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="stem_conv7_nchw"):
        ops.stem_conv7_nchw(x, torch.zeros(64, 5, 7, 7, device=DEV))
    with pytest.raises(ValueError):
        ops.stem_conv7_nchw(x[:, :3], torch.zeros(64, 3, 3, 3, device=DEV))


# ---- the padded max pool ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(1, 4, 1, 1), (2, 8, 2, 3), (1, 64, 7, 9), (1, 12, 16, 24)])
def test_maxpool_pad1_equals_torch(N, C, H, W):
    r = _rng(N, C, H, W)
    x = r.standard_normal((N, H, W, C)).astype(np.float32)
    x[r.random(x.shape) < 0.15] = -np.inf                      # -inf values, whole windows of them on the small maps
    x[0, 0, 0, :] = -np.inf
    want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    assert np.array_equal(R.maxpool3s2_pad1(x), want.numpy())
    buf, y = out_sl(tuple(want.shape))
    got = ops.nhwc_maxpool3s2_pad1(sl(x), out=y)
    assert got.data_ptr() == y.data_ptr()
    assert torch.equal(y.cpu(), want) and untouched(buf, C)
    fresh = ops.nhwc_maxpool3s2_pad1(dev(x))
    assert fresh.is_contiguous() and torch.equal(fresh.cpu(), want)
    with pytest.raises(ValueError):
        ops.nhwc_maxpool3s2_pad1(dev(x), out=torch.zeros(N, H + 2, W, C, device=DEV))


# ---- the residual form of the 1x1 GEMM ----------------------------------------------------------------------------------
FAMILY_ENV = {"lds": {}, "direct": {"SRF_GEMM_DIRECT": "1"}, "split": {"SRF_GEMM_SPLIT_MIN": "1"}}


@pytest.mark.parametrize("K,Cout", [(64, 256), (32, 96), (512, 2048)])
@pytest.mark.parametrize("shape", [(1, 7, 10), (2, 10, 15)], ids=["70rows", "300rows"])      # partial row tiles of 64 and of 128
@pytest.mark.parametrize("family", ["lds", "direct", "split"])
def test_residual_gemm_is_the_plain_gemm_plus_one_add(family, shape, K, Cout, monkeypatch):
    for k in ("SRF_GEMM_DIRECT", "SRF_GEMM_SPLIT_MIN", "SRF_GEMM_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FAMILY_ENV[family].items():
        monkeypatch.setenv(k, v)
    taken = []
    choose = ops._choose_gemm
    monkeypatch.setattr(ops, "_choose_gemm", lambda *a, **kw: (lambda r: (taken.append(r[0]), r)[1])(choose(*a, **kw)))
    r = _rng(K, Cout, *shape)
    N, H, W = shape
    x = sl(r.standard_normal((N, H, W, K)))
    w = dev(r.standard_normal((Cout, K)) / np.sqrt(K))
    sc, sh = dev(r.standard_normal(Cout) + 1.5), dev(r.standard_normal(Cout))
    res = sl(r.standard_normal((N, H, W, Cout)) * 3.0 - 1.0, off=8, extra=16)       # negatives larger than the GEMM's values
    packs = dict(packed_direct=ops.pack_conv1x1_nhwc_direct_weights(w), packed_split=ops.pack_conv1x1_nhwc_split_weights(w))
    pw = ops.pack_conv1x1_nhwc_weights(w)
    z = ops.conv1x1_nhwc(x, pw, Cout, sc, sh, False, **packs)
    for relu in (True, False):
        want = torch.relu(z + res) if relu else z + res         # an f32 add is correctly rounded: bit for bit
        buf, y = out_sl((N, H, W, Cout))
        got = ops.conv1x1_nhwc_residual(x, pw, Cout, res, sc, sh, relu, out=y, **packs)
        assert got.data_ptr() == y.data_ptr()
        assert torch.equal(y, want), (family, relu, (y - want).abs().max().item())
        assert untouched(buf, Cout)
    assert not torch.equal(torch.relu(z) + res, torch.relu(z + res))      # the top-down form's order (ReLU, then add) is another function
    assert (res == SENT).sum() == 0 and torch.isfinite(z).all()
    assert set(taken) == {family}, taken
    # a fresh contiguous output, scale / shift absent
    z0 = ops.conv1x1_nhwc(x, pw, Cout, None, None, False, **packs)
    assert torch.equal(ops.conv1x1_nhwc_residual(x, pw, Cout, res, relu=True, **packs), torch.relu(z0 + res))


@pytest.mark.parametrize("shape,launch", [((1, 140, 301), "128 x 128 tiles"), ((2, 115, 250), "mixed: 128 x 128 tiles + a tail of 64 x 64")])
def test_residual_gemm_on_the_large_tiles_of_the_lds_family(shape, launch, monkeypatch):
    """With the split and the direct family switched off a large launch stays on the LDS family, where `conv1x1_launch` (csrc/conv.hip)
    takes 128 x 128 tiles from 640 tiles on: 42140 rows x 256 channels = 330 x 2 = 660 tiles, below one round of 3 x 256 workgroups, run on
    srf_conv1x1_nhwc_res_k<2, 2, 3>; 57500 rows = 450 x 2 = 900 tiles = one whole round + a partial one, the mixed launch
    (srf_conv1x1_nhwc_mixed_res_k: 384 row blocks of 128, the last 8348 rows in blocks of 64, the last of them partial)."""
    monkeypatch.setenv("SRF_GEMM_SPLIT", "0")
    monkeypatch.setenv("SRF_GEMM_DIRECT", "0")
    monkeypatch.delenv("SRF_GEMM_SPLIT_MIN", raising=False)
    N, H, W = shape
    K, Cout = 32, 256
    assert -(-N * H * W // 128) * 2 >= 640 and (N * H * W) % 128 and (N * H * W) % 64
    r = _rng(K, Cout, *shape)
    x = sl(r.standard_normal((N, H, W, K)))
    w = dev(r.standard_normal((Cout, K)) / np.sqrt(K))
    sc, sh = dev(r.standard_normal(Cout) + 1.5), dev(r.standard_normal(Cout))
    res = sl(r.standard_normal((N, H, W, Cout)) * 3.0 - 1.0, off=8, extra=16)
    pw = ops.pack_conv1x1_nhwc_weights(w)
    z = ops.conv1x1_nhwc(x, pw, Cout, sc, sh, False)
    buf, y = out_sl((N, H, W, Cout))
    ops.conv1x1_nhwc_residual(x, pw, Cout, res, sc, sh, True, out=y)
    assert torch.equal(y, torch.relu(z + res)), launch
    assert untouched(buf, Cout)


def test_residual_gemm_refuses_a_residual_of_another_shape():
    x, w = torch.zeros(1, 4, 4, 32, device=DEV), torch.zeros(64, 32, device=DEV)
    with pytest.raises(ValueError, match="res"):
        ops.conv1x1_nhwc_residual(x, ops.pack_conv1x1_nhwc_weights(w), 64, torch.zeros(1, 4, 4, 32, device=DEV))


# ---- 1x1 / stride 2 through srf_conv_gemm_nhwc (the downsample branch and a caffe-style conv1) ---------------------------
def test_strided_pointwise_conv_within_the_bound_and_exact_on_integers():
    N, H, W, Cin, Cout = 2, 9, 13, 256, 512
    r = _rng(N, H, W, Cin, Cout)
    x = r.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 1, 1)) / 16).astype(np.float32)
    sc, sh = (r.standard_normal(Cout) + 1.5).astype(np.float32), r.standard_normal(Cout).astype(np.float32)
    want, bound = R.conv_nhwc(x, w, 2, 0, sc, sh, False)
    assert want.shape == (N, 5, 7, Cout)
    assert np.allclose(want, (x[:, ::2, ::2].astype(np.float64) @ w[:, :, 0, 0].astype(np.float64).T) * sc + sh, rtol=0, atol=1e-12)
    buf, y = out_sl(want.shape)
    ops.conv_gemm_nhwc(sl(x), ops.pack_conv_gemm_weights(dev(w)), Cout, (1, 1), 2, 0, dev(sc), dev(sh), False, out=y)
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    print(f"1x1 / s2 256 -> 512: worst error / bound = {np.max(err / bound):.3f}")
    assert (err <= bound).all() and untouched(buf, Cout)
    xi = r.integers(-8, 9, (N, H, W, Cin)).astype(np.float32)
    wi = r.integers(-4, 5, (Cout, Cin, 1, 1)).astype(np.float32)
    si, bi = r.integers(-3, 4, Cout).astype(np.float32), r.integers(-50, 51, Cout).astype(np.float32)
    want, _ = R.conv_nhwc(xi, wi, 2, 0, si, bi, True)
    got = ops.conv_gemm_nhwc(sl(xi), ops.pack_conv_gemm_weights(dev(wi)), Cout, (1, 1), 2, 0, dev(si), dev(bi), True)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
