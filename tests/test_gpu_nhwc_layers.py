"""The streaming channels-last layers (csrc/nhwc.hip) against their definition, tests/nhwc_ref.py.

Rules common to every kernel: every input is a channel slice of a wider buffer at a non-zero offset (ld != C, the other channels
hold a sentinel), every output is a slice of a wider sentinel-filled buffer whose other channels must come back untouched, and
every call is made twice and must repeat bit for bit.  Element-wise results are compared bit for bit (NaN against NaN), sums
exactly on integer data and within the derived bound gamma_d * sum |terms| on random data; the worst error / bound ratio of each
reduction is printed (DESIGN.md section 2 records them).

(A (N, 1, 1, C) view with N > 1 cannot say its row stride, ops.nhwc_ld: cases whose input or output map is 1 x 1 run with N = 1.)"""
import numpy as np
import pytest
import torch

import nhwc_ref as R
from srfdet3d_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1.2345e30          # no kernel result comes near it
OFF, EXTRA = 4, 12        # inputs: channels [4, 4 + C) of a buffer C + 12 wide; outputs: [8, 8 + C) of one C + 20 wide
OOFF, OEXTRA = 8, 20


def rng_for(*key):
    return np.random.default_rng([int(k) for k in key])


def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def normal(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def sl(a, off=OFF, extra=EXTRA):
    """numpy (..., C) -> GPU view: the channels [off, off + C) of a buffer `extra` channels wider, the rest a sentinel."""
    a = np.asarray(a, np.float32)
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + extra,), SENT, dtype=torch.float32, device=DEV)
    v = buf[..., off:off + a.shape[-1]]
    v.copy_(torch.from_numpy(a))
    return v


def out_sl(shape, off=OOFF, extra=OEXTRA):
    buf = torch.full(tuple(shape[:-1]) + (shape[-1] + extra,), SENT, dtype=torch.float32, device=DEV)
    return buf, buf[..., off:off + shape[-1]]


def untouched(buf, C, off=OOFF):
    s = torch.full((), SENT, dtype=torch.float32, device=DEV)
    return torch.equal(buf[..., :off], s.expand_as(buf[..., :off])) and torch.equal(buf[..., off + C:], s.expand_as(buf[..., off + C:]))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_bits(got, want, what=""):
    """float32 equality to the bit, +0 != -0; a NaN must meet a NaN (payloads are free)."""
    g = got.detach().cpu().contiguous().numpy()
    w = np.ascontiguousarray(want, dtype=np.float32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gn, wn = np.isnan(g), np.isnan(w)
    ok = (gn & wn) | (~gn & ~wn & (g.view(np.uint32) == w.view(np.uint32)))
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {i}: got {g[i]!r}, want {w[i]!r}")


def worst_ratio(got, val, bound, what):
    """max |got - val| / bound (0 / 0 counts as 0: an exact zero with nothing summed)."""
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - val)
    assert np.all(err <= bound), (what, float((err - bound).max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def batch_for(H, W, N):
    return 1 if H * W == 1 else N


# ---- affine -------------------------------------------------------------------------------------------------------------------
AFFINE_SHAPES = [(1, 1, 1, 4), (1, 15, 17, 4), (1, 16, 16, 4), (1, 1, 257, 4), (3, 5, 7, 12), (3, 3, 4, 64), (1, 8, 8, 12)]


def _affine_case(x, scale, shift, res, relu, ps, inplace=False):
    N, H, W, C = x.shape
    want = R.affine(x, scale, shift, res, relu, ps)
    outs = []
    for _ in range(2):
        xs = sl(x)
        args = (xs, None if scale is None else torch.from_numpy(scale).to(DEV), None if shift is None else torch.from_numpy(shift).to(DEV), relu)
        rs = None if res is None else sl(res, 8, 16)
        if inplace:
            y = ops.nhwc_affine(*args, residual=rs, out=xs)
            assert y.data_ptr() == xs.data_ptr() and untouched(xs._base, C, OFF)
        else:
            buf, o = out_sl(x.shape)
            y = ops.nhwc_affine(*args, residual=rs, out=o)
            assert y.data_ptr() == o.data_ptr() and untouched(buf, C)
            assert same_bits(xs, torch.from_numpy(x).to(DEV))                   # the input is left alone
        outs.append(y.clone())
    assert same_bits(outs[0], outs[1])
    assert_bits(outs[0], want, f"affine {x.shape} ps={ps} scale={scale is not None} shift={shift is not None} res={res is not None} relu={relu}")


@pytest.mark.parametrize("shape", AFFINE_SHAPES)
def test_affine_equals_the_definition(shape):
    """Quads below, at and above one workgroup (255, 256, 257 at C = 4), every per_sample value, every operand present and absent."""
    N, H, W, C = shape
    rng = rng_for(1, *shape)
    x, res = normal(rng, shape), normal(rng, shape)
    k = 0
    for ps in range(4):
        for has_scale, has_shift, has_res in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
            if (ps & 1 and not has_scale) or (ps & 2 and not has_shift):
                continue
            scale = normal(rng, (N, C) if ps & 1 else (C,)) if has_scale else None
            shift = normal(rng, (N, C) if ps & 2 else (C,)) if has_shift else None
            _affine_case(x, scale, shift, res if has_res else None, bool(k & 1), ps, inplace=(k % 3 == 2))
            k += 1


def test_affine_per_sample_shift_selects_its_own_row():
    """Scale per channel, shift per image and the reverse: reading bit 1 as bit 0 (or the reverse) takes the wrong row."""
    rng = rng_for(2)
    x = normal(rng, (3, 2, 3, 12))
    _affine_case(x, normal(rng, (12,)), ints(rng, (3, 12), 10, 90), None, False, 2)
    _affine_case(x, ints(rng, (3, 12), 10, 90), normal(rng, (12,)), None, False, 1)


def test_affine_non_finite_values():
    """relu(NaN) = 0, relu(-inf) = 0, relu(-0) = +0; without the ReLU, NaN and +-inf pass as IEEE arithmetic has them."""
    rng = rng_for(3)
    x = normal(rng, (1, 4, 4, 12))
    x[0, 0, 0, :6] = [np.nan, np.inf, -np.inf, -0.0, 0.0, np.nan]
    x[0, 1, 2, 3] = np.inf
    sc = np.ones(12, np.float32)
    sc[1], sc[4] = 0.0, -1.0                                                   # inf * 0 = NaN; 0 * -1 = -0
    res = np.zeros(x.shape, np.float32)
    res[0, 1, 2, 3] = -np.inf                                                  # inf + -inf = NaN
    for relu in (False, True):
        _affine_case(x, sc, None, res, relu, 0)
        _affine_case(x, None, None, None, relu, 0)
    want = R.affine(x, sc, None, res, True)
    assert want[0, 0, 0, 0] == 0 and want[0, 0, 0, 1] == 0 and want[0, 1, 2, 3] == 0 and not np.isnan(want).any()


def test_affine_ignores_r_ld_without_a_residual():
    """C ABI: residual = NULL with r_ld = 0, 2 and -6 (the last two were refused as 'not a multiple of 4')."""
    rng = rng_for(4)
    x = normal(rng, (2, 3, 3, 8))
    sc = torch.from_numpy(normal(rng, (8,))).to(DEV)
    L = _lib.lib()
    for r_ld in (0, 2, -6):
        xs = sl(x)
        buf, o = out_sl(x.shape)
        rc = L.srf_nhwc_affine(ops._ptr(xs), ops.nhwc_ld(xs), 2, 9, 8, ops._ptr(sc), 0, None, None, r_ld, 0, ops._ptr(o), ops.nhwc_ld(o), ops._stream())
        assert rc == 0, r_ld
        assert_bits(o, R.affine(x, sc.cpu().numpy()))
        assert untouched(buf, 8)


# ---- max pool ------------------------------------------------------------------------------------------------------------------
def _maxpool_case(x):
    N, H, W, C = x.shape
    want = R.maxpool3s2_ceil(x)
    outs = []
    for _ in range(2):
        buf, o = out_sl(want.shape)
        y = ops.nhwc_maxpool3s2_ceil(sl(x), out=o)
        assert untouched(buf, C)
        outs.append(y.clone())
    assert same_bits(outs[0], outs[1])
    assert_bits(outs[0], want, f"maxpool {x.shape}")


@pytest.mark.parametrize("H", range(1, 10))
def test_maxpool_every_small_map(H):
    """H, W = 1 .. 9: odd and even Ho / Wo, Ho = 1, 2 x 2 output blocks whose second row / column is clipped, windows clipped
    at the bottom / right edge.  The values are distinct, so a window off by one pixel gives another maximum."""
    for W in range(1, 10):
        N = 1 if R.pool3s2_out(H) * R.pool3s2_out(W) == 1 else 2
        x = rng_for(5, H, W).permutation(N * H * W * 4).astype(np.float32).reshape(N, H, W, 4) - 100.0
        _maxpool_case(x)
        assert ops.nhwc_maxpool3s2_ceil(sl(x)).shape == (N, R.pool3s2_out(H), R.pool3s2_out(W), 4)


@pytest.mark.parametrize("N,H,W,C", [(1, 13, 18, 12), (3, 29, 50, 12), (3, 13, 18, 64)])
def test_maxpool_model_maps(N, H, W, C):
    _maxpool_case(normal(rng_for(6, N, H, W, C), (N, H, W, C)))


def test_maxpool_non_finite_values():
    """Rows of -inf give -inf; a NaN in a window is dropped (fmaxf); a whole window of NaN gives NaN, a clipped one -inf (the taps
    past the edge are -inf values); +0 beats -0."""
    rng = rng_for(7)
    x = normal(rng, (2, 9, 8, 4))
    x[0, 0:3] = -np.inf
    x[0, 4, 3] = np.nan
    x[1, :, :, 1] = np.nan
    x[1, 2:7, 2:7, 2] = -0.0
    x[1, 3, 3, 2] = 0.0                                                        # in the window of output (1, 1) alone
    x[1, 6, 6, 3] = np.inf
    want = R.maxpool3s2_ceil(x)
    assert np.all(want[0, 0] == -np.inf) and np.isnan(want[1, :, :3, 1]).all() and np.all(want[1, :, 3, 1] == -np.inf)
    assert not np.isnan(want[0]).any() and not np.isnan(want[1][..., [0, 2, 3]]).any()
    assert not np.signbit(want[1, 1, 1, 2]) and np.signbit(want[1, 2, 2, 2]) and np.signbit(want[1, 1, 2, 2]) and want[1, 1, 2, 2] == 0
    _maxpool_case(x)


# ---- upsample + add ------------------------------------------------------------------------------------------------------------
UPSAMPLE = [(8, 8, 8, 8), (8, 6, 4, 3), (13, 18, 7, 9), (29, 50, 15, 25), (50, 29, 25, 15), (13, 50, 7, 25), (5, 7, 1, 1), (6, 5, 1, 3),
            (3, 4, 7, 9), (9, 4, 4, 9), (1, 1, 3, 2),
            (4, 22, 2, 26), (46, 3, 14, 2)]      # 22 <- 26 and 46 <- 14: floor(dst * f32(in / out)) is one below dst * in // out at dst = 11 / 23


@pytest.mark.parametrize("H,W,Ht,Wt", UPSAMPLE)
def test_upsample_add_equals_the_definition(H, W, Ht, Wt):
    for N, C in ((1, 4), (3, 12), (3, 64)):
        if H * W == 1 or Ht * Wt == 1:
            N = 1
        rng = rng_for(8, H, W, Ht, Wt, C)
        lat, top = normal(rng, (N, H, W, C)), normal(rng, (N, Ht, Wt, C))
        want = R.upsample_add(lat, top)
        outs = []
        for _ in range(2):
            buf, o = out_sl(lat.shape)
            ls, ts = sl(lat), sl(top, 8, 16)
            y = ops.nhwc_upsample_add(ls, ts, out=o)
            assert y.data_ptr() == o.data_ptr() and untouched(buf, C) and same_bits(ls, torch.from_numpy(lat).to(DEV))
            z = ops.nhwc_upsample_add(ls, ts)                                   # out=None: lat in place
            assert z.data_ptr() == ls.data_ptr() and untouched(ls._base, C, OFF) and same_bits(z, y)
            outs.append(y.clone())
        assert same_bits(outs[0], outs[1])
        assert_bits(outs[0], want, f"upsample_add {(N, H, W, C)} <- {(Ht, Wt)}")


def test_upsample_add_index_rule_on_a_coded_map():
    """top holds its own (y, x) index: every output pixel names its source, for each of the size pairs above."""
    for H, W, Ht, Wt in UPSAMPLE:
        if Ht * Wt == 1 or H * W == 1:
            continue
        top = np.zeros((1, Ht, Wt, 4), np.float32)
        top[0, :, :, 0] = np.arange(Ht)[:, None] * 64 + np.arange(Wt)[None, :]
        y = ops.nhwc_upsample_add(sl(np.zeros((1, H, W, 4), np.float32)), sl(top))
        want = R.nearest_index(H, Ht)[:, None] * 64 + R.nearest_index(W, Wt)[None, :]
        assert np.array_equal(y[0, :, :, 0].cpu().numpy(), want.astype(np.float32)), (H, W, Ht, Wt)


def test_upsample_add_non_finite_values():
    rng = rng_for(9)
    lat, top = normal(rng, (1, 6, 6, 4)), normal(rng, (1, 3, 3, 4))
    lat[0, 0, 0] = [np.inf, -np.inf, np.nan, -0.0]
    top[0, 0, 0] = [-np.inf, -np.inf, 1.0, -0.0]
    y = ops.nhwc_upsample_add(sl(lat), sl(top))
    assert_bits(y, R.upsample_add(lat, top))


# ---- depthwise 3x3 / stride 2 ---------------------------------------------------------------------------------------------------
def _pow2(rng, C):
    return (2.0 ** rng.integers(-2, 3, size=C)).astype(np.float32) * np.where(rng.random(C) < 0.3, -1, 1).astype(np.float32)


def _dwconv_run(x, w, scale, shift, relu):
    """-> the kernel's output (checked for repeatability, neighbours, and equality with the NCHW twin)."""
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tw = torch.from_numpy(w).to(DEV)
    ts = None if scale is None else torch.from_numpy(scale).to(DEV)
    tt = None if shift is None else torch.from_numpy(shift).to(DEV)
    outs = []
    for _ in range(2):
        buf, o = out_sl((N, Ho, Wo, C))
        y = ops.nhwc_dwconv3x3s2(sl(x), tw, ts, tt, relu, out=o)
        assert y.data_ptr() == o.data_ptr() and untouched(buf, C)
        outs.append(y.clone())
    assert same_bits(outs[0], outs[1])
    twin = ops.dwconv3x3s2(torch.from_numpy(x).to(DEV).permute(0, 3, 1, 2).contiguous(), tw, ts, tt, relu)
    assert same_bits(outs[0], twin.permute(0, 2, 3, 1)), "the NCHW twin adds its taps in the same order"
    return outs[0]


def _dwconv_exact_and_bounded(N, H, W, C, key):
    """Integer data (every step exact): bit-equal; random data: within gamma_11 of float64.  Returns the worst error / bound."""
    rng = rng_for(10, key, N, H, W, C)
    worst = 0.0
    for k, (has_scale, has_shift) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        relu = bool((k + key) & 1)
        x, w = ints(rng, (N, H, W, C)), ints(rng, (C, 1, 3, 3), -5, 5)
        x[rng.random(x.shape) < 0.1] = -0.0
        scale, shift = (_pow2(rng, C) if has_scale else None), (ints(rng, (C,)) if has_shift else None)
        val, _ = R.dwconv3x3s2(x, w, scale, shift, relu)
        assert_bits(_dwconv_run(x, w, scale, shift, relu), val.astype(np.float32), f"dwconv ints {(N, H, W, C)} scale={has_scale} shift={has_shift}")
        x, w = normal(rng, (N, H, W, C)), normal(rng, (C, 1, 3, 3))
        scale, shift = (normal(rng, (C,)) if has_scale else None), (normal(rng, (C,)) if has_shift else None)
        val, mag = R.dwconv3x3s2(x, w, scale, shift, not relu)
        worst = max(worst, worst_ratio(_dwconv_run(x, w, scale, shift, not relu), val, R.dwconv_bound(mag), f"dwconv {(N, H, W, C)}"))
    return worst


@pytest.mark.parametrize("H", range(1, 10))
def test_dwconv_every_small_map(H):
    """H, W = 1 .. 9 at C = 4: the halo row / column of zeros on every side, odd and even Ho / Wo, clipped second rows / columns
    of the 2 x 2 output blocks.  Distinct tap weights: a transposed tap order or a dropped halo changes the integer result."""
    worst = max(_dwconv_exact_and_bounded(1 if H <= 2 and W <= 2 else 2, H, W, 4, H) for W in range(1, 10))
    print(f"\nRATIO dwconv H={H}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("N,H,W,C", [(3, 29, 51, 12), (1, 13, 18, 64)])
def test_dwconv_model_maps(N, H, W, C):
    print(f"\nRATIO dwconv {(N, H, W, C)}: worst error / bound {_dwconv_exact_and_bounded(N, H, W, C, 0):.3f}")


def test_dwconv_taps_are_read_in_ky_kx_order():
    """One non-zero tap at a time on a coded map: output (yo, xo) must be x[2 yo + ky - 1][2 xo + kx - 1] (0 outside)."""
    H, W = 7, 6
    x = np.zeros((1, H, W, 4), np.float32)
    x[0, :, :, :] = (np.arange(H)[:, None] * 16 + np.arange(W)[None, :] + 1)[:, :, None]
    for ky in range(3):
        for kx in range(3):
            w = np.zeros((4, 1, 3, 3), np.float32)
            w[:, 0, ky, kx] = 1.0
            y = ops.nhwc_dwconv3x3s2(sl(x), torch.from_numpy(w).to(DEV)).cpu().numpy()
            for yo in range(4):
                for xo in range(3):
                    yi, xi = 2 * yo + ky - 1, 2 * xo + kx - 1
                    assert y[0, yo, xo, 0] == (x[0, yi, xi, 0] if 0 <= yi < H and 0 <= xi < W else 0.0), (ky, kx, yo, xo)


def test_dwconv_non_finite_values():
    """relu(NaN) = 0; without the ReLU a NaN / inf input reaches exactly the outputs whose window holds it."""
    rng = rng_for(11)
    x, w = ints(rng, (1, 8, 8, 4)), ints(rng, (4, 1, 3, 3), 1, 4)
    x[0, 3, 3, 0], x[0, 4, 4, 1], x[0, 0, 0, 2] = np.nan, np.inf, -np.inf
    for relu in (False, True):
        val, _ = R.dwconv3x3s2(x, w, None, None, relu)
        assert_bits(_dwconv_run(x, w, None, None, relu), val.astype(np.float32), f"dwconv non-finite relu={relu}")
    assert np.isnan(R.dwconv3x3s2(x, w)[0][0, 1:3, 1:3, 0]).all() and not np.isnan(R.dwconv3x3s2(x, w, relu_=True)[0]).any()


@pytest.mark.parametrize("N,H,W,C,Cs", [(1, 1, 1, 4, 4), (2, 5, 8, 4, 64), (3, 29, 51, 12, 4), (2, 9, 9, 12, 64), (3, 40, 40, 64, 64)])
def test_dwconv_cat_is_the_copy_plus_the_plain_call(N, H, W, C, Cs):
    """`side` itself a slice; (3, 40, 40, 64, 64) has 19 workgroups of convolution threads followed by 75 of copy threads, the
    boundary between them inside a workgroup."""
    rng = rng_for(12, N, H, W, C, Cs)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w, side = normal(rng, (N, H, W, C)), normal(rng, (C, 1, 3, 3)), normal(rng, (N, Ho, Wo, Cs))
    sc, sh = normal(rng, (C,)), normal(rng, (C,))
    tw, ts, tt = (torch.from_numpy(a).to(DEV) for a in (w, sc, sh))
    plain = ops.nhwc_dwconv3x3s2(sl(x), tw, ts, tt, True)
    outs = []
    for _ in range(2):
        buf, o = out_sl((N, Ho, Wo, Cs + C))
        y = ops.nhwc_dwconv3x3s2_cat(sl(x), tw, ts, tt, True, sl(side, 8, 16), o)
        assert y.data_ptr() == o.data_ptr() and untouched(buf, Cs + C)
        outs.append(y.clone())
    assert same_bits(outs[0], outs[1])
    assert same_bits(outs[0][..., :Cs], torch.from_numpy(side).to(DEV)) and same_bits(outs[0][..., Cs:], plain)
    val, mag = R.dwconv3x3s2_cat(side, x, w, sc, sh, True)
    worst_ratio(outs[0], val, R.dwconv_bound(mag), "dwconv_cat")


# ---- column mean / column sum of a product ---------------------------------------------------------------------------------------
def _hw_list(C):
    lanes = 256 // (C // 4)
    return [1, 63, 64, 65, 64 * lanes + 1, 1500 + C // 4]


@pytest.mark.parametrize("C", [4, 12, 192, 768, 1024])
def test_column_sums(C):
    """lanes = 256, 85, 5, 1, 1 pixel lanes (idle threads at C = 12, 192, 768); HW below / at / above the 64 chunks (empty chunks),
    one pixel past a full round of the lanes, and ~1500.  a and b with different ld."""
    worst = {"colmean": 0.0, "colsum_prod": 0.0}
    for HW in _hw_list(C):
        N = 1 if HW == 1 else 3
        shape = (N, 1, HW, C)
        rng = rng_for(13, C, HW)
        # integers: every partial sum is exact in float32, whatever the order
        a, b = ints(rng, shape), ints(rng, shape)
        S = a.astype(np.float64).sum(axis=(1, 2))
        assert_bits(ops.nhwc_colmean(sl(a)), S.astype(np.float32) * (np.float32(1.0) / np.float32(HW)), f"colmean ints C={C} HW={HW}")
        assert_bits(ops.nhwc_colsum_prod(sl(a), sl(b, 8, 16)), (a.astype(np.float64) * b).sum(axis=(1, 2)).astype(np.float32),
                    f"colsum_prod ints C={C} HW={HW}")
        a, b = normal(rng, shape) + np.float32(0.5), normal(rng, shape)
        m = [ops.nhwc_colmean(sl(a)) for _ in range(2)]
        p = [ops.nhwc_colsum_prod(sl(a), sl(b, 8, 16)) for _ in range(2)]
        assert same_bits(m[0], m[1]) and same_bits(p[0], p[1])
        worst["colmean"] = max(worst["colmean"], worst_ratio(m[0], *R.colmean(a), f"colmean C={C} HW={HW}"))
        worst["colsum_prod"] = max(worst["colsum_prod"], worst_ratio(p[0], *R.colsum_prod(a, b), f"colsum_prod C={C} HW={HW}"))
    print(f"\nRATIO colmean C={C}: {worst['colmean']:.4f}   colsum_prod C={C}: {worst['colsum_prod']:.4f}")


def test_column_sums_count_every_pixel_once():
    """One pixel at a time holds a 1: the sum is 1 wherever the pixel lies -- first and last pixel of a chunk, of a lane round, of
    the map (C = 12: 85 lanes, HW = 64 * 85 + 1: the last pixel is the second one of lane 0 in chunk 63)."""
    C, HW = 12, 64 * 85 + 1
    per = -(-HW // 64)
    for p in (0, 1, 84, 85, 86, per - 1, per, per + 84, per + 85, HW - 2, HW - 1):
        a = np.zeros((1, 1, HW, C), np.float32)
        a[0, 0, p] = np.arange(1, C + 1)
        assert np.array_equal(ops.nhwc_colsum_prod(sl(a), sl(np.ones_like(a))).cpu().numpy()[0], np.arange(1, C + 1)), p


# ---- pool_sum ------------------------------------------------------------------------------------------------------------------
POOL = [(1, 4), (3, 84), (2, 128), (5, 52), (6, 64)]          # n_cam * C / 4 = 1, 63, 64, 65, 96


@pytest.mark.parametrize("n_cam,C", POOL)
def test_pool_sum(n_cam, C):
    """Lanes idle (1, 63), one full stride (64), a second partial stride (65, 96); size None / smaller / larger / equal in one
    axis; pad_to 1 and 4 with Ho Wo odd (B out_ld no multiple of the 4 outputs of a workgroup); the padding is exactly 0.
    Channel 0 of the integer map holds (image, y, x): the exact sum names the source pixels."""
    H, W = 7, 5
    worst = 0.0
    for B in (1, 3):
        for size in (None, (3, 3), (9, 11), (7, 9), (3, 5)):
            for pad_to in (1, 4):
                rng = rng_for(14, n_cam, C, B, pad_to, *(size or (0, 0)))
                x = ints(rng, (B * n_cam, H, W, C), -2, 2)
                x[..., 0] = np.arange(B * n_cam)[:, None, None] * 64 + np.arange(H)[None, :, None] * 8 + np.arange(W)[None, None, :]
                val, _ = R.pool_sum(x, n_cam, size, pad_to)
                got = ops.nhwc_pool_sum(sl(x), n_cam, size, pad_to)
                n = H * W if size is None else size[0] * size[1]
                assert got.shape == val.shape and got.shape[1] == -(-n // pad_to) * pad_to
                assert_bits(got, val.astype(np.float32), f"pool_sum ints n_cam={n_cam} C={C} B={B} size={size} pad_to={pad_to}")
                assert not got[:, n:].any() and not torch.signbit(got[:, n:]).any()
                x = normal(rng, (B * n_cam, H, W, C))
                g = [ops.nhwc_pool_sum(sl(x), n_cam, size, pad_to) for _ in range(2)]
                assert same_bits(g[0], g[1]) and not g[0][:, n:].any()
                worst = max(worst, worst_ratio(g[0], *R.pool_sum(x, n_cam, size, pad_to), "pool_sum"))
    print(f"\nRATIO pool_sum n_cam={n_cam} C={C}: {worst:.4f}")


# ---- affine_relu_bwd ---------------------------------------------------------------------------------------------------------------
def _arb(gy, y, scale, relu, gy2=None, two_entry=True):
    """C ABI with real buffers: gz is a slice of a sentinel buffer.  -> gz, sums (both checked for repeatability / neighbours)."""
    M, C = gy.shape
    L = _lib.lib()
    ts = None if scale is None else torch.from_numpy(scale).to(DEV)
    res = []
    for _ in range(2):
        g, v = sl(gy), sl(y, 8, 16)
        g2 = None if gy2 is None else sl(gy2, 4, 8)
        buf, gz = out_sl((M, C))
        sums = torch.full((2, C), SENT, dtype=torch.float32, device=DEV)
        nbytes = L.srf_nhwc_affine_relu_bwd_workspace_bytes(M, C)
        ws = torch.full((max(nbytes, 4) // 4 + 4,), SENT, dtype=torch.float32, device=DEV)
        if gy2 is None and not two_entry:
            rc = L.srf_nhwc_affine_relu_bwd(ops._ptr(g), g.stride(0), ops._ptr(v), v.stride(0), M, C, ops._ptr(ts), int(relu), ops._ptr(gz),
                                            gz.stride(0), ops._ptr(sums), ops._ptr(ws), nbytes, ops._stream())
        else:
            rc = L.srf_nhwc_affine_relu_bwd2(ops._ptr(g), g.stride(0), ops._ptr(g2), 0 if g2 is None else g2.stride(0), ops._ptr(v), v.stride(0),
                                             M, C, ops._ptr(ts), int(relu), ops._ptr(gz), gz.stride(0), ops._ptr(sums), ops._ptr(ws), nbytes,
                                             ops._stream())
        assert rc == 0
        assert untouched(buf, C) and torch.all(ws[nbytes // 4:] == SENT)
        res.append((gz.clone(), sums))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    return res[0]


ARB_M = [1, 255, 256, 257, 5 * 256, 16 * 256 + 1]        # 1, 1, 1, 2, 5, 17 blocks: empty, uneven and full finish segments


@pytest.mark.parametrize("C", [4, 12, 40, 1024])
def test_affine_relu_bwd(C):
    """rpp = 256, 85, 25, 1 rows per pass (idle threads at C = 12 and 40).  gz to the bit; the sums exactly on integers, within the
    bound on random data.  scale / relu / gy2 take every combination over the six M."""
    worst = [0.0, 0.0]
    for k, M in enumerate(ARB_M):
        rng = rng_for(15, C, M)
        for j in range(2):
            v = 2 * k + j
            has_scale, relu, has_gy2 = bool(v & 1), bool(v & 2) or v >= 8, bool(v & 4)
            gy, y = ints(rng, (M, C)), ints(rng, (M, C))
            gy2 = ints(rng, (M, C)) if has_gy2 else None
            scale = _pow2(rng, C) if has_scale else None
            gz, sums = _arb(gy, y, scale, relu, gy2, two_entry=bool(j))
            wz, ws, _ = R.affine_relu_bwd(gy, y, scale, relu, gy2)
            what = f"affine_relu_bwd ints M={M} C={C} scale={has_scale} relu={relu} gy2={has_gy2}"
            assert_bits(gz, wz, what)
            assert_bits(sums, ws.astype(np.float32), what)
            gy, y = normal(rng, (M, C)), normal(rng, (M, C)) + np.float32(0.3)
            gy2 = normal(rng, (M, C)) if has_gy2 else None
            scale = normal(rng, (C,)) if has_scale else None
            gz, sums = _arb(gy, y, scale, relu, gy2, two_entry=bool(j))
            wz, ws, bound = R.affine_relu_bwd(gy, y, scale, relu, gy2)
            assert_bits(gz, wz, what.replace("ints", "random"))
            for i in range(2):
                worst[i] = max(worst[i], worst_ratio(sums[i], ws[i], bound[i], what))
    print(f"\nRATIO affine_relu_bwd C={C}: sum gu {worst[0]:.4f}   sum gu y {worst[1]:.4f}")


def test_affine_relu_bwd_every_combination_at_one_shape():
    rng = rng_for(16)
    M, C = 300, 12
    gy, y, gy2, scale = ints(rng, (M, C)), ints(rng, (M, C)), ints(rng, (M, C)), _pow2(rng, C)
    for has_scale in (0, 1):
        for relu in (0, 1):
            for has_gy2 in (0, 1):
                gz, sums = _arb(gy, y, scale if has_scale else None, relu, gy2 if has_gy2 else None)
                wz, ws, _ = R.affine_relu_bwd(gy, y, scale if has_scale else None, relu, gy2 if has_gy2 else None)
                assert_bits(gz, wz)
                assert_bits(sums, ws.astype(np.float32))


def test_affine_relu_bwd_mask_is_y_above_zero():
    """+0, -0 are masked, the smallest subnormal is not; a NaN in y masks; a masked gy (NaN, inf) reaches neither gz nor the sums.
    (sum gu y adds gu * y = 0 * y for a masked row: NaN only where y itself is NaN or infinite -- column 3 -- which the output of a
    ReLU never is.)"""
    f = np.float32
    M, C = 260, 4
    y = np.ones((M, C), f)
    gy = np.ones((M, C), f)
    y[0], gy[0] = [0.0, -0.0, 2.0 ** -149, np.nan], [7.0, 7.0, 3.0, 5.0]
    y[1], gy[1] = [-1.0, -2.0, 0.0, -0.0], [np.nan, np.inf, -np.inf, np.nan]
    y[259], gy[259] = [0.0, 5.0, -0.0, 1.0], [9.0, 2.0, 9.0, 1.0]
    scale = np.array([2.0, -2.0, 2.0, 0.5], f)
    gz, sums = _arb(gy, y, scale, True)
    wz, ws, _ = R.affine_relu_bwd(gy, y, scale, True)
    assert_bits(gz, wz)
    assert_bits(sums, ws.astype(f))
    assert np.array_equal(wz[0], [0, -0.0, 6, 0]) and not wz[1].any() and np.array_equal(ws[0], [257, 259, 260, 258])
    assert ws[1][2] == 257 + 3 * 2.0 ** -149 and np.isnan(ws[1][3]) and ws[1][1] == 257 + 10
    # without the ReLU nothing is masked
    gz, sums = _arb(gy, y, None, False)
    wz, ws, _ = R.affine_relu_bwd(gy, y, None, False)
    assert_bits(gz, wz)
    assert_bits(sums, ws.astype(f))


def test_affine_relu_bwd_empty_batch_zeroes_the_sums():
    L = _lib.lib()
    C = 12
    sums = torch.full((2, C), SENT, dtype=torch.float32, device=DEV)
    g = torch.zeros((4, C), dtype=torch.float32, device=DEV)
    for entry in ("one", "two"):
        sums.fill_(SENT)
        if entry == "one":
            rc = L.srf_nhwc_affine_relu_bwd(ops._ptr(g), C, ops._ptr(g), C, 0, C, None, 1, ops._ptr(g), C, ops._ptr(sums), None, 0, ops._stream())
        else:
            rc = L.srf_nhwc_affine_relu_bwd2(ops._ptr(g), C, None, 0, ops._ptr(g), C, 0, C, None, 1, ops._ptr(g), C, ops._ptr(sums), None, 0,
                                             ops._stream())
        assert rc == 0 and not sums.any() and not torch.signbit(sums).any()


def test_affine_relu_bwd_through_ops_equals_the_c_abi():
    rng = rng_for(17)
    gy, y, gy2, scale = normal(rng, (2, 9, 15, 40)), normal(rng, (2, 9, 15, 40)), normal(rng, (2, 9, 15, 40)), normal(rng, (40,))
    gz, sums = ops.nhwc_affine_relu_bwd(sl(gy), sl(y, 8, 16), torch.from_numpy(scale).to(DEV), True, gy2=sl(gy2))
    wz, ws = _arb(gy.reshape(-1, 40), y.reshape(-1, 40), scale, True, gy2.reshape(-1, 40))
    assert same_bits(gz.reshape(-1, 40), wz) and same_bits(sums, ws)


# ---- eval-BatchNorm arithmetic -------------------------------------------------------------------------------------------------
# srf_bn_eval_fold against float64, in float32 ulps of the value (t0 = beta - mean s: of its larger term).  No accuracy statement
# for rsqrtf ships with the toolchain, so the bars are twice the worst case measured on an MI355X over the four C below
# (measured: see DESIGN.md section 2).
FOLD_ULPS = {"s": 3.3, "t0": 4.6, "inv": 2.0}             # measured: 1.642, 2.297, 0.985


def _bn_inputs(C, rng):
    gamma, beta, mean = normal(rng, (C,)), normal(rng, (C,)), normal(rng, (C,))
    var = (rng.random(C) * 2).astype(np.float32)
    gamma[::7] = 0.0                                         # the s == 0 branch of the gradients
    var[1::5] = (10.0 ** rng.uniform(-30, -6, size=len(var[1::5]))).astype(np.float32)     # tiny var: var + eps = eps (normal, no subnormals)
    var[2::11] = 0.0
    var[3::13] = (10.0 ** rng.uniform(1, 6, size=len(var[3::13]))).astype(np.float32)
    return gamma, beta, mean, var


@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_eval_fold_and_grads(C):
    rng = rng_for(18, C)
    worst = {"s": 0.0, "t0": 0.0, "inv": 0.0}
    for eps in (1e-5, 1e-3):
        gamma, beta, mean, var = _bn_inputs(C, rng)
        if C == 1:
            gamma[0] = 0.0 if eps == 1e-5 else 1.5
        t = [torch.from_numpy(a).to(DEV) for a in (gamma, beta, mean, var)]
        fold = ops.bn_eval_fold(*t, eps)
        assert same_bits(fold, ops.bn_eval_fold(*t, eps)) and fold.shape == (3, C)
        ref = R.bn_eval_fold(gamma, beta, mean, var, eps)
        got = fold.cpu().numpy().astype(np.float64)
        larger = np.maximum(np.abs(beta.astype(np.float64)), np.abs(mean.astype(np.float64) * ref[0]))
        for i, (name, scale_of) in enumerate((("s", np.abs(ref[0])), ("t0", larger), ("inv", ref[2]))):
            ulp = np.spacing(np.maximum(scale_of, 2.0 ** -126).astype(np.float32)).astype(np.float64)
            worst[name] = max(worst[name], float((np.abs(got[i] - ref[i]) / ulp).max()))
        assert np.all(got[0][gamma == 0] == 0)
        # gradients: single-rounded elementary operations, the same expressions through torch in float32 on the GPU
        sums = torch.from_numpy(np.stack([normal(rng, (C,)) * 50, normal(rng, (C,)) * 50])).to(DEV)
        g = ops.bn_eval_grads(sums, fold, t[2])
        assert same_bits(g, ops.bn_eval_grads(sums, fold, t[2]))
        s0, s1, sc, t0, inv = sums[0], sums[1], fold[0], fold[1], fold[2]
        z = torch.where(sc != 0, (s1 - t0 * s0) / sc, torch.zeros_like(sc))
        assert_bits(g, torch.stack([(z - t[2] * s0) * inv, s0]).cpu().numpy(), f"bn_eval_grads C={C}")
        want = R.bn_eval_grads(sums.cpu().numpy(), fold.cpu().numpy(), mean)
        assert np.allclose(g.cpu().numpy(), want, rtol=1e-4, atol=1e-4 * np.abs(want).max())
    print(f"\nRATIO bn_eval_fold C={C}: worst error in ulps s {worst['s']:.3f}  t0 {worst['t0']:.3f}  inv {worst['inv']:.3f}")
    for name in worst:
        assert worst[name] <= FOLD_ULPS[name], (name, worst[name])


# ---- host checks of ops.py: each raises before any launch ---------------------------------------------------------------------------
# Every mismatched operand is LARGER than the right one, so a wrapper without the check would still stay inside its buffers.
def _z(*shape):
    return torch.zeros(shape, dtype=torch.float32, device=DEV)


def test_upsample_add_refuses_mismatched_operands():
    lat = _z(2, 6, 6, 8)
    for top in (_z(3, 3, 3, 8), _z(2, 3, 3, 12)):
        with pytest.raises(ValueError):
            ops.nhwc_upsample_add(lat, top)
    for out in (_z(2, 6, 7, 8), _z(3, 6, 6, 8), _z(2, 6, 6, 12)):
        with pytest.raises(ValueError):
            ops.nhwc_upsample_add(lat, _z(2, 3, 3, 8), out=out)
    assert not lat.any()


def test_affine_refuses_mismatched_operands():
    x = _z(2, 3, 3, 8)
    for bad in (_z(2, 3, 4, 8), _z(3, 3, 3, 8), _z(2, 3, 3, 12)):
        with pytest.raises(ValueError):
            ops.nhwc_affine(x, residual=bad)
        with pytest.raises(ValueError):
            ops.nhwc_affine(x, out=bad)
    with pytest.raises(ValueError):
        ops.nhwc_affine(x, scale=_z(12))
    with pytest.raises(ValueError):
        ops.nhwc_affine(x, shift=_z(3, 8))


def test_affine_relu_bwd_refuses_another_y():
    gy = _z(2, 3, 3, 8)
    for y in (_z(2, 3, 4, 8), _z(2, 3, 3, 12), _z(3, 3, 3, 8)):
        with pytest.raises(ValueError):
            ops.nhwc_affine_relu_bwd(gy, y, None, True)
    with pytest.raises(ValueError):
        ops.nhwc_affine_relu_bwd(gy, gy, _z(12), True)
    with pytest.raises(ValueError):
        ops.nhwc_affine_relu_bwd(gy, gy, None, True, gy2=_z(2, 3, 4, 8))


def test_pool_sum_refuses_a_ragged_camera_count():
    with pytest.raises(ValueError):
        ops.nhwc_pool_sum(_z(7, 4, 4, 8), n_cam=6)
    with pytest.raises(ValueError):
        ops.nhwc_pool_sum(_z(5, 4, 4, 8), n_cam=6)
    assert ops.nhwc_pool_sum(_z(6, 4, 4, 8), n_cam=6).shape == (1, 16)


def test_vectors_of_the_wrong_length_are_refused():
    x = _z(2, 5, 5, 8)
    w = _z(8, 1, 3, 3)
    for kw in (dict(weight=_z(12, 1, 3, 3)), dict(weight=w, scale=_z(12)), dict(weight=w, shift=_z(12)), dict(weight=w, scale=_z(8), shift=_z(16))):
        with pytest.raises(ValueError):
            ops.nhwc_dwconv3x3s2(x, **kw)
    side, out = _z(2, 3, 3, 4), _z(2, 3, 3, 12)
    for args in ((_z(12, 1, 3, 3), None, None), (w, _z(12), None), (w, None, _z(12))):
        with pytest.raises(ValueError):
            ops.nhwc_dwconv3x3s2_cat(x, *args, True, side, out)
    with pytest.raises(ValueError):
        ops.nhwc_dwconv3x3s2(x, w, out=_z(2, 3, 4, 8))
    with pytest.raises(ValueError):
        ops.nhwc_maxpool3s2_ceil(x, out=_z(2, 2, 3, 8))
    with pytest.raises(ValueError):
        ops.nhwc_colsum_prod(x, _z(2, 5, 6, 8))
    with pytest.raises(ValueError):
        ops.bn_eval_fold(_z(8), _z(8), _z(12), _z(8), 1e-5)
    with pytest.raises(ValueError):
        ops.bn_eval_grads(_z(2, 12), _z(3, 8), _z(8))
    with pytest.raises(ValueError):
        ops.bn_eval_grads(_z(2, 8), _z(3, 12), _z(8))
