"""tests/conv_gemm_ref.py (no GPU): the reference tests/test_gpu_conv_gemm_edges.py holds the three implicit-im2col kernels to is
torch's float64 convolution on every geometry of its table; every integer case meets the condition under which `torch.equal` is the
right assertion; every real-valued case's bound is far below the size of one dropped or misplaced tap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R
import conv_gemm_ref as C

ALL = C.GEOMETRY + [C.BIG]


def _torch_conv(x, w, stride, pad):
    y = F.conv2d(torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2), torch.from_numpy(np.asarray(w, dtype=np.float64)),
                 stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", ALL, ids=C.case_id)
def test_reference_is_torch_conv2d_in_float64(case):
    """Real-valued data (an integer case would hide a tap swapped with an all-zero neighbour): the unrounded reference, its sum |x| |w|,
    and the rounded one of bf16_ref on the same geometry -- non-square kernels, pad >= k, maps smaller than the kernel included."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    g = np.random.default_rng(list(case))
    x, w = g.standard_normal((N, H, W, Cin)), g.standard_normal((Cout, Cin, kh, kw))
    got, mag = C.conv(x, w, stride, pad)
    want = _torch_conv(x, w, stride, pad)
    assert got.shape == want.shape == (N,) + C.out_size(case) + (Cout,)
    tol = 1e-13 * mag.max()                     # float64 sums of K <= 960 terms in two orders
    assert np.abs(got - want).max() <= tol
    assert np.abs(mag - _torch_conv(np.abs(x), np.abs(w), stride, pad)).max() <= tol
    if case != C.BIG:
        x32, w32 = x.astype(np.float32), w.astype(np.float32)
        got_r, mag_r = R.conv(x32, w32, stride, pad)
        assert np.abs(got_r - _torch_conv(R.bf16_round(x32), R.bf16_round(w32), stride, pad)).max() <= tol
        assert np.abs(mag_r - mag).max() <= 2.0 ** -6 * mag.max()


def test_a_padding_of_the_kernel_size_leaves_a_ring_of_zeros():
    """pad >= k: the outermost outputs see nothing but padding (the GPU test then wants relu(shift) there, exactly)."""
    case = C.GEOMETRY[5]
    x, w, scale, shift, acc, mag = C.int_reference(case)
    assert case[8] >= case[5] and case[8] >= case[6]
    ring = np.ones(acc.shape[:3], dtype=bool)
    ring[:, 1:-1, 1:-1] = False
    assert (mag[ring] == 0).all() and (mag[~ring] > 0).any()
    # and the 1 x 3 kernel with pad 1: the first and the last output row
    x, w, scale, shift, acc, mag = C.int_reference(C.GEOMETRY[0])
    assert (mag[:, 0] == 0).all() and (mag[:, -1] == 0).all() and (mag[:, 1:-1] > 0).any()


@pytest.mark.parametrize("case", ALL, ids=C.case_id)
@pytest.mark.parametrize("epilogue", [False, True])
def test_integer_cases_are_exact_in_f32(case, epilogue):
    x, w, scale, shift, acc, mag = C.int_reference(case, epilogue)
    for a in (x, w) + ((scale, shift) if epilogue else ()):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() < 2 ** 8
    assert np.array_equal(R.bf16_round(x), x) and np.array_equal(R.bf16_round(w), w)          # the bf16 family sees the same operands
    print(f"\n[{C.case_id(case)}] max sum |x||w| = {mag.max():.0f} = 2^{np.log2(mag.max()):.1f}, non-zero outputs: {(acc != 0).mean():.2f}")
    assert C.exact_condition(acc, mag, scale, shift)
    for relu in (False, True):
        want = R.epilogue(acc, scale, shift, relu)
        assert np.abs(want).max() > 0 and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert (R.epilogue(acc, scale, shift, False) < 0).any()      # the ReLU has something to do


def test_the_big_case_reaches_the_128_tile_and_its_twin_does_not():
    assert C.out_size(C.BIG) == (64, 65)
    assert C.live_tiles(C.BIG) == 392 and C.live_tiles(C.BIG, C.BIG_TWIN_COUT) == 294
    assert max(C.live_tiles(c) for c in C.GEOMETRY) < 294


@pytest.mark.parametrize("case", C.REAL, ids=C.case_id)
def test_real_valued_bounds_are_far_below_one_tap(case):
    """A dropped or misplaced tap is an error of order mag / (kh kw) >= mag / 15: a bound below 1e-3 of max mag cannot hide it."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    K = kh * kw * Cin
    for rounded in (False, True):
        x, w, scale, shift, acc, mag = C.real_reference(case, rounded)
        for sc, sh in ((None, None), (scale, shift)):
            want = R.epilogue(acc, sc, sh, sc is not None)
            for name, bound in (("f32", C.bound_f32), ("split", C.bound_split)):
                b = bound(K, mag, want, sc, sh)
                print(f"\n[{C.case_id(case)} {name}{' rounded' if rounded else ''}{' epilogue' if sc is not None else ''}] "
                      f"max bound / max mag = {b.max() / mag.max():.3g}")
                assert b.shape == mag.shape and (b >= 0).all()
                assert b.max() < 1e-3 * mag.max()
    assert (x == 0).mean() > 0.3 and (scale > 0).all() and (shift > 0).all()


def test_covers_marks_the_windows_of_a_pixel():
    m = np.zeros((1, 9, 11), dtype=bool)
    m[0, 3, 5] = True
    c = C.covers(m, 3, 3, 2, 1)
    assert c.shape == (1, 5, 6) and sorted(zip(*np.nonzero(c)[1:])) == [(1, 2), (1, 3), (2, 2), (2, 3)]
    m[:] = False
    m[0, 0, 0] = True
    assert sorted(zip(*np.nonzero(C.covers(m, 3, 3, 2, 1))[1:])) == [(0, 0)]
