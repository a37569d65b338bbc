"""The definition of the implicit-im2col convolution of the three dense GEMM families -- srf_conv_gemm_nhwc (csrc/conv.hip),
srf_conv_gemm_nhwc_split (csrc/gemm_split.hip), srf_conv_gemm_nhwc_bf16 (csrc/gemm_bf16.hip) -- in numpy, with the cases
tests/test_gpu_conv_gemm_edges.py runs and the error bounds it holds them to.  tests/test_conv_gemm_ref.py checks this file on the CPU.

    y[n][oy][ox][co] = epilogue( sum over (ky, kx, ci) of x[n][oy s - p + ky][ox s - p + kx][ci] w[co][ci][ky][kx] ),   zero outside the map,

k = (tap, channel) with the tap slowest, one padding `p` and one stride `s` for both axes (the ABI has no other), any kh, kw > 0.
`conv` is the UNROUNDED float64 value (the f32 and the split family); `bf16_ref.conv` is the float64 value of the operands rounded to
bf16 (the bf16 family).  Both return mag = sum |x| |w| per output, the scale of every rounding-error bound.

Two kinds of data:
  * integers below 2^8 in magnitude, sparse activations (`int_case`).  They are bf16 values, so all three families see the same
    operands; under `exact_condition` every partial sum of every summation order is an integer below 2^24, hence exact in f32, and the
    result is THE integer: the GPU test compares with torch.equal;
  * post-ReLU activations and randn weights (`real_case`), held per output to `bound_f32` / `bound_split`, which are derived below and
    not measured."""
import functools

import numpy as np

import bf16_ref as R

U = 2.0 ** -24      # unit roundoff of f32

# (N, H, W, Cin, Cout, kh, kw, stride, pad): the smallest shapes that reach the edge named
GEOMETRY = [
    (2, 5, 7, 32, 37, 1, 3, 1, 1),      # kw != kh; pad > kh / 2: the first and last output rows see only padding; cin_chunks == 1; odd
                                        # Cout; K = 96: the last 64-block of the bf16 kernel is half empty
    (2, 6, 5, 96, 40, 3, 1, 1, 0),      # kw == 1 under kh == 3: the bf16 walker bumps ky with every tap; Cin = 96: a 64-block straddles a tap
    (1, 6, 7, 32, 129, 2, 2, 2, 0),     # even kernel; Cout just above a column tile
    (1, 9, 11, 64, 260, 3, 5, 2, 2),    # kw > kh; pad = 2 = kw / 2 across and > kh / 2 down; Cout > 256 (a second packed block of the f32 family)
    (3, 7, 9, 32, 72, 3, 3, 1, 0),      # 3x3 without padding; M = 105: image boundaries inside one row tile
    (1, 4, 5, 64, 40, 3, 3, 1, 3),      # pad >= k: the outermost ring of outputs is epilogue(0) = relu(shift)
    (2, 1, 2, 32, 8, 3, 3, 1, 1),       # a map smaller than the kernel
    (1, 10, 13, 32, 40, 3, 3, 3, 1),    # stride 3; (H + 2 pad - kh) % stride != 0
    (1, 9, 9, 64, 40, 1, 1, 4, 0),      # stride > k: most input pixels are read by no output
    (3, 21, 19, 32, 40, 3, 3, 1, 1),    # M = 1197: 10 row blocks of 128 = two groups of 8, six workgroups past the grid, a partial last block
]
# the 128 x 128 tile of the f32 family with a stride: Ho x Wo = 64 x 65, M = 12480 = 97.5 row blocks, 4 column tiles: 392 live tiles
BIG = (3, 127, 129, 32, 512, 3, 3, 2, 1)
BIG_TWIN_COUT = 384                     # the same rows at 3 column tiles: 294 live tiles, the 64 x 64 form
# the real-valued cases: one non-square, one strided 3x3
REAL = [GEOMETRY[3], GEOMETRY[7]]
# the pitched cases: one strided 3x3, the 1 x 3 kernel
PITCHED = [GEOMETRY[7], GEOMETRY[0]]


def case_id(case):
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    return f"{N}x{H}x{W}x{Cin}-{Cout}-k{kh}x{kw}-s{stride}-p{pad}"


def out_size(case):
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


def live_tiles(case, cout=None):
    """128 x 128 tiles that hold real rows and channels: what srf_conv_gemm_nhwc compares with its threshold (csrc/conv.hip, `live`)."""
    Ho, Wo = out_size(case)
    return -(-(case[0] * Ho * Wo) // 128) * -(-(case[4] if cout is None else cout) // 128)


def conv(x, w, stride, pad):
    """x (N, H, W, Cin), w (Cout, Cin, kh, kw) -> (float64 convolution of the operands AS THEY ARE (N, Ho, Wo, Cout), sum |x| |w|)."""
    Cout, Cin, kh, kw = w.shape
    cols = R.im2col(np.asarray(x, dtype=np.float64), kh, kw, stride, pad)
    a = cols.reshape(-1, kh * kw * Cin)
    b = np.asarray(w, dtype=np.float64).transpose(0, 2, 3, 1).reshape(Cout, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        y, mag = a @ b.T, np.abs(a) @ np.abs(b).T
    return y.reshape(cols.shape[:3] + (Cout,)), mag.reshape(cols.shape[:3] + (Cout,))


def covers(mask, kh, kw, stride, pad):
    """mask (N, H, W) bool -> (N, Ho, Wo) bool: the outputs whose window holds a marked pixel."""
    return R.im2col(np.asarray(mask, dtype=np.float64)[..., None], kh, kw, stride, pad).sum(axis=3) > 0


def _rng(case, salt):
    return np.random.default_rng([salt] + list(case))


def int_case(case, epilogue=True):
    """-> x, w, scale, shift (f32 arrays of integers; scale = shift = None without `epilogue`).  |x|, |w| <= 255; about 8 non-zero
    activations per dot product (as _sparse_ints of test_gpu_gemm_bf16.py); scale in +-{1, 2, 3}, shift in -8 .. 8."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    g = _rng(case, 1)
    x = g.integers(-255, 256, (N, H, W, Cin)) * (g.integers(0, max(1, kh * kw * Cin // 8), (N, H, W, Cin)) == 0)
    w = g.integers(-255, 256, (Cout, Cin, kh, kw))
    if not epilogue:
        return x.astype(np.float32), w.astype(np.float32), None, None
    scale = g.integers(1, 4, Cout) * (g.integers(0, 2, Cout) * 2 - 1)
    shift = g.integers(-8, 9, Cout)
    return x.astype(np.float32), w.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32)


def exact_condition(want, mag, scale=None, shift=None):
    """The condition under which any kernel of any family must return `want` bit for bit: every partial sum of any order is an
    integer of magnitude <= mag < 2^24, the fma of the epilogue has an integer result below 2^24 too, and the map is not all zero."""
    s = 1.0 if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    h = 0.0 if shift is None else np.abs(np.asarray(shift, dtype=np.float64))
    return bool(mag.max() < 2 ** 24 and (mag * s + h).max() < 2 ** 24 and np.abs(want).max() > 0)


@functools.lru_cache(maxsize=None)
def int_reference(case, epilogue=True):
    """-> x, w, scale, shift, acc, mag of `int_case`: computed once per process and shared; nobody writes into them."""
    x, w, scale, shift = int_case(case, epilogue)
    acc, mag = conv(x, w, case[7], case[8])
    return x, w, scale, shift, acc, mag


@functools.lru_cache(maxsize=None)
def real_reference(case, rounded=False):
    """-> x, w, scale, shift, acc, mag of `real_case`; rounded: acc and mag of the operands rounded to bf16 (bf16_ref.conv)."""
    x, w, scale, shift = real_case(case)
    acc, mag = (R.conv if rounded else conv)(x, w, case[7], case[8])
    return x, w, scale, shift, acc, mag


def real_case(case):
    """-> x (post-ReLU: ~45 % zeros), w (randn / sqrt(K)), scale in [0.5, 1.5), shift > 0: f32 arrays."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    g = _rng(case, 2)
    x = np.maximum(g.standard_normal((N, H, W, Cin)) * 1.5 + 0.2, 0.0)
    w = g.standard_normal((Cout, Cin, kh, kw)) / np.sqrt(kh * kw * Cin)
    scale, shift = g.random(Cout) + 0.5, g.random(Cout) * 0.2 + 0.01
    return x.astype(np.float32), w.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): n roundings to f32 in sequence change a value by at most this factor - 1."""
    return n * U / (1.0 - n * U)


def _epilogue_term(want, shift):
    # y = fl(fma(acc, scale, shift)) is ONE rounding of a value of magnitude <= max(|y|, |shift|) (1 + small); the factor 2 covers the
    # "small" and an accumulator error that moves y across the ReLU's zero
    return 0.0 if shift is None else 2.0 * U * np.maximum(np.abs(want), np.abs(np.asarray(shift, dtype=np.float64)))


def bound_f32(K, mag, want, scale=None, shift=None):
    """f32 family (and the bf16 family against the float64 of its ROUNDED operands): a sum of K products accumulated in f32 in any
    order, each product rounded at most once with its addition (fma) -- at most K roundings on the way of any term: gamma_K sum |a b|;
    scaled by |scale| in the epilogue, plus the epilogue's own rounding."""
    s = 1.0 if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    return gamma(K) * s * mag + _epilogue_term(want, shift)


def bound_split(K, mag, want, scale=None, shift=None):
    """Split family: six exact partial products per product accumulated in f32 -- 6 K terms, no rounding in a product, at most 6 K
    roundings on the way of any term: gamma_{6K} sum |a b| -- and three dropped partial products that are together below 2^-23 |a b|
    (the header of csrc/gemm_split.hip)."""
    s = 1.0 if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    return (gamma(6 * K) + 2.0 ** -23) * s * mag + _epilogue_term(want, shift)
