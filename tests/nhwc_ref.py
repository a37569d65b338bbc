"""The definition of the streaming channels-last layers (csrc/nhwc.hip) in numpy -- what tests/test_gpu_nhwc_layers.py holds the
kernels to.  Arrays are (N, H, W, C) float32 unless said otherwise; nothing here imports torch or the project.

Element-wise kernels (affine, maxpool, upsample_add, affine_relu_bwd's gz) are defined to the bit: the library is built with
-ffp-contract=off and the kernels spell every rounding out, so a float32 numpy expression with one rounding per operation IS
the kernel's arithmetic.  The fma chain of the depthwise convolution cannot be reproduced in numpy without double rounding, and
the sums of the three reduction kernels depend on a summation tree: those are defined as the float64 value plus an error bound
gamma_d * sum |terms| whose d is the longest chain of rounded operations behind one output (derived from the kernel's structure,
not fitted); on data where every step is exact (small integers) they are bit-exact too.

max(a, b) everywhere is the GPU's fmaxf (v_max_f32): a NaN operand is dropped, and +0 is larger than -0.  So relu(NaN) = 0,
relu(-0) = +0, and a pooling window with a NaN returns the maximum of its other values.  The taps of a pooling window that lie past
the bottom / right edge count as -inf VALUES: a clipped window whose pixels are all NaN returns -inf, a whole window of nine NaN
returns NaN."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def gamma(d):
    """Higham's gamma_d for float32: the relative error bound of d successive roundings."""
    return d * U / (1.0 - d * U)


def fmaxf(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    r = np.fmax(a, b)                                   # drops a NaN operand
    zz = (a == 0) & (b == 0)
    return np.where(zz, np.where(np.signbit(a) & np.signbit(b), np.float32(-0.0), np.float32(0.0)), r).astype(np.float32)


def relu(v):
    return fmaxf(v, np.float32(0.0))


# ---- element-wise -----------------------------------------------------------------------------------------------------------
def affine(x, scale=None, shift=None, residual=None, relu_=False, per_sample=0):
    """x * scale, + shift, + residual, max(., 0): each step only if its operand is given, one float32 rounding each.
    scale / shift: (C,), or (N, C) where per_sample has bit 0 / bit 1."""
    v = np.asarray(x, np.float32)
    N, C = v.shape[0], v.shape[3]
    with np.errstate(all="ignore"):
        if scale is not None:
            s = np.asarray(scale, np.float32)
            v = v * (s.reshape(N, 1, 1, C) if per_sample & 1 else s.reshape(-1)[:C].reshape(1, 1, 1, C))
        if shift is not None:
            t = np.asarray(shift, np.float32)
            v = v + (t.reshape(N, 1, 1, C) if per_sample & 2 else t.reshape(-1)[:C].reshape(1, 1, 1, C))
        if residual is not None:
            v = v + np.asarray(residual, np.float32)
    return relu(v) if relu_ else v.astype(np.float32)


def pool3s2_out(h):
    """Output extent of MaxPool2d(3, 2, ceil_mode=True): ceil((h - 3) / 2) + 1, the last window dropped when it would start past
    the input; h = 1 and 2 give 1 (torch refuses h = 1; the library returns the one clipped window)."""
    ho = 1 if h < 3 else -(-(h - 3) // 2) + 1
    return ho - 1 if (ho - 1) * 2 >= h else ho


def maxpool3s2_ceil(x):
    x = np.asarray(x, np.float32)
    N, H, W, C = x.shape
    Ho, Wo = pool3s2_out(H), pool3s2_out(W)
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, np.float32)      # taps past the edge are -inf values
    xp[:, :H, :W] = x
    y = None
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
            y = tap.copy() if y is None else fmaxf(y, tap)
    return y


def nearest_index(n_out, n_in):
    """torch's 'nearest' source index, in float32: min(floor(f32(dst) * (f32(in) / f32(out))), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def upsample_add(lat, top):
    lat, top = np.asarray(lat, np.float32), np.asarray(top, np.float32)
    ys, xs = nearest_index(lat.shape[1], top.shape[1]), nearest_index(lat.shape[2], top.shape[2])
    with np.errstate(all="ignore"):
        return (lat + top[:, ys][:, :, xs]).astype(np.float32)


# ---- depthwise 3x3 / stride 2 / padding 1 -------------------------------------------------------------------------------------
def dwconv3x3s2(x, w, scale=None, shift=None, relu_=False):
    """-> (float64 value (N, Ho, Wo, C), magnitude sum |x w| |scale| + |shift| of the error bound).  w: (C, 3, 3) or (C, 1, 3, 3).
    Nine taps added from 0 in (ky, kx) order over the zero-padded input, then o * scale + shift (or o + shift), then max(., 0).
    The kernel does the same with one float32 fma per tap and one for scale / shift: at most 11 roundings (dwconv_bound)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    N, H, W, C = x.shape
    w = np.asarray(w, np.float32).astype(np.float64).reshape(C, 3, 3)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C))
    xp[:, 1:1 + H, 1:1 + W] = x
    acc, mag = np.zeros((N, Ho, Wo, C)), np.zeros((N, Ho, Wo, C))
    with np.errstate(all="ignore"):
        for ky in range(3):
            for kx in range(3):
                t = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] * w[:, ky, kx]
                acc, mag = acc + t, mag + np.abs(t)
        if scale is not None:
            s = np.asarray(scale, np.float32).astype(np.float64)
            acc, mag = acc * s, mag * np.abs(s)
        if shift is not None:
            t = np.asarray(shift, np.float32).astype(np.float64)
            acc, mag = acc + t, mag + np.abs(t)
        elif scale is not None:
            acc = acc + 0.0                     # fma(o, scale, +0): a product of -0 comes out as +0
    if relu_:
        acc = np.where(acc > 0, acc, 0.0)       # fmaxf(., 0): NaN and -0 give +0
    return acc, mag


def dwconv_bound(mag):
    """|kernel - value| <= gamma_11 * magnitude: nine fma of the chain, one for scale / shift, one spare for the final rounding
    of the float64 value to float32 in the comparison."""
    return gamma(11) * mag


def dwconv3x3s2_cat(side, x, w, scale=None, shift=None, relu_=False):
    """cat([side, dwconv(x)], channels): the copy is exact."""
    y, mag = dwconv3x3s2(x, w, scale, shift, relu_)
    side = np.asarray(side, np.float32).astype(np.float64)
    return np.concatenate([side, y], axis=3), np.concatenate([np.zeros_like(side), mag], axis=3)


# ---- reductions: float64 value + derived bound ------------------------------------------------------------------------------
def colsum_depth(HW, C, prod=False, mean=False):
    """Longest chain of float32 roundings behind one output of srf_nhwc_colsum_k + finish: per = ceil(HW / 64) pixels per chunk,
    lanes = 256 / (C / 4) pixel lanes: ceil(per / lanes) adds in a lane, lanes - 1 to combine them, 64 over the chunks."""
    per = -(-HW // 64)
    lanes = 256 // (C // 4)
    return -(-per // lanes) + (lanes - 1) + 64 + int(prod) + int(mean)


def colmean(x):
    """-> (sum over the pixels * f32(1 / HW) in float64 (N, C), bound).  The kernel multiplies by the ROUNDED reciprocal."""
    x = np.asarray(x, np.float32).astype(np.float64)
    N, H, W, C = x.shape
    inv = float(np.float32(1.0) / np.float32(H * W))
    return x.sum(axis=(1, 2)) * inv, gamma(colsum_depth(H * W, C, mean=True)) * np.abs(x).sum(axis=(1, 2)) * inv


def colsum_prod(a, b):
    """-> (sum over the pixels of a * b in float64 (N, C), bound)."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    N, H, W, C = a.shape
    t = a * b
    return t.sum(axis=(1, 2)), gamma(colsum_depth(H * W, C, prod=True)) * np.abs(t).sum(axis=(1, 2))


def pool_sum_depth(n_cam, C):
    """ceil(n_cam (C / 4) / 64) float4 sums added in a lane, 3 adds inside a float4 (two levels, counted as 3), 6 shuffle steps."""
    return -(-(n_cam * (C // 4)) // 64) + 3 + 6


def pool_sum(x, n_cam=1, size=None, pad_to=4):
    """x (B * n_cam, H, W, C) -> (value (B, out_ld) float64, bound): per output pixel the sum over cameras and channels at its
    'nearest' source pixel (an axis whose size is unchanged maps to itself); out_ld = Ho Wo rounded up to pad_to, the tail zero."""
    x = np.asarray(x, np.float32).astype(np.float64)
    Nimg, H, W, C = x.shape
    assert Nimg % n_cam == 0
    B = Nimg // n_cam
    Ho, Wo = (H, W) if size is None else (int(size[0]), int(size[1]))
    ys = np.arange(H) if Ho == H else nearest_index(Ho, H)
    xs = np.arange(W) if Wo == W else nearest_index(Wo, W)
    g = x[:, ys][:, :, xs].reshape(B, n_cam, Ho * Wo, C)
    out_ld = -(-(Ho * Wo) // pad_to) * pad_to
    val, mag = np.zeros((B, out_ld)), np.zeros((B, out_ld))
    val[:, :Ho * Wo] = g.sum(axis=(1, 3))
    mag[:, :Ho * Wo] = np.abs(g).sum(axis=(1, 3))
    return val, gamma(pool_sum_depth(n_cam, C)) * mag


def arb_depth(M, C, fma=False):
    """srf_affine_relu_bwd_k + finish: rpp = 256 / (C / 4) rows per pass: ceil(256 / rpp) adds in a thread, rpp to combine the
    threads, ceil(nb / 16) blocks in a finish segment (nb = ceil(M / 256)), 16 segments; + 1 for the fma of sum gu y."""
    rpp = 256 // (C // 4)
    nb = -(-M // 256)
    return -(-256 // rpp) + rpp + -(-nb // 16) + 16 + int(fma)


def affine_relu_bwd(gy, y, scale=None, relu_=True, gy2=None):
    """gy, y (, gy2): (M, C) -> gz (M, C) float32 (exact), sums (2, C) float64 [sum gu, sum gu y], bound (2, C).
    g = gy (+ gy2, one rounding); gu = g where not relu or y > 0, else +0 (a NaN in y masks); gz = gu * scale, one rounding.
    The sums are IEEE: a masked row contributes gu y = 0 * y, which is NaN where y is NaN or infinite."""
    g = np.asarray(gy, np.float32)
    y = np.asarray(y, np.float32)
    M, C = g.shape
    with np.errstate(all="ignore"):
        if gy2 is not None:
            g = g + np.asarray(gy2, np.float32)
        gu = np.where(y > 0, g, np.float32(0.0)).astype(np.float32) if relu_ else g.astype(np.float32)
        gz = gu if scale is None else (gu * np.asarray(scale, np.float32).reshape(1, C)).astype(np.float32)
        gu64, t = gu.astype(np.float64), gu.astype(np.float64) * y.astype(np.float64)
        sums = np.stack([gu64.sum(axis=0), t.sum(axis=0)])
        mag = np.stack([np.abs(gu64).sum(axis=0) * gamma(arb_depth(M, C)), np.abs(t).sum(axis=0) * gamma(arb_depth(M, C, fma=True))])
    return gz, sums, mag


# ---- the per-channel arithmetic of an eval-mode BatchNorm --------------------------------------------------------------------
def bn_eval_fold(gamma_, beta, mean, var, eps):
    """-> (3, C) float64: s = gamma inv, t0 = beta - mean s, inv = 1 / sqrt(var + eps); eps is the float32 the C ABI takes."""
    g, b, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (gamma_, beta, mean, var))
    inv = 1.0 / np.sqrt(v + float(np.float32(eps)))
    s = g * inv
    return np.stack([s, b - m * s, inv])


def bn_eval_grads(sums, fold, mean):
    """sums (2, C) = [sum gu, sum gu y], fold (3, C) = [s, t0, inv] -> (2, C) float64:
    d gamma = ((s != 0 ? (sum gu y - t0 sum gu) / s : 0) - mean sum gu) inv, d beta = sum gu."""
    sums, fold, mean = np.asarray(sums, np.float64), np.asarray(fold, np.float64), np.asarray(mean, np.float64)
    s0, s1, sc, t0, inv = sums[0], sums[1], fold[0], fold[1], fold[2]
    with np.errstate(all="ignore"):
        z = np.where(sc != 0, (s1 - t0 * s0) / np.where(sc != 0, sc, 1.0), 0.0)
    return np.stack([(z - mean * s0) * inv, s0])
