"""The definition of the bf16-product mode (csrc/gemm_bf16.hip) in numpy -- what tests/test_gpu_gemm_bf16.py holds the kernels to:

    y = epilogue( sum_k bf16(x_k) * bf16(w_k) )

with bf16() = round to nearest even of the f32 value to 8 significant bits (as v_cvt_pk_bf16_f32 and torch.Tensor.bfloat16()), the
sum taken here in float64 (every product of two bf16 values is exact in float64, and in f32).  Nothing else is rounded."""
import numpy as np

BF16_MAX = float.fromhex("0x1.FEp127")     # the largest bf16; |x| > 0x1.FEFFFFp127 rounds to infinity
FLT_MIN = float.fromhex("0x1p-126")        # below it a bf16 is subnormal


def bf16_round(x):
    """f32 array -> f32 array whose values are the bf16 roundings (RNE, by bit arithmetic).  +-inf stay, NaN stays NaN (quiet),
    finite values beyond the largest bf16 become +-inf, subnormals are rounded on the subnormal grid (not flushed)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    nan = np.isnan(x)
    r = np.where(nan, (x.view(np.uint32) & np.uint32(0x80000000)) | np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape)


def gemm(x, w):
    """x (M, K), w (Cout, K) f32 -> (float64 product of the ROUNDED operands (M, Cout), sum |a b| of the rounded operands)."""
    xr, wr = bf16_round(x).astype(np.float64), bf16_round(w).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return xr @ wr.T, np.abs(xr) @ np.abs(wr).T


def im2col(x, kh, kw, stride, pad):
    """x (N, H, W, C) -> (N, Ho, Wo, kh * kw * C): k = (tap, channel), tap slowest -- the order of the packed conv weights."""
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, C), dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] for ky in range(kh) for kx in range(kw)]
    return np.concatenate(cols, axis=3)


def conv(x, w, stride, pad):
    """x (N, H, W, Cin), w (Cout, Cin, kh, kw) f32 -> (float64 convolution of the rounded operands (N, Ho, Wo, Cout), sum |a b|)."""
    Cout, Cin, kh, kw = w.shape
    cols = im2col(np.asarray(x, dtype=np.float32), kh, kw, stride, pad)
    y, mag = gemm(cols.reshape(-1, kh * kw * Cin), np.asarray(w, dtype=np.float32).transpose(0, 2, 3, 1).reshape(Cout, -1))
    return y.reshape(cols.shape[:3] + (Cout,)), mag.reshape(cols.shape[:3] + (Cout,))


def epilogue(acc, scale=None, shift=None, relu=False):
    y = acc * (1.0 if scale is None else np.asarray(scale, dtype=np.float64)) + (0.0 if shift is None else np.asarray(shift, dtype=np.float64))
    return np.maximum(y, 0.0) if relu else y
