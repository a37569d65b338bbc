"""The definition of srf_conv_wgrad_nhwc_bf16 (csrc/wgrad_bf16.hip) in numpy -- what tests/test_gpu_wgrad_bf16.py holds the kernel to:

    dW[co][ci][ky][kx] = sum over p of bf16(g[p][co]) * bf16(X[p + tap][ci])

    p = (n, y, x) runs over the N H W output pixels; p + tap = (n, y + ky - pad, x + kx - pad); k = 1 (pad 0) or 3 (pad 1).
    * Each operand is rounded once, to nearest even (v_cvt_pk_bf16_f32 = Tensor.bfloat16()).
    * Every product is exact in f32 (v_mfma_f32_32x32x16_bf16); accumulation is f32.
    * Pixels outside the image contribute zero: X is zero-padded (a NaN of g times such a zero is NaN).
    * Pixel ranges are added in a fixed order; no atomics; two launches give the same bytes.
    * Non-finite values behave as IEEE arithmetic on the rounded operands.

Here the sum is taken in float64 (the products of two bf16 values are exact there too), so the kernel's f32 accumulation is the only
difference between it and `wgrad`."""
import numpy as np

from bf16_ref import bf16_round


def wgrad(g, x, k, rounded=True):
    """g (N, H, W, Cout), x (N, H, W, Cin) f32 -> (dW (Cout, Cin, k, k) float64, sum |g| |x| per output, same shape).
    rounded=False: the same on the operands as given (the UNROUNDED float64 weight gradient)."""
    g, x = np.asarray(g, dtype=np.float32), np.asarray(x, dtype=np.float32)
    N, H, W, Cin = x.shape
    Cout = g.shape[3]
    assert g.shape[:3] == (N, H, W) and k in (1, 3)
    pad = k // 2
    gr = (bf16_round(g) if rounded else g).astype(np.float64).reshape(-1, Cout)
    xr = (bf16_round(x) if rounded else x).astype(np.float64)
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = xr
    dW, mag = np.zeros((Cout, Cin, k, k)), np.zeros((Cout, Cin, k, k))
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(k):
            for kx in range(k):
                xs = xp[:, ky:ky + H, kx:kx + W].reshape(-1, Cin)      # X[p + tap], zero outside the image
                dW[:, :, ky, kx] = gr.T @ xs
                mag[:, :, ky, kx] = np.abs(gr).T @ np.abs(xs)
    return dW, mag
