"""The definition of the bf16-product mode of the sparse convolution (csrc/spconv_bf16.hip) in numpy -- what
tests/test_gpu_spconv_bf16.py holds the kernel to:

    out[o, :] = epilogue( sum over offsets k with nbr[k][o] >= 0, over channels c of  bf16(x[nbr[k][o], c]) * bf16(W[k, c, :]) )

with bf16() = round to nearest even (tests/bf16_ref.bf16_round: as v_cvt_pk_bf16_f32 and torch.Tensor.bfloat16()), every product exact,
the sum taken here in float64.  epilogue = fma(acc, alpha, beta), + residual, ReLU; alpha, beta and the residual are not rounded."""
import numpy as np

from bf16_ref import bf16_round


def conv(x, W, nbr, rounded=True):
    """x (A_in, Cin), W (K, Cin, Cout) f32, nbr (K, A_out) int (-1: no pair) -> (float64 sum of the rounded operands' products
    (A_out, Cout), sum |a b| of the rounded operands (A_out, Cout), number of terms per output row (A_out,)).
    rounded=False: the same on the operands as given (the UNROUNDED float64 convolution)."""
    x, W, nbr = np.asarray(x, dtype=np.float32), np.asarray(W, dtype=np.float32), np.asarray(nbr)
    xr = (bf16_round(x) if rounded else x).astype(np.float64)
    Wr = (bf16_round(W) if rounded else W).astype(np.float64)
    K, Cin, Cout = W.shape
    A_out = nbr.shape[1]
    acc, mag, terms = np.zeros((A_out, Cout)), np.zeros((A_out, Cout)), np.zeros(A_out, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            o = np.nonzero(nbr[k] >= 0)[0]
            if len(o) == 0:
                continue
            rows = xr[nbr[k, o]]
            acc[o] += rows @ Wr[k]
            mag[o] += np.abs(rows) @ np.abs(Wr[k])
            terms[o] += Cin
    return acc, mag, terms


def epilogue(acc, alpha=None, beta=None, residual=None, relu=False):
    y = acc if alpha is None else acc * np.asarray(alpha, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    if residual is not None:
        y = y + np.asarray(residual, dtype=np.float64)
    return np.maximum(y, 0.0) if relu else y
