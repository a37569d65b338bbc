"""tests/spconv_bf16_ref.py (the definition csrc/spconv_bf16.hip is held to) checked without a GPU: against naive loops on a hand-sized
rulebook, and against tests/spconv_ref.conv_ref on operands that are bf16 values already (where rounding changes nothing)."""
import numpy as np
import torch

import spconv_bf16_ref as R
import spconv_ref
from bf16_ref import bf16_round


def _hand_rulebook():
    # K = 3 offsets, 5 outputs, 4 inputs: output 2 has no pair, offset 1 is unused, input 3 (the last) feeds three outputs
    return np.array([[0, 3, -1, 3, 1],
                     [-1, -1, -1, -1, -1],
                     [2, -1, -1, 3, 3]], dtype=np.int32)


def test_against_naive_loops():
    rng = np.random.default_rng(0)
    nbr = _hand_rulebook()
    x = rng.standard_normal((4, 6)).astype(np.float32)
    W = rng.standard_normal((3, 6, 5)).astype(np.float32)
    acc, mag, terms = R.conv(x, W, nbr)
    xr, Wr = bf16_round(x).astype(np.float64), bf16_round(W).astype(np.float64)
    assert not np.array_equal(xr, x.astype(np.float64))          # the rounding does something
    want, wmag, wterms = np.zeros((5, 5)), np.zeros((5, 5)), np.zeros(5, dtype=np.int64)
    for o in range(5):
        for k in range(3):
            i = nbr[k, o]
            if i < 0:
                continue
            wterms[o] += 6
            for c in range(6):
                for n in range(5):
                    want[o, n] += xr[i, c] * Wr[k, c, n]
                    wmag[o, n] += abs(xr[i, c] * Wr[k, c, n])
    np.testing.assert_allclose(acc, want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(mag, wmag, rtol=0, atol=1e-14)
    assert np.array_equal(terms, wterms) and terms[2] == 0 and not acc[2].any()
    # rounded=False is the same sum on the operands as given
    raw, _, _ = R.conv(x, W, nbr, rounded=False)
    want_raw = sum(np.where((nbr[k] >= 0)[:, None], x[np.maximum(nbr[k], 0)].astype(np.float64) @ W[k].astype(np.float64), 0.0) for k in range(3))
    np.testing.assert_allclose(raw, want_raw, rtol=0, atol=1e-14)


def test_epilogue_order():
    acc = np.array([[-3.0, 2.0]])
    y = R.epilogue(acc, alpha=[2.0, 0.5], beta=[1.0, -4.0], residual=[[4.0, 1.0]], relu=True)
    assert np.array_equal(y, [[0.0, 0.0]])                       # (-6 + 1 + 4 = -1 -> 0), (1 - 4 + 1 = -2 -> 0)
    assert np.array_equal(R.epilogue(acc, alpha=[2.0, 0.5], beta=[1.0, -4.0], residual=[[4.0, 1.0]]), [[-1.0, -2.0]])
    assert np.array_equal(R.epilogue(acc), acc) and np.array_equal(R.epilogue(acc, relu=True), [[0.0, 2.0]])


def test_against_conv_ref_on_bf16_operands():
    rng = np.random.default_rng(1)
    K, A_in, A_out, Cin, Cout = 27, 40, 33, 32, 64
    nbr = rng.integers(-1, A_in, size=(K, A_out)).astype(np.int32)
    nbr[:, 7] = -1
    nbr[5] = -1
    x = bf16_round(rng.standard_normal((A_in, Cin)).astype(np.float32))
    W = bf16_round(rng.standard_normal((K, Cin, Cout)).astype(np.float32))
    acc, mag, terms = R.conv(x, W, nbr)
    g = torch.zeros(A_out, Cout)
    (out, _, _), (omag, _, _) = spconv_ref.conv_ref(torch.from_numpy(nbr), torch.from_numpy(x), torch.from_numpy(W), g)
    np.testing.assert_allclose(acc, out.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(mag, omag.numpy(), rtol=0, atol=1e-12)
    assert np.array_equal(terms, (nbr >= 0).sum(0) * Cin)
    # on bf16 operands rounding is the identity
    assert np.array_equal(R.conv(x, W, nbr, rounded=False)[0], acc)
