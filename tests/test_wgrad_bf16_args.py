"""Argument checks of srf_conv_wgrad_nhwc_bf16 (csrc/wgrad_bf16.hip) and the mode's layer limits (train_conv.bf16_layer_ok); no GPU.

Every pointer is a fake address and every row of the return-code table is REFUSED, so no row ever launches a kernel: the codes are all
decided before any HIP call, in the order of the other entry points (SRF_EINVAL, then SRF_EUNSUPPORTED, then SRF_EWORKSPACE)."""
import pytest
import torch

from srfdet3d_amd import _lib, train_conv

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
P = 0x10000            # 16-byte aligned, never dereferenced
BIG = 1 << 40          # a workspace size that is always enough


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def call(L, g=P, g_ld=64, x=P, x_ld=32, N=2, H=5, W=7, Cin=32, Cout=64, k=3, ws=P, ws_bytes=0, dW=P):
    return L.srf_conv_wgrad_nhwc_bf16(g, g_ld, x, x_ld, N, H, W, Cin, Cout, k, ws, ws_bytes, dW, None)


def test_the_base_row_is_refused_only_for_its_workspace(L):
    assert call(L) == EWORKSPACE            # every other check passes: the rows below each break one thing
    need = L.srf_conv_wgrad_bf16_workspace_bytes(2, 5, 7, 32, 64, 3)
    assert need > 0 and call(L, ws_bytes=need - 1) == EWORKSPACE


ROWS = [
    (dict(N=0), EINVAL), (dict(H=0), EINVAL), (dict(W=-1), EINVAL), (dict(Cin=0), EINVAL), (dict(Cout=0), EINVAL),
    (dict(g=None), EINVAL), (dict(x=None), EINVAL), (dict(dW=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(g_ld=60), EINVAL), (dict(x_ld=28), EINVAL),                       # a pitch below the channel count
    (dict(g=None, k=5), EINVAL),                                            # the null pointer before the shape
    (dict(k=5), EUNSUPPORTED), (dict(k=2), EUNSUPPORTED), (dict(k=0), EUNSUPPORTED),
    (dict(Cin=30, x_ld=32), EUNSUPPORTED), (dict(Cout=62), EUNSUPPORTED),
    (dict(g_ld=66), EUNSUPPORTED), (dict(x_ld=34), EUNSUPPORTED),
    (dict(g=P + 4), EUNSUPPORTED), (dict(x=P + 8), EUNSUPPORTED), (dict(ws=P + 4), EUNSUPPORTED),
    (dict(N=1, H=1, W=(1 << 31) // (64 * 4)), EUNSUPPORTED),                # g of exactly 2 GB
    (dict(N=1, H=1, W=(1 << 31) // (64 * 4) - 1, x_ld=128), EUNSUPPORTED),  # x's pitch makes it 2 GB
    (dict(k=5, ws_bytes=BIG), EUNSUPPORTED),                                # the shape before the workspace
    (dict(W=1), EWORKSPACE), (dict(k=1), EWORKSPACE), (dict(Cin=36, x_ld=36, Cout=20, g_ld=20), EWORKSPACE),   # all taken, but for ws_bytes = 0
]


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_return_code_table(L, i):
    kw, want = ROWS[i]
    assert call(L, **kw) == want, kw


def test_workspace_bytes(L):
    f = L.srf_conv_wgrad_bf16_workspace_bytes
    for bad in [(0, 5, 7, 32, 64, 3), (2, 5, 7, 32, 64, 2), (2, 5, 7, 0, 64, 3), (1, 1, (1 << 31) // 256, 32, 64, 1)]:
        assert f(*bad) == 0, bad
    # one pixel range here: partial sums, then the two planes (channels padded to 8, 2 bytes each), every part rounded up to 256 bytes
    up = lambda v: (v + 255) // 256 * 256
    assert f(2, 5, 7, 36, 20, 3) == up(20 * 9 * 36 * 4) + up(70 * 24 * 2) + up(70 * 40 * 2)


# (k, N, H, W, Cin, Cout) -> verdict, and where it comes from
LAYERS = [
    ((3, 2, 21, 34, 64, 96), True, "both channel counts in chunks of 32"),
    ((1, 2, 21, 34, 192, 256), True, ""),
    ((3, 2, 21, 34, 48, 64), False, "Cin & 31: the forward's K (csrc/gemm_host.hpp, srf_gemm_check_conv)"),
    ((3, 2, 21, 34, 64, 48), False, "Cout & 31: the data gradient's K"),
    ((1, 2, 21, 34, 36, 64), False, "K & 31 (srf_gemm_check_1x1)"),
    ((5, 2, 21, 34, 64, 64), False, "1x1 and 3x3 only"),
    ((3, 0, 21, 34, 64, 64), False, "an empty batch has no layer"),
    ((1, 1, 1, 1, 32, (1 << 22) - 32), True, "128 rows of 2^22 - 32 floats: 2^31 - 2^14 bytes"),
    ((1, 1, 1, 1, 32, 1 << 22), False, "128 rows of 2^22 floats are 2^31 bytes (x_ld * tile_rows * 4)"),
    ((3, 1, 1 << 10, 1 << 10, 32, 480), True, "one image of 480 channels: 2^31 - 2^27 bytes"),
    ((3, 1, 1 << 10, 1 << 10, 32, 512), False, "one image of the data gradient's input is 2^31 bytes (*x_bytes >= 2^31)"),
    ((1, 1, 1 << 10, 1 << 10, 32, 512), True, "the 1x1 GEMM has no per-image range"),
    ((3, 64, 1 << 9, 1 << 9, 32, 64), True, "batches run in groups of images: only one image has to fit"),
]


@pytest.mark.parametrize("i", range(len(LAYERS)))
def test_bf16_layer_ok(i):
    args, want, why = LAYERS[i]
    assert train_conv.bf16_layer_ok(*args) is want, why


def test_the_context_takes_bf16_or_none_only():
    with train_conv.mfma_dtype(None) as m:
        assert m.launches == 0 and train_conv._MFMA is None
    with train_conv.mfma_dtype(torch.bfloat16) as m:
        assert train_conv._MFMA is m
        with train_conv.mfma_dtype(None):
            assert train_conv._MFMA is None
        assert train_conv._MFMA is m
    assert train_conv._MFMA is None
    for bad in (torch.float16, torch.float32, "bf16"):
        with pytest.raises(ValueError):
            train_conv.mfma_dtype(bad)
