"""Argument checks of srf_conv_wgrad_nhwc_bf16 (csrc/wgrad_bf16.hip), the mode's layer limits (train_conv.bf16_layer_ok,
ops.gemm_bf16_why_not) and the context class the three bf16-product modes share (srfdet3d_amd/mfma_mode.py); no GPU.

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
        assert m.launches == 0 and train_conv.mfma_dtype.active() is None
    with train_conv.mfma_dtype(torch.bfloat16) as m:
        assert train_conv.mfma_dtype.active() is m
        with train_conv.mfma_dtype(None):
            assert train_conv.mfma_dtype.active() is None
        assert train_conv.mfma_dtype.active() is m
    assert train_conv.mfma_dtype.active() is None
    for bad in (torch.float16, torch.float32, "bf16"):
        with pytest.raises(ValueError):
            train_conv.mfma_dtype(bad)


def test_the_three_modes_share_one_base_and_stay_independent():
    from srfdet3d_amd import mfma_mode, nhwc, sparse
    kinds = (nhwc.mfma_dtype, sparse.mfma_dtype, train_conv.mfma_dtype)
    assert all(issubclass(k, mfma_mode.MfmaMode) and k.active() is None for k in kinds)
    for kind, name in zip(kinds, ("nhwc", "sparse", "train_conv")):
        with pytest.raises(ValueError, match=f"^{name}.mfma_dtype: only torch.bfloat16"):
            kind(torch.float16)
    ri, rt = [], []
    with nhwc.mfma_dtype(torch.bfloat16, routes=ri) as a:
        assert (nhwc.mfma_dtype.active(), sparse.mfma_dtype.active(), train_conv.mfma_dtype.active()) == (a, None, None)
        with sparse.mfma_dtype(torch.bfloat16) as b, train_conv.mfma_dtype(torch.bfloat16, routes=rt) as c:
            assert (nhwc.mfma_dtype.active(), sparse.mfma_dtype.active(), train_conv.mfma_dtype.active()) == (a, b, c)
            assert nhwc.mfma_active() and sparse.mfma_active()
            with sparse.mfma_dtype(None) as off:                     # hides its own kind only
                assert (nhwc.mfma_dtype.active(), sparse.mfma_dtype.active(), train_conv.mfma_dtype.active()) == (a, None, c)
                assert not sparse.mfma_active()
            assert sparse.mfma_dtype.active() is b
            # the report: a falsy reason is the bf16 route and counts, any other is the f32 route with that reason
            assert a.report("L0", None) is True and a.report("L1", "") is True and a.report("L2", "operand alignment") is False
            assert c.report("L3", None, direction="fwd") is True and c.report("L3", "no", direction="dgrad") is False
            b.report("L4", None)                                     # no list given: counted all the same
            with pytest.raises(KeyError):
                with train_conv.mfma_dtype(None):
                    assert train_conv.mfma_dtype.active() is None
                    raise KeyError("inside")
            assert train_conv.mfma_dtype.active() is c               # ... the exit under an exception restored the outer one
        assert (sparse.mfma_dtype.active(), train_conv.mfma_dtype.active()) == (None, None)
    assert all(k.active() is None for k in kinds)
    assert (a.launches, b.launches, c.launches, off.launches) == (2, 1, 1, 0)
    assert ri == [dict(layer="L0", route="bf16", why=None), dict(layer="L1", route="bf16", why=""), dict(layer="L2", route="f32", why="operand alignment")]
    assert rt == [dict(layer="L3", direction="fwd", route="bf16", why=None), dict(layer="L3", direction="dgrad", route="f32", why="no")]
    assert [list(r) for r in ri + rt] == [["layer", "route", "why"]] * 3 + [["layer", "direction", "route", "why"]] * 2     # the key order
    a.require_launches("unused")
    for asked, what in ((nhwc.mfma_dtype(torch.bfloat16), RuntimeError), (nhwc.mfma_dtype(None), None)):
        with asked:
            pass
        if what is None:
            asked.require_launches("a mode that was not asked for requires nothing")
        else:
            with pytest.raises(what, match="nothing ran"):
                asked.require_launches("nothing ran")


class _Dense:
    """What `ops.gemm_bf16_why_not` reads of a dense channels-last (N, H, W, C) f32 tensor at an aligned address, without its storage."""
    dtype = torch.float32

    def __init__(self, N, H, W, C):
        self.shape = (N, H, W, C)

    dim = lambda self: 4
    data_ptr = lambda self: P

    def stride(self, i):
        N, H, W, C = self.shape
        return (H * W * C, W * C, C, 1)[i]


@pytest.mark.parametrize("i", [i for i, (args, _, _) in enumerate(LAYERS) if args[0] in (1, 3)])
def test_gemm_bf16_why_not_agrees_with_bf16_layer_ok_on_dense_tensors(i, monkeypatch):
    import make_nhwc_calls
    from srfdet3d_amd import ops
    (k, N, H, W, Cin, Cout), want, why = LAYERS[i]
    monkeypatch.setattr(ops, "nhwc_ld", make_nhwc_calls._ld)        # (`ops.nhwc_ld` without its device test)
    got = ops.gemm_bf16_why_not(_Dense(N, H, W, Cin), Cout, None, im2col=k == 3, dgrad=True)
    assert (got is None) is want, (why, got)
    assert got in (None, "input or output channels are no multiple of 32", "beyond the 32-bit ranges")
