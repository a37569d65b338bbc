"""Argument checks of the six entry points of the bf16-product family (csrc/gemm_bf16.hip; no GPU): they go through the shared host
front (csrc/gemm_host.hpp), so a defective call is answered with the same code, in the same order of checks, as
tests/test_dense_gemm_args.py expects of the split family: size errors, the empty batch, null pointers, shape / alignment, 32-bit
ranges, workspace.

Every pointer is a fake address, so no row expects a launch: each call is either rejected or an empty batch, and the module skips
itself where a GPU is present (there a call that passes the checks would hand the fake address to a kernel)."""
import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
P = 0x10000                           # 16-byte aligned, never dereferenced
FAMILIES = ("_split", "_bf16")        # the yardstick beside the family under test: every row must hold for both
FORMS_1X1 = ("plain", "topdown", "pooled")
ALL = FORMS_1X1 + ("conv",)

BASE = dict(x=P, M=256, N=2, H=8, W=16, HW=200, K=64, x_ld=64, Wp=P, Cout=32, top=P, Ht=4, Wt=8, top_ld=32, y=P, y_ld=32, mean=P, ws=P,
            ws_bytes=1 << 40, kh=3, kw=3, stride=2, pad=1)


@pytest.fixture(scope="module", autouse=True)
def L():
    lib = _lib.lib()
    if lib.srf_device_count() > 0:
        pytest.skip("a GPU is present: a fake address must never reach a kernel")
    return lib


def call(L, form, family, **kw):
    a = dict(BASE, **kw)
    if form == "plain":
        return getattr(L, "srf_conv1x1_nhwc" + family)(a["x"], a["M"], a["K"], a["x_ld"], a["Wp"], a["Cout"], None, None, 0, a["y"], a["y_ld"],
                                                        None)
    if form == "topdown":
        return getattr(L, f"srf_conv1x1_nhwc{family}_topdown")(a["x"], a["N"], a["H"], a["W"], a["K"], a["x_ld"], a["Wp"], a["Cout"], None, None, 0,
                                                                a["top"], a["Ht"], a["Wt"], a["top_ld"], a["y"], a["y_ld"], None)
    if form == "pooled":
        return getattr(L, f"srf_conv1x1_nhwc{family}_pooled")(a["x"], a["N"], a["HW"], a["K"], a["x_ld"], a["Wp"], a["Cout"], None, None, 0,
                                                               a["y"], a["y_ld"], a["mean"], a["ws"], a["ws_bytes"], None)
    assert form == "conv"
    return getattr(L, "srf_conv_gemm_nhwc" + family)(a["x"], a["N"], a["H"], a["W"], a["K"], a["x_ld"], a["Wp"], a["Cout"], a["kh"], a["kw"],
                                                      a["stride"], a["pad"], None, None, 0, a["y"], a["y_ld"], None)


# (forms, arguments that differ from BASE, expected code); K is Cin for the conv form -- the rows of tests/test_dense_gemm_args.py
SINGLE = [
    # 1. sizes
    (("plain",), dict(M=-1), EINVAL),
    (("topdown", "pooled", "conv"), dict(N=-1), EINVAL),
    (ALL, dict(K=0), EINVAL),
    (ALL, dict(Cout=0), EINVAL),
    (("pooled",), dict(HW=0), EINVAL),
    (("topdown", "conv"), dict(H=0), EINVAL),
    (("topdown", "conv"), dict(W=0), EINVAL),
    (("topdown",), dict(Ht=0), EINVAL),
    (("topdown",), dict(Wt=0), EINVAL),
    (("conv",), dict(kh=0), EINVAL),
    (("conv",), dict(kw=0), EINVAL),
    (("conv",), dict(stride=0), EINVAL),
    (("conv",), dict(pad=-1), EINVAL),
    (ALL, dict(x_ld=60), EINVAL),
    (ALL, dict(y_ld=28), EINVAL),
    (("topdown",), dict(top_ld=28), EINVAL),
    # 2. an empty batch that is otherwise valid
    (("plain",), dict(M=0), OK),
    (("topdown", "pooled", "conv"), dict(N=0), OK),
    # 3. each required pointer null in turn
    (ALL, dict(x=None), EINVAL),
    (ALL, dict(Wp=None), EINVAL),
    (ALL, dict(y=None), EINVAL),
    (("topdown",), dict(top=None), EINVAL),
    (("pooled",), dict(mean=None), EINVAL),
    (("pooled",), dict(ws=None), EINVAL),
    # 4. shape and alignment
    (ALL, dict(K=48, x_ld=48), EUNSUPPORTED),
    (ALL, dict(x_ld=66), EUNSUPPORTED),
    (ALL, dict(x=P + 4), EUNSUPPORTED),
    (ALL, dict(Wp=P + 4), EUNSUPPORTED),
    (("pooled",), dict(N=65536), EUNSUPPORTED),
    # 5. ranges
    (("topdown",), dict(N=2, Ht=1024, Wt=1024, top_ld=1024), EUNSUPPORTED),
    (("conv",), dict(N=64, H=512, W=512, K=32, x_ld=32), EUNSUPPORTED),     # 2 GiB of input
    (("conv",), dict(H=2, W=2, pad=0, stride=1), EINVAL),                   # no output pixel
    (("conv",), dict(H=2, W=2, pad=0, stride=2), EINVAL),                   # the same where C's division gives (2 - 3) / 2 + 1 = 1
    (("conv",), dict(kh=1, kw=19, stride=3), EINVAL),                       # a 1 x 19 kernel on a padded width of 18
    (FORMS_1X1, dict(x_ld=1 << 22), EUNSUPPORTED),                          # x_ld * 128 rows * 4 bytes reaches 2^31
    (ALL, dict(y_ld=1 << 22), EUNSUPPORTED),                                # y is written through a descriptor of one 128-row tile
    # 6. two defects at once: the earlier check of the common order answers
    (("plain",), dict(M=0, x=P + 4), OK),
    (("topdown", "pooled", "conv"), dict(N=0, x=P + 4), OK),
    (("plain",), dict(M=0, K=48, x_ld=48), OK),
    (ALL, dict(x=None, K=48, x_ld=48), EINVAL),
    (ALL, dict(y=None, x_ld=66), EINVAL),
    (("topdown",), dict(top=None, N=2, Ht=1024, Wt=1024, top_ld=1024), EINVAL),
    (("pooled",), dict(ws=None, N=65536), EINVAL),
    (("pooled",), dict(K=48, x_ld=48, ws_bytes=0), EUNSUPPORTED),
    (ALL, dict(Cout=0, x=None), EINVAL),
]


@pytest.mark.parametrize("row", range(len(SINGLE)))
def test_a_defective_call_gets_the_split_familys_code(L, row):
    forms, kw, want = SINGLE[row]
    for form in forms:
        for fam in FAMILIES:
            assert call(L, form, fam, **kw) == want, (form, fam, kw)


def test_workspace_one_byte_below_the_bound(L):
    """N * ceil(HW / 128) * Cout * 4 bytes, as the split family; srf_conv1x1_nhwc_pooled_workspace_bytes (blocks of 64 rows) covers it."""
    N, HW, Cout = BASE["N"], BASE["HW"], BASE["Cout"]
    need = N * -(-HW // 128) * Cout * 4
    assert L.srf_conv1x1_nhwc_pooled_workspace_bytes(N, HW, Cout) >= need
    for fam in FAMILIES:
        assert call(L, "pooled", fam, ws_bytes=need - 1) == EWORKSPACE, fam
        assert call(L, "pooled", fam, ws_bytes=0) == EWORKSPACE, fam


def test_packed_weight_size_and_pack_arguments(L):
    """One bf16 plane in blocks of 64 channels x 128 output channels: 2 bytes per weight of the padded (ceil(Cout / 128) 128, ceil(K / 64) 64)
    matrix; K % 32 != 0 has no packed form (0 bytes; SRF_EUNSUPPORTED from the pack call, after the null / size checks)."""
    size = L.srf_conv1x1_nhwc_bf16_packed_weight_bytes
    assert size(128, 64) == 128 * 64 * 2
    assert size(200, 96) == 256 * 128 * 2
    assert size(40, 32) == 128 * 64 * 2
    assert size(1024, 2144) == 1024 * 2176 * 2
    assert size(128, 48) == 0 and size(0, 64) == 0 and size(128, 0) == 0 and size(-1, 64) == 0
    assert size(768, 1728) * 3 == L.srf_conv1x1_nhwc_split_packed_weight_bytes(768, 1728)      # a third of the split's three planes (K % 64 == 0)
    for fam in FAMILIES:
        pack = getattr(L, f"srf_conv1x1_nhwc{fam}_pack_weights")
        assert pack(None, 128, 64, P, None) == EINVAL
        assert pack(P, 128, 64, None, None) == EINVAL
        assert pack(P, 0, 64, P, None) == EINVAL
        assert pack(P, 128, 0, P, None) == EINVAL
        assert pack(P, 128, 48, P, None) == EUNSUPPORTED
        assert pack(None, 128, 48, P, None) == EINVAL                  # null pointer before K % 32
