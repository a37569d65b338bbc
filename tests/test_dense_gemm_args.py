"""Argument checks of the eleven dense-GEMM entry points (no GPU): the LDS-staged, the LDS-free and the bf16-split family answer a
defective call with the same code, in the same order of checks (csrc/gemm_host.hpp): size errors, the empty batch, null pointers,
shape / alignment, 32-bit ranges, workspace.

Every pointer is a fake address, so no row expects a launch: each call is either rejected or an empty batch, and the module skips
itself where a GPU is present (there a call that passes the checks would hand the fake address to a kernel)."""
import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
P = 0x10000                           # 16-byte aligned, never dereferenced
FAMILIES = ("", "_direct", "_split")
FORMS_1X1 = ("plain", "topdown", "pooled")
TILE = {"": 256, "_direct": 128, "_split": 128}     # rows of the tile the 32-bit range limits are stated for
POOL_ROWS = {"": 64, "_direct": 128, "_split": 128}  # rows per workspace block of the pooled form

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
    assert form == "conv" and family in ("", "_split")
    return getattr(L, "srf_conv_gemm_nhwc" + family)(a["x"], a["N"], a["H"], a["W"], a["K"], a["x_ld"], a["Wp"], a["Cout"], a["kh"], a["kw"],
                                                      a["stride"], a["pad"], None, None, 0, a["y"], a["y_ld"], None)


def entry_points(forms):
    return [(form, fam) for form in forms for fam in FAMILIES if form != "conv" or fam != "_direct"]


ALL = FORMS_1X1 + ("conv",)
# (forms, arguments that differ from BASE, expected code); K is Cin for the conv forms
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
    # 5. ranges (the x_ld / y_ld / workspace rows, which differ per family, follow in the tests below)
    (("topdown",), dict(N=2, Ht=1024, Wt=1024, top_ld=1024), EUNSUPPORTED),
    (("conv",), dict(N=64, H=512, W=512, K=32, x_ld=32), EUNSUPPORTED),     # 2 GiB of input
    (("conv",), dict(H=2, W=2, pad=0, stride=1), EINVAL),                   # no output pixel
    (("conv",), dict(H=2, W=2, pad=0, stride=2), EINVAL),                   # the same where C's division gives (2 - 3) / 2 + 1 = 1
    (("conv",), dict(kh=1, kw=19, stride=3), EINVAL),                       # a 1 x 19 kernel on a padded width of 18
]


@pytest.mark.parametrize("row", range(len(SINGLE)))
def test_one_defect_gives_the_same_code_in_every_family(L, row):
    forms, kw, want = SINGLE[row]
    for form, fam in entry_points(forms):
        assert call(L, form, fam, **kw) == want, (form, fam, kw)


def test_first_x_ld_at_the_range_limit_of_each_family(L):
    """x_ld * tile rows * 4 bytes reaches 2^31: 256 rows in the LDS family (x_ld = 2^21), 128 in the other two (2^22)."""
    for form, fam in entry_points(FORMS_1X1):
        assert call(L, form, fam, x_ld=(1 << 29) // TILE[fam]) == EUNSUPPORTED, (form, fam)


def test_first_y_ld_at_the_range_limit(L):
    """y_ld * 128 * 4 reaches 2^31 in the direct, split and conv-split forms (the LDS family states no limit on y_ld)."""
    for form, fam in [(f, m) for f in FORMS_1X1 for m in ("_direct", "_split")] + [("conv", "_split")]:
        assert call(L, form, fam, y_ld=1 << 22) == EUNSUPPORTED, (form, fam)


def test_conv_reduction_length_past_the_int_range(L):
    """kh * kw * Cin is the K of the implicit im2col and an int in the kernels' arguments: 64 * 64 * 2^20 = 2^32 is refused by the split
    and the bf16-product form (one shared body, csrc/gemm_tile128.hpp `srf_tile128_conv`), after every check of `srf_gemm_check_conv`
    has passed (4 MiB of input, 2 x 2 output pixels); one tap less in each direction of a 2^19-channel input (63 * 63 * 2^19 < 2^31)
    is not what this row refuses, and a null pointer is still answered first."""
    big = dict(N=1, H=1, W=1, K=1 << 20, x_ld=1 << 20, kh=64, kw=64, stride=1, pad=32)
    a = dict(BASE, **big)
    for name in ("srf_conv_gemm_nhwc_split", "srf_conv_gemm_nhwc_bf16"):
        fn = getattr(L, name)
        args = lambda a: (a["x"], a["N"], a["H"], a["W"], a["K"], a["x_ld"], a["Wp"], a["Cout"], a["kh"], a["kw"], a["stride"], a["pad"],  # noqa: E731
                          None, None, 0, a["y"], a["y_ld"], None)
        assert fn(*args(a)) == EUNSUPPORTED, name
        assert fn(*args(dict(a, x=None))) == EINVAL, name
        assert fn(*args(dict(a, N=0))) == OK, name


def test_workspace_one_byte_below_the_bound_of_each_family(L):
    """N * ceil(HW / block rows) * Cout * 4 bytes: blocks of 64 rows in the LDS family (srf_conv1x1_nhwc_pooled_workspace_bytes),
    of 128 in the other two."""
    N, HW, Cout = BASE["N"], BASE["HW"], BASE["Cout"]
    assert L.srf_conv1x1_nhwc_pooled_workspace_bytes(N, HW, Cout) == N * 4 * Cout * 4
    for fam in FAMILIES:
        need = N * -(-HW // POOL_ROWS[fam]) * Cout * 4
        assert call(L, "pooled", fam, ws_bytes=need - 1) == EWORKSPACE, fam
        assert call(L, "pooled", fam, ws_bytes=0) == EWORKSPACE, fam


# two defects at once: the earlier check of the common order answers
DOUBLE = [
    (("plain",), dict(M=0, x=P + 4), OK),                                 # an empty batch is nothing to do, whatever else is wrong
    (("topdown", "pooled", "conv"), dict(N=0, x=P + 4), OK),
    (("plain",), dict(M=0, K=48, x_ld=48), OK),
    (ALL, dict(x=None, K=48, x_ld=48), EINVAL),                           # null pointer before K % 32
    (ALL, dict(y=None, x_ld=66), EINVAL),
    (("topdown",), dict(top=None, N=2, Ht=1024, Wt=1024, top_ld=1024), EINVAL),
    (("pooled",), dict(ws=None, N=65536), EINVAL),
    (("pooled",), dict(K=48, x_ld=48, ws_bytes=0), EUNSUPPORTED),         # shape before workspace
    (ALL, dict(Cout=0, x=None), EINVAL),
]


@pytest.mark.parametrize("row", range(len(DOUBLE)))
def test_two_defects_are_answered_in_the_common_order(L, row):
    forms, kw, want = DOUBLE[row]
    for form, fam in entry_points(forms):
        assert call(L, form, fam, **kw) == want, (form, fam, kw)
