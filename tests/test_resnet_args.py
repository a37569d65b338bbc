"""Argument checks of the five entry points the bottleneck ResNets added (no GPU): srf_stem_conv7_nchw (the codes and the refusal order
of srf_stem_conv_nchw), srf_nhwc_maxpool3s2_pad1 (those of srf_nhwc_maxpool3s2_ceil) and the residual form of the three f32-accurate
GEMM families (csrc/gemm_host.hpp: size errors, the empty batch, null pointers, shape / alignment, 32-bit ranges).

Every pointer is a fake address, so no row expects a launch: each call is either rejected or an empty batch, and the module skips
itself where a GPU is present (there a call that passes the checks would hand the fake address to a kernel)."""
import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
P = 0x10000                           # 16-byte aligned, never dereferenced
FAMILIES = ("", "_direct", "_split")
TILE = {"": 256, "_direct": 128, "_split": 128}     # rows of the tile the 32-bit range limits are stated for

ENTRY = {
    "stem7": ("x N Cin H W Wt Cout scale shift relu y y_ld", dict(x=P, N=2, Cin=3, H=11, W=13, Wt=P, Cout=64, scale=P, shift=P, relu=1, y=P, y_ld=64)),
    "stem3": ("x N Cin H W Wt Cout scale shift relu y y_ld", dict(x=P, N=2, Cin=3, H=11, W=13, Wt=P, Cout=64, scale=P, shift=P, relu=1, y=P, y_ld=64)),
    "pool_p1": ("x x_ld N H W C y y_ld", dict(x=P, x_ld=16, N=2, H=5, W=4, C=8, y=P, y_ld=16)),
    "pool_ceil": ("x x_ld N H W C y y_ld", dict(x=P, x_ld=16, N=2, H=5, W=4, C=8, y=P, y_ld=16)),
}
RES = ("x M K x_ld Wp Cout scale shift relu y y_ld res res_ld",
       dict(x=P, M=256, K=64, x_ld=64, Wp=P, Cout=32, scale=None, shift=None, relu=1, y=P, y_ld=32, res=P, res_ld=32))
for _f in FAMILIES:
    ENTRY["res" + _f] = RES
SYMBOL = {"stem7": "srf_stem_conv7_nchw", "stem3": "srf_stem_conv_nchw", "pool_p1": "srf_nhwc_maxpool3s2_pad1", "pool_ceil": "srf_nhwc_maxpool3s2_ceil",
          "res": "srf_conv1x1_nhwc_residual", "res_direct": "srf_conv1x1_nhwc_direct_residual", "res_split": "srf_conv1x1_nhwc_split_residual"}
STEMS, POOLS, RESIDUALS = ("stem7", "stem3"), ("pool_p1", "pool_ceil"), ("res", "res_direct", "res_split")
# the two older entry points ride along: the new ones answer as they do, row for row


@pytest.fixture(scope="module", autouse=True)
def L():
    lib = _lib.lib()
    if lib.srf_device_count() > 0:
        pytest.skip("a GPU is present: a fake address must never reach a kernel")
    return lib


def call(L, entry, **kw):
    names, base = ENTRY[entry]
    a = dict(base, **kw)
    assert set(a) == set(base), (entry, set(a) - set(base))
    return getattr(L, SYMBOL[entry])(*[a[n] for n in names.split()], None)


# (entry points, arguments that differ from the passing call, expected code)
TABLE = [
    # 1. sizes
    (STEMS + POOLS, dict(N=-1), EINVAL),
    (RESIDUALS, dict(M=-1), EINVAL),
    (STEMS, dict(Cin=0), EINVAL),
    (STEMS, dict(Cin=-1), EINVAL),
    (STEMS + POOLS, dict(H=0), EINVAL),
    (STEMS + POOLS, dict(W=0), EINVAL),
    (STEMS + POOLS, dict(H=-1), EINVAL),
    (STEMS, dict(y_ld=60), EINVAL),
    (POOLS, dict(C=0), EINVAL),
    (POOLS, dict(C=-1), EINVAL),
    (POOLS, dict(x_ld=4), EINVAL),
    (POOLS, dict(y_ld=4), EINVAL),
    (RESIDUALS, dict(K=0), EINVAL),
    (RESIDUALS, dict(Cout=0), EINVAL),
    (RESIDUALS, dict(x_ld=60), EINVAL),
    (RESIDUALS, dict(y_ld=28), EINVAL),
    (RESIDUALS, dict(res_ld=28), EINVAL),                # res_ld < Cout
    (RESIDUALS, dict(res_ld=0), EINVAL),
    # 2. the empty batch
    (STEMS + POOLS, dict(N=0), OK),
    (RESIDUALS, dict(M=0), OK),
    # 3. each required pointer null in turn
    (STEMS + POOLS, dict(x=None), EINVAL),
    (STEMS + POOLS, dict(y=None), EINVAL),
    (STEMS, dict(Wt=None), EINVAL),
    (RESIDUALS, dict(x=None), EINVAL),
    (RESIDUALS, dict(Wp=None), EINVAL),
    (RESIDUALS, dict(y=None), EINVAL),
    (RESIDUALS, dict(res=None), EINVAL),
    (STEMS, dict(scale=None, shift=None, N=0), OK),      # optional operands: absent is fine as far as the checks go
    (STEMS, dict(scale=None, shift=None, y=None), EINVAL),
    # 4. shape and alignment
    (STEMS, dict(Cin=5), EUNSUPPORTED),
    (STEMS, dict(Cout=32, y_ld=32), EUNSUPPORTED),
    (STEMS, dict(Cout=128, y_ld=128), EUNSUPPORTED),
    (STEMS, dict(y_ld=66), EUNSUPPORTED),
    (STEMS, dict(y=P + 4), EUNSUPPORTED),
    (POOLS, dict(C=6), EUNSUPPORTED),
    (POOLS, dict(x_ld=18), EUNSUPPORTED),
    (POOLS, dict(y_ld=18), EUNSUPPORTED),
    (POOLS, dict(x=P + 4), EUNSUPPORTED),
    (POOLS, dict(y=P + 4), EUNSUPPORTED),
    (RESIDUALS, dict(K=48, x_ld=48), EUNSUPPORTED),
    (RESIDUALS, dict(x_ld=66), EUNSUPPORTED),
    (RESIDUALS, dict(x=P + 4), EUNSUPPORTED),
    (RESIDUALS, dict(Wp=P + 4), EUNSUPPORTED),
    (RESIDUALS, dict(res_ld=34), EUNSUPPORTED),          # not in whole float4s
    (RESIDUALS, dict(res=P + 4), EUNSUPPORTED),
    (RESIDUALS, dict(res=P + 8), EUNSUPPORTED),
    # 5. ranges
    (STEMS, dict(H=4096, W=4096, y_ld=128), EUNSUPPORTED),     # one image's output: 2048 x 2048 x 128 x 4 = 2^31 bytes
]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_one_defect(L, row):
    entries, kw, want = TABLE[row]
    for e in entries:
        assert call(L, e, **kw) == want, (e, kw)


def test_the_stem_checks_its_range_last(L):
    """One image's output of 2^31 bytes (4096 x 4096 images, y_ld = 128): the empty batch and a null pointer answer first."""
    for e in STEMS:
        assert call(L, e, H=4096, W=4096, y_ld=128, N=0) == OK
        assert call(L, e, H=4096, W=4096, y_ld=128, x=None) == EINVAL


def test_first_res_ld_at_the_range_limit_of_each_family(L):
    """res is read through a descriptor over the rows of one tile: res_ld * tile rows * 4 bytes reaches 2^31 at res_ld = 2^21 in the LDS
    family (256 rows) and 2^22 in the other two (128 rows); one float4 less passes."""
    for fam in FAMILIES:
        first = (1 << 29) // TILE[fam]
        assert call(L, "res" + fam, res_ld=first) == EUNSUPPORTED, fam
        assert call(L, "res" + fam, res_ld=first - 4, M=0) == OK, fam
        # ... and it is a range like the others: x_ld and (direct, split) y_ld at theirs
        assert call(L, "res" + fam, x_ld=first) == EUNSUPPORTED, fam
    for fam in ("_direct", "_split"):
        assert call(L, "res" + fam, y_ld=1 << 22) == EUNSUPPORTED, fam


# two defects at once: the earlier check answers
ORDER = [
    (RESIDUALS, dict(M=0, res=None), OK),                                # an empty batch is nothing to do, whatever else is wrong
    (RESIDUALS, dict(M=0, res=P + 4, res_ld=34), OK),
    (RESIDUALS, dict(M=0, res_ld=28), EINVAL),                           # a size error even in an empty batch
    (RESIDUALS, dict(res=None, res_ld=34), EINVAL),                      # null pointer before res_ld % 4
    (RESIDUALS, dict(res=None, K=48, x_ld=48), EINVAL),
    (RESIDUALS, dict(x=None, res=P + 4), EINVAL),
    (RESIDUALS, dict(res_ld=28, x=P + 4), EINVAL),                       # size before alignment
    (RESIDUALS, dict(res=None, res_ld=1 << 22), EINVAL),                 # null pointer before the range
    (STEMS, dict(N=-1, Cin=5), EINVAL),                                  # size before shape
    (STEMS, dict(Cin=5, N=0), EUNSUPPORTED),                             # shape before the empty batch (the order of srf_stem_conv_nchw)
    (STEMS, dict(Cin=5, x=None), EUNSUPPORTED),                          # ... and before the pointers
    (STEMS, dict(N=0, x=None), OK),
    (POOLS, dict(N=-1, C=6), EINVAL),
    (POOLS, dict(N=0, C=6), OK),                                         # the empty batch before everything but the sizes
    (POOLS, dict(N=0, x=None), OK),
    (POOLS, dict(N=0, C=0), EINVAL),
    (POOLS, dict(y=None, x=P + 4), EINVAL),                              # null pointer before alignment
    (POOLS, dict(x=None, C=6), EINVAL),
]


@pytest.mark.parametrize("row", range(len(ORDER)))
def test_two_defects_are_answered_in_the_stated_order(L, row):
    entries, kw, want = ORDER[row]
    for e in entries:
        assert call(L, e, **kw) == want, (e, kw)
