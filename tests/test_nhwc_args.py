"""Argument checks of the entry points of csrc/nhwc.hip (no GPU): one table of defective calls and the code each is answered with,
in the order of checks the file's header states: sizes (SRF_EINVAL), the empty batch (SRF_OK), null pointers (SRF_EINVAL), C % 4 /
ld % 4 / alignment / range limits (SRF_EUNSUPPORTED), workspace size (SRF_EWORKSPACE).

Every pointer is a fake address, so no row expects a launch: each call is either rejected or an empty batch, and the module skips
itself where a GPU is present (there a call that passes the checks would hand the fake address to a kernel).  The empty batch of
srf_nhwc_affine_relu_bwd*, which zeroes `sums`, is therefore a GPU test (tests/test_gpu_nhwc_layers.py)."""
import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
P = 0x10000                           # 16-byte aligned, never dereferenced
BIG = 1 << 40

# entry point -> (argument names in ABI order, a call that passes every check)
ENTRY = {
    "affine": ("x x_ld N HW C scale per_sample shift residual r_ld relu y y_ld",
               dict(x=P, x_ld=16, N=2, HW=6, C=8, scale=P, per_sample=0, shift=P, residual=P, r_ld=16, relu=1, y=P, y_ld=16)),
    "colmean": ("x x_ld N HW C mean ws ws_bytes", dict(x=P, x_ld=16, N=2, HW=6, C=8, mean=P, ws=P, ws_bytes=BIG)),
    "colsum_prod": ("a a_ld b b_ld N HW C out ws ws_bytes", dict(a=P, a_ld=16, b=P, b_ld=12, N=2, HW=6, C=8, out=P, ws=P, ws_bytes=BIG)),
    "maxpool3s2_ceil": ("x x_ld N H W C y y_ld", dict(x=P, x_ld=16, N=2, H=5, W=4, C=8, y=P, y_ld=16)),
    "upsample_add": ("lat l_ld top t_ld N H W Ht Wt C y y_ld",
                     dict(lat=P, l_ld=16, top=P, t_ld=16, N=2, H=5, W=4, Ht=3, Wt=2, C=8, y=P, y_ld=16)),
    "dwconv3x3s2": ("x x_ld N H W C w scale shift relu y y_ld",
                    dict(x=P, x_ld=16, N=2, H=5, W=4, C=8, w=P, scale=P, shift=P, relu=1, y=P, y_ld=16)),
    "dwconv3x3s2_cat": ("x x_ld N H W C w scale shift relu y y_ld side side_ld Cs side_out",
                        dict(x=P, x_ld=16, N=2, H=5, W=4, C=8, w=P, scale=P, shift=P, relu=1, y=P, y_ld=16, side=P, side_ld=8, Cs=8,
                             side_out=P)),
    "pool_sum": ("x x_ld B n_cam H W C Ho Wo out out_ld", dict(x=P, x_ld=16, B=2, n_cam=3, H=5, W=4, C=8, Ho=3, Wo=3, out=P, out_ld=12)),
    "affine_relu_bwd": ("gy gy_ld y y_ld M C scale relu gz gz_ld sums ws ws_bytes",
                        dict(gy=P, gy_ld=16, y=P, y_ld=16, M=300, C=8, scale=P, relu=1, gz=P, gz_ld=16, sums=P, ws=P, ws_bytes=BIG)),
    "affine_relu_bwd2": ("gy gy_ld gy2 gy2_ld y y_ld M C scale relu gz gz_ld sums ws ws_bytes",
                         dict(gy=P, gy_ld=16, gy2=P, gy2_ld=16, y=P, y_ld=16, M=300, C=8, scale=P, relu=1, gz=P, gz_ld=16, sums=P, ws=P,
                              ws_bytes=BIG)),
    "bn_eval_fold": ("gamma beta mean var eps C out", dict(gamma=P, beta=P, mean=P, var=P, eps=1e-5, C=8, out=P)),
    "bn_eval_grads": ("sums fold mean C out", dict(sums=P, fold=P, mean=P, C=8, out=P)),
}
SYMBOL = {k: ("srf_" if k.startswith("bn_") else "srf_nhwc_") + k for k in ENTRY}
MAPS = ("maxpool3s2_ceil", "upsample_add", "dwconv3x3s2", "dwconv3x3s2_cat")      # (N, H, W) entry points
DW = ("dwconv3x3s2", "dwconv3x3s2_cat")
COLS = ("colmean", "colsum_prod")
BWD = ("affine_relu_bwd", "affine_relu_bwd2")
BN = ("bn_eval_fold", "bn_eval_grads")
NHW = ("affine",) + COLS + MAPS                                                   # those with a batch count N


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
    # 1. sizes: each at -1 and at 0
    (NHW, dict(N=-1), EINVAL),
    (BWD, dict(M=-1), EINVAL),
    (("pool_sum",), dict(B=-1), EINVAL),
    (tuple(ENTRY), dict(C=0), EINVAL),
    (tuple(ENTRY), dict(C=-1), EINVAL),
    (("affine",) + COLS, dict(HW=-1), EINVAL),
    (("affine",), dict(HW=0), OK),                       # an empty tensor: nothing to do
    (COLS, dict(HW=0), EINVAL),                          # the mean / sum over no pixels of N > 0 images
    (MAPS + ("pool_sum",), dict(H=0), EINVAL),
    (MAPS + ("pool_sum",), dict(H=-1), EINVAL),
    (MAPS + ("pool_sum",), dict(W=0), EINVAL),
    (MAPS + ("pool_sum",), dict(W=-1), EINVAL),
    (("upsample_add",), dict(Ht=0), EINVAL),
    (("upsample_add",), dict(Ht=-1), EINVAL),
    (("upsample_add",), dict(Wt=0), EINVAL),
    (("upsample_add",), dict(Wt=-1), EINVAL),
    (("pool_sum",), dict(Ho=0), EINVAL),
    (("pool_sum",), dict(Ho=-1), EINVAL),
    (("pool_sum",), dict(Wo=0), EINVAL),
    (("pool_sum",), dict(Wo=-1), EINVAL),
    (("pool_sum",), dict(n_cam=0), EINVAL),
    (("pool_sum",), dict(n_cam=-1), EINVAL),
    (("dwconv3x3s2_cat",), dict(Cs=0), EINVAL),
    (("dwconv3x3s2_cat",), dict(Cs=-1), EINVAL),
    # ... each ld below its C
    (("affine", "colmean", "pool_sum") + MAPS[:1] + DW, dict(x_ld=4), EINVAL),
    (("affine",) + MAPS, dict(y_ld=4), EINVAL),
    (("affine",), dict(r_ld=4), EINVAL),
    (("colsum_prod",), dict(a_ld=4), EINVAL),
    (("colsum_prod",), dict(b_ld=4), EINVAL),
    (("upsample_add",), dict(l_ld=4), EINVAL),
    (("upsample_add",), dict(t_ld=4), EINVAL),
    (("dwconv3x3s2_cat",), dict(side_ld=4), EINVAL),
    (("dwconv3x3s2_cat",), dict(y_ld=12), EINVAL),       # y_ld < C + Cs: both slices lie in one row
    (("pool_sum",), dict(out_ld=8), EINVAL),             # out_ld < Ho * Wo
    (BWD, dict(gy_ld=4), EINVAL),
    (BWD, dict(y_ld=4), EINVAL),
    (BWD, dict(gz_ld=4), EINVAL),
    (("affine_relu_bwd2",), dict(gy2_ld=4), EINVAL),
    # 2. the empty batch
    (NHW, dict(N=0), OK),
    (("pool_sum",), dict(B=0), OK),
    (COLS, dict(N=0, HW=0), OK),                         # ... whatever the pixel count
    (("affine",), dict(N=0, HW=0), OK),
    # 3. each required pointer null in turn
    (("affine", "colmean", "pool_sum") + MAPS[:1] + DW, dict(x=None), EINVAL),
    (("affine",) + MAPS, dict(y=None), EINVAL),
    (("colmean",), dict(mean=None), EINVAL),
    (COLS + BWD, dict(ws=None), EINVAL),
    (("colsum_prod",), dict(a=None), EINVAL),
    (("colsum_prod",), dict(b=None), EINVAL),
    (("colsum_prod", "pool_sum", "bn_eval_fold", "bn_eval_grads"), dict(out=None), EINVAL),
    (("upsample_add",), dict(lat=None), EINVAL),
    (("upsample_add",), dict(top=None), EINVAL),
    (DW, dict(w=None), EINVAL),
    (("dwconv3x3s2_cat",), dict(side=None), EINVAL),
    (("dwconv3x3s2_cat",), dict(side_out=None), EINVAL),
    (BWD, dict(gy=None), EINVAL),
    (BWD, dict(y=None), EINVAL),
    (BWD, dict(gz=None), EINVAL),
    (BWD, dict(sums=None), EINVAL),
    (("bn_eval_fold",), dict(gamma=None), EINVAL),
    (("bn_eval_fold",), dict(beta=None), EINVAL),
    (("bn_eval_fold",), dict(var=None), EINVAL),
    (BN, dict(mean=None), EINVAL),
    (("bn_eval_grads",), dict(sums=None), EINVAL),
    (("bn_eval_grads",), dict(fold=None), EINVAL),
    # 4. C % 4, each ld not a multiple of 4, each vector-accessed pointer off by 4 bytes
    (tuple(k for k in ENTRY if k not in BN), dict(C=6), EUNSUPPORTED),
    (("dwconv3x3s2_cat",), dict(Cs=6), EUNSUPPORTED),
    (("affine", "colmean", "pool_sum") + MAPS[:1] + DW, dict(x_ld=18), EUNSUPPORTED),
    (("affine",) + MAPS, dict(y_ld=18), EUNSUPPORTED),
    (("affine",), dict(r_ld=18), EUNSUPPORTED),
    (("colsum_prod",), dict(a_ld=18), EUNSUPPORTED),
    (("colsum_prod",), dict(b_ld=18), EUNSUPPORTED),
    (("upsample_add",), dict(l_ld=18), EUNSUPPORTED),
    (("upsample_add",), dict(t_ld=18), EUNSUPPORTED),
    (("dwconv3x3s2_cat",), dict(side_ld=18), EUNSUPPORTED),
    (BWD, dict(gy_ld=18), EUNSUPPORTED),
    (BWD, dict(y_ld=18), EUNSUPPORTED),
    (BWD, dict(gz_ld=18), EUNSUPPORTED),
    (("affine_relu_bwd2",), dict(gy2_ld=18), EUNSUPPORTED),
    (("affine", "colmean", "pool_sum") + MAPS[:1] + DW, dict(x=P + 4), EUNSUPPORTED),
    (("affine",) + MAPS, dict(y=P + 4), EUNSUPPORTED),
    (("affine",), dict(residual=P + 4), EUNSUPPORTED),
    (("affine",), dict(scale=P + 4), EUNSUPPORTED),
    (("affine",), dict(shift=P + 4), EUNSUPPORTED),
    (COLS, dict(ws=P + 4), EUNSUPPORTED),                # the partial sums are stored as 16-byte vectors
    (COLS, dict(ws=P + 8), EUNSUPPORTED),
    (("colsum_prod",), dict(a=P + 4), EUNSUPPORTED),
    (("colsum_prod",), dict(b=P + 4), EUNSUPPORTED),
    (("upsample_add",), dict(lat=P + 4), EUNSUPPORTED),
    (("upsample_add",), dict(top=P + 4), EUNSUPPORTED),
    (("dwconv3x3s2_cat",), dict(side=P + 4), EUNSUPPORTED),
    (("dwconv3x3s2_cat",), dict(side_out=P + 4), EUNSUPPORTED),
    (BWD, dict(gy=P + 4), EUNSUPPORTED),
    (BWD, dict(y=P + 4), EUNSUPPORTED),
    (BWD, dict(gz=P + 4), EUNSUPPORTED),
    (BWD, dict(scale=P + 4), EUNSUPPORTED),
    (("affine_relu_bwd2",), dict(gy2=P + 4), EUNSUPPORTED),
    # ... range limits
    (COLS + BWD, dict(C=1028), EINVAL),                  # C above the limit with the ld's left behind is a size error; see WIDE
    (COLS, dict(N=65536), EUNSUPPORTED),
    # 5. workspace one byte short
    (COLS, dict(ws_bytes=2 * 64 * 8 * 4 - 1), EWORKSPACE),
    (COLS, dict(ws_bytes=0), EWORKSPACE),
    (BWD, dict(ws_bytes=2 * 2 * 8 * 4 - 1), EWORKSPACE),
    (BWD, dict(ws_bytes=0), EWORKSPACE),
    # optional operands: absent is fine as far as the checks go (the call then stops at a later defect)
    (("affine",), dict(residual=None, r_ld=0, y=None), EINVAL),
    (("affine",), dict(residual=None, r_ld=18, x=P + 4), EUNSUPPORTED),
    (("affine_relu_bwd2",), dict(gy2=None, gy2_ld=0, ws_bytes=0), EWORKSPACE),   # gy2_ld is ignored without gy2
    (("affine_relu_bwd2",), dict(gy2=None, gy2_ld=18, ws_bytes=0), EWORKSPACE),
    (BWD, dict(scale=None, ws_bytes=0), EWORKSPACE),
]
# C above the limit, the ld's following it
WIDE = [
    ("colmean", dict(C=1028, x_ld=1028), EUNSUPPORTED),                          # C / 4 > 256
    ("colsum_prod", dict(C=1028, a_ld=1028, b_ld=1028), EUNSUPPORTED),
    ("affine_relu_bwd", dict(C=1028, gy_ld=1028, y_ld=1028, gz_ld=1028), EUNSUPPORTED),
    ("affine_relu_bwd2", dict(C=1028, gy_ld=1028, gy2_ld=1028, y_ld=1028, gz_ld=1028), EUNSUPPORTED),
    ("colmean", dict(C=1024, x_ld=1024, ws_bytes=0), EWORKSPACE),                # 1024 itself passes the shape checks
    ("affine_relu_bwd", dict(C=1024, gy_ld=1024, y_ld=1024, gz_ld=1024, ws_bytes=0), EWORKSPACE),
]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_one_defect(L, row):
    entries, kw, want = TABLE[row]
    for e in entries:
        assert call(L, e, **kw) == want, (e, kw)


@pytest.mark.parametrize("row", range(len(WIDE)))
def test_channel_limit(L, row):
    e, kw, want = WIDE[row]
    assert call(L, e, **kw) == want, (e, kw)


def test_r_ld_without_a_residual_is_no_size_error(L):
    """r_ld below C, 0 or negative with residual = NULL: the call goes on to its later checks.  (That an r_ld % 4 != 0 is ignored
    as well can only be seen on a call that passes every check: test_gpu_nhwc_layers.py.)"""
    for r_ld in (0, 4, -5):
        assert call(L, "affine", residual=None, r_ld=r_ld, y=P + 4) == EUNSUPPORTED
        assert call(L, "affine", residual=None, r_ld=r_ld, N=0) == OK


def test_workspace_bytes(L):
    assert L.srf_nhwc_colmean_workspace_bytes(2, 8) == 2 * 64 * 8 * 4 and L.srf_nhwc_colmean_workspace_bytes(0, 8) == 0
    assert L.srf_nhwc_affine_relu_bwd_workspace_bytes(300, 8) == 2 * 2 * 8 * 4 and L.srf_nhwc_affine_relu_bwd_workspace_bytes(0, 8) == 0
    assert L.srf_nhwc_affine_relu_bwd_workspace_bytes(256, 8) == 2 * 8 * 4 and L.srf_nhwc_affine_relu_bwd_workspace_bytes(257, 8) == 2 * 2 * 8 * 4


# two defects at once: the earlier check answers
ORDER = [
    (NHW, dict(N=-1, C=6), EINVAL),                                      # size before shape
    (("affine", "colmean") + MAPS[:1] + DW, dict(x_ld=4, x=None), EINVAL),
    (("affine", "colmean", "pool_sum") + MAPS[:1] + DW, dict(C=0, x=None), EINVAL),   # size error before null pointer (same code, and ...)
    (NHW, dict(N=0, C=6), OK),                                           # ... the empty batch before everything but the sizes
    (("affine", "colmean") + MAPS[:1] + DW, dict(N=0, x=None), OK),
    (("affine", "colmean") + MAPS[:1] + DW, dict(N=0, x=P + 4), OK),
    (("pool_sum",), dict(B=0, x=None), OK),
    (NHW, dict(N=0, C=0), EINVAL),                                       # a size error even in an empty batch
    (COLS, dict(N=0, HW=-1), EINVAL),
    (("affine", "colmean", "pool_sum") + MAPS[:1] + DW, dict(x=None, C=6), EINVAL),   # null pointer before C % 4
    (("affine", "maxpool3s2_ceil") + DW, dict(y=None, x=P + 4), EINVAL),  # null pointer before alignment
    (("upsample_add",), dict(top=None, lat=P + 4), EINVAL),
    (("colsum_prod",), dict(b=None, a=P + 4), EINVAL),
    (COLS, dict(ws=None, N=65536), EINVAL),
    (COLS, dict(ws=P + 4, ws_bytes=0), EUNSUPPORTED),                    # alignment before workspace size
    (COLS, dict(C=6, ws_bytes=0), EUNSUPPORTED),
    (COLS, dict(N=65536, ws_bytes=0), EUNSUPPORTED),
    # srf_nhwc_affine_relu_bwd*: shape and alignment are checked before the pointers (M == 0 still has `sums` to zero)
    (BWD, dict(M=-1, C=6), EINVAL),
    (BWD, dict(gy_ld=4, sums=None), EINVAL),
    (BWD, dict(C=6, sums=None), EUNSUPPORTED),
    (BWD, dict(gy=P + 4, sums=None), EUNSUPPORTED),
    (BWD, dict(M=0, C=6), EUNSUPPORTED),
    (BWD, dict(M=0, sums=None), EINVAL),
    (BWD, dict(gy=None, ws_bytes=0), EINVAL),                            # null pointer before workspace size
]


@pytest.mark.parametrize("row", range(len(ORDER)))
def test_two_defects_are_answered_in_the_stated_order(L, row):
    entries, kw, want = ORDER[row]
    for e in entries:
        assert call(L, e, **kw) == want, (e, kw)
