"""Return codes of srf_roi_extract_bwd_ordered and srf_spconv_bwd_weight_ordered, their workspace queries, and the switch
`ops.deterministic_enabled()`.  Both entry points decide every refusal on the host before they enqueue anything, so they answer
on a machine without a GPU.

As in tests/test_rulebook_args.py every device pointer is a made-up address that no kernel may ever see: each call is the entry
point's VALID call (which is never made) with exactly one thing wrong.  The level table and the array of gradient pointers are host
arrays and real."""
import ctypes

import pytest

from srfdet3d_amd import _lib, ops
from srfdet3d_amd._lib import FeatMap

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
PTR = ctypes.c_void_p(0x10000)       # never dereferenced: not a device address, 16-byte aligned
BIG = 1 << 40                        # a workspace size no check objects to
NL, C, R, POOLED, SR = 4, 256, 100, 7, 2


def _levels(shapes=((2, 48, 80), (2, 24, 40), (2, 12, 20), (2, 6, 10)), data=0x20000):
    return (FeatMap * len(shapes))(*[FeatMap(data, n, h, w, h * w * C, 1, w * C, C, 1.0 / (4 << i)) for i, (n, h, w) in enumerate(shapes)])


def _grads(n=NL, null_at=None):
    return (ctypes.c_void_p * n)(*[None if i == null_at else 0x30000 + 0x1000 * i for i in range(n)])


ROI_NAMES = "levels grad_levels num_levels C rois R pooled sr finest grad_out so_r so_c so_b workspace workspace_bytes".split()


def _roi_valid():
    return dict(levels=_levels(), grad_levels=_grads(), num_levels=NL, C=C, rois=PTR, R=R, pooled=POOLED, sr=SR, finest=56.0, grad_out=PTR,
                so_r=C * 49, so_c=1, so_b=C, workspace=PTR, workspace_bytes=BIG)


def roi_refusal(**wrong):
    valid = _roi_valid()
    assert wrong and set(wrong) <= set(valid)
    kw = dict(valid, **wrong)
    return _lib.lib().srf_roi_extract_bwd_ordered(*[kw[n] for n in ROI_NAMES], None)


def test_roi_entry_refusals():
    L = _lib.lib()
    need = L.srf_roi_extract_bwd_ordered_workspace_bytes(R, POOLED, SR)
    assert need >= R * POOLED * POOLED * SR * SR * 4 * 24
    table = [
        # the rows of srf_roi_extract_bwd, in its order
        (dict(levels=None), EINVAL), (dict(grad_levels=None), EINVAL), (dict(num_levels=0), EINVAL), (dict(num_levels=5), EINVAL),
        (dict(C=0), EINVAL), (dict(R=-1), EINVAL), (dict(pooled=0), EINVAL), (dict(pooled=9), EINVAL), (dict(sr=0), EINVAL),
        (dict(sr=5), EINVAL), (dict(finest=0.0), EINVAL), (dict(finest=float("nan")), EINVAL),
        (dict(rois=None), EINVAL), (dict(grad_out=None), EINVAL),
        (dict(grad_levels=_grads(null_at=2)), EINVAL), (dict(levels=_levels(((2, 48, 80), (0, 24, 40), (2, 12, 20), (2, 6, 10)))), EINVAL),
        (dict(levels=_levels(((2, 48, 80), (2, 0, 40), (2, 12, 20), (2, 6, 10)))), EINVAL),
        # the key width: 2^30 pixels in one level, or between the levels
        (dict(levels=_levels(((1 << 10, 1 << 10, 1 << 10), (2, 24, 40), (2, 12, 20), (2, 6, 10)))), EUNSUPPORTED),
        (dict(levels=_levels(((1 << 9, 1 << 10, 1 << 10),) * 2), grad_levels=_grads(2), num_levels=2), EUNSUPPORTED),
        (dict(R=(1 << 24) + 1), EUNSUPPORTED), (dict(R=1 << 24, pooled=8, sr=4), EUNSUPPORTED),
        # the workspace
        (dict(workspace=None), EINVAL), (dict(workspace_bytes=need - 1), EWORKSPACE), (dict(workspace_bytes=0), EWORKSPACE),
        (dict(workspace=ctypes.c_void_p(0x10004), workspace_bytes=need), EUNSUPPORTED),
    ]
    for wrong, code in table:
        assert roi_refusal(**wrong) == code, wrong
    # order: bad scalars before R == 0, R == 0 before the pointers, the pointers before the limits, the limits before the workspace
    assert roi_refusal(R=0, rois=None, grad_out=None, workspace=None, workspace_bytes=0) == 0
    assert roi_refusal(R=0, pooled=9) == EINVAL
    assert roi_refusal(rois=None, R=(1 << 24) + 1) == EINVAL
    assert roi_refusal(R=(1 << 24) + 1, workspace_bytes=0) == EUNSUPPORTED
    assert roi_refusal(workspace_bytes=0, workspace=ctypes.c_void_p(0x10004)) == EWORKSPACE
    # levels of 2^28 pixels each: four of them fill the 30 bits, three stay inside
    half = ((1 << 9, 1 << 10, 1 << 9),)
    assert roi_refusal(levels=_levels(half * 4), workspace_bytes=0) == EUNSUPPORTED
    assert roi_refusal(levels=_levels(half * 3), grad_levels=_grads(3), num_levels=3, workspace_bytes=0) == EWORKSPACE


def test_roi_workspace_bytes():
    f = _lib.lib().srf_roi_extract_bwd_ordered_workspace_bytes
    for args in ((0, 7, 2), (-1, 7, 2), (10, 0, 2), (10, -7, 2), (10, 7, 0), (10, 7, -2), (10, 9, 2), (10, 7, 5), ((1 << 24) + 1, 7, 2),
                 (1 << 24, 8, 4)):
        assert f(*args) == 0, args
    for pooled, sr in ((7, 2), (2, 3), (8, 4), (1, 1)):
        sizes = [f(r, pooled, sr) for r in (1, 2, 3, 10, 11, 100, 1000, 10800, 10801, 100000)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (pooled, sr, sizes)
    assert f(10800, 7, 2) < 256 << 20                                        # config 4's 10800 image RoIs: about 200 MB


SP_NAMES = "inp A_in Cin grad_out A_out Cout nbr nbr_stride K grad_W workspace workspace_bytes".split()
SP_VALID = dict(inp=PTR, A_in=5000, Cin=64, grad_out=PTR, A_out=5000, Cout=128, nbr=PTR, nbr_stride=5000, K=27, grad_W=PTR, workspace=PTR,
                workspace_bytes=BIG)


def sp_refusal(**wrong):
    assert wrong and set(wrong) <= set(SP_VALID) and any(v is None or v != SP_VALID[k] for k, v in wrong.items())
    kw = dict(SP_VALID, **wrong)
    return _lib.lib().srf_spconv_bwd_weight_ordered(*[kw[n] for n in SP_NAMES], None)


def test_spconv_entry_refusals():
    L = _lib.lib()
    need = L.srf_spconv_bwd_weight_ordered_workspace_bytes(5000, 64, 128, 27)
    assert need == 3 * 27 * 64 * 128 * 4                                     # three ranges of 2048 rows
    table = [(dict(A_in=-1), EINVAL), (dict(A_out=-1), EINVAL), (dict(Cin=0), EINVAL), (dict(Cout=0), EINVAL), (dict(K=0), EINVAL),
             (dict(nbr_stride=4999), EINVAL), (dict(Cin=129), EUNSUPPORTED), (dict(Cout=256), EUNSUPPORTED), (dict(grad_W=None), EINVAL),
             (dict(inp=None), EINVAL), (dict(grad_out=None), EINVAL), (dict(nbr=None), EINVAL), (dict(workspace=None), EINVAL),
             (dict(workspace_bytes=need - 1), EWORKSPACE), (dict(workspace_bytes=0), EWORKSPACE)]
    for wrong, code in table:
        assert sp_refusal(**wrong) == code, wrong
    # the order of srf_spconv_bwd_weight: sizes, then the channel limit, then the pointers; the workspace last
    assert sp_refusal(Cin=129, K=0) == EINVAL
    assert sp_refusal(Cin=129, grad_W=None) == EUNSUPPORTED
    assert sp_refusal(inp=None, workspace_bytes=0) == EINVAL
    # ... and the codes of the atomic entry on the rows they share
    for wrong, code in table[:9]:
        kw = dict(SP_VALID, **wrong)
        assert L.srf_spconv_bwd_weight(*[kw[n] for n in SP_NAMES[:10]], None) == code, wrong


def test_spconv_workspace_bytes():
    f = _lib.lib().srf_spconv_bwd_weight_ordered_workspace_bytes
    for args in ((0, 16, 16, 27), (-5, 16, 16, 27), (100, 0, 16, 27), (100, 16, -1, 27), (100, 16, 16, 0), (100, 129, 16, 27), (100, 16, 130, 27)):
        assert f(*args) == 0, args
    sizes = [f(a, 5, 16, 27) for a in (1, 2047, 2048, 2049, 4096, 4097, 180000)]
    assert sizes == [n * 27 * 5 * 16 * 4 for n in (1, 1, 1, 2, 2, 3, 88)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_the_switch_is_read_at_every_call(monkeypatch):
    monkeypatch.delenv("SRF_DETERMINISTIC", raising=False)
    assert ops.deterministic_enabled() is False
    monkeypatch.setenv("SRF_DETERMINISTIC", "0")
    assert ops.deterministic_enabled() is False
    monkeypatch.setenv("SRF_DETERMINISTIC", "1")
    assert ops.deterministic_enabled() is True
    monkeypatch.delenv("SRF_DETERMINISTIC")
    assert ops.deterministic_enabled() is False
    # torch's own flags do not move it
    import torch
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        assert ops.deterministic_enabled() is False
    finally:
        torch.use_deterministic_algorithms(before)
