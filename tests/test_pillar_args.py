"""Return codes of `srf_pillar_vfe` and `srf_pillar_scatter_nhwc`: null pointers and non-positive sizes are SRF_EINVAL, a shape outside the
limits SRF_EUNSUPPORTED, both before any HIP call -- the library loads and answers on a machine without a GPU, and every pointer handed in
here is a made-up address that no kernel may ever see."""
import ctypes

import pytest

from srfdet3d_amd import _lib, ops

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
PTR = ctypes.c_void_p(0x1000)        # never dereferenced: 16-byte aligned, not a device address
V3 = _lib.hf([0.2, 0.2, 8.0])


def vfe(voxels=PTR, num=PTR, coors=PTR, rows_dev=None, rows=100, P=20, nf=5, vs=V3, off=V3, cluster=1, centre=1, legacy=0, W=PTR, scale=PTR,
        shift=PTR, cout=64, out=PTR):
    return _lib.lib().srf_pillar_vfe(voxels, num, coors, rows_dev, rows, P, nf, vs, off, cluster, centre, legacy, W, scale, shift, cout, out,
                                     None)


def scatter(feats=PTR, coors=PTR, rows_dev=None, rows=100, C=64, B=1, H=8, W=8, out=PTR):
    return _lib.lib().srf_pillar_scatter_nhwc(feats, coors, rows_dev, rows, C, B, H, W, out, None)


@pytest.mark.parametrize("name", ["voxels", "num", "coors", "W", "scale", "shift", "out", "vs", "off"])
def test_vfe_null_pointers(name):
    assert vfe(**{name: None}) == EINVAL


@pytest.mark.parametrize("kw", [dict(rows=-1), dict(P=0), dict(P=-3), dict(nf=0), dict(nf=-1), dict(cout=0), dict(cout=-64)])
def test_vfe_non_positive_sizes(kw):
    assert vfe(**kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(cout=32), dict(cout=96), dict(cout=320), dict(nf=2), dict(nf=9), dict(P=65),
                                dict(rows=(1 << 29) // 100 + 1), dict(rows=(1 << 29) // 256, cout=256, P=1, nf=3)])
def test_vfe_limits(kw):
    assert vfe(**kw) == EUNSUPPORTED
    shape = dict(rows=100, P=20, nf=5, cout=64)
    shape.update(kw)
    assert not ops.pillar_vfe_ok(shape["rows"], shape["P"], shape["nf"], shape["cout"])    # the Python gate mirrors the code


def test_vfe_empty_is_ok_without_a_launch():
    assert vfe(rows=0, voxels=None, num=None, coors=None, out=None) == OK
    assert vfe(rows=0, cout=96) == EUNSUPPORTED


@pytest.mark.parametrize("kw", [dict(out=None), dict(feats=None), dict(coors=None), dict(rows=-1), dict(C=0), dict(C=-4), dict(B=0),
                                dict(H=0), dict(W=-1), dict(out=ctypes.c_void_p(0x1004)), dict(feats=ctypes.c_void_p(0x1008))])
def test_scatter_invalid(kw):
    assert scatter(**kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(C=6), dict(C=63), dict(B=8, H=1024, W=1024), dict(rows=(1 << 29) // 64)])
def test_scatter_limits(kw):
    assert scatter(**kw) == EUNSUPPORTED
    shape = dict(rows=100, C=64, B=1, H=8, W=8)
    shape.update(kw)
    assert not ops.pillar_scatter_ok(shape["rows"], shape["C"], shape["B"], shape["H"], shape["W"])


def test_both_are_declared_and_bound():
    assert {"srf_pillar_vfe", "srf_pillar_scatter_nhwc"} <= set(_lib.SIGNATURES)
    assert _lib.lib().srf_abi_version() == 1
