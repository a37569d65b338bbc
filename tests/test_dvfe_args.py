"""Return codes of `srf_dvfe_fwd`, in the order the entry point checks: non-positive sizes are SRF_EINVAL, an empty input SRF_OK with no
launch, null pointers SRF_EINVAL, a shape outside the limits SRF_EUNSUPPORTED, a workspace too small SRF_EWORKSPACE -- all before any HIP
call: the library loads and answers on a machine without a GPU, and every pointer handed in here is a made-up address that no kernel may
ever see."""
import ctypes

import pytest

from srfdet3d_amd import _lib, ops

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
PTR = ctypes.c_void_p(0x1000)        # never dereferenced: not a device address
V3 = _lib.hf([0.1, 0.1, 0.15])
POINTERS = ["points", "p2v", "order", "offsets", "counts", "num_voxels", "vcoors", "vs", "off", "W1", "s1", "h1", "W2", "s2", "h2", "Wa", "sa",
            "ha", "out", "ws"]


def fwd(points=PTR, n=1000, nf=5, p2v=PTR, order=PTR, offsets=PTR, counts=PTR, num_voxels=PTR, vcoors=PTR, rows=400, vs=V3, off=V3, centre=1,
        W1=PTR, s1=PTR, h1=PTR, W2=PTR, s2=PTR, h2=PTR, d=32, Wa=PTR, sa=PTR, ha=PTR, C0=5, Wb=PTR, sb=PTR, hb=PTR, C1=5, out=PTR, ws=PTR,
        ws_bytes=0):
    """ws_bytes = 0 by default: a call that passes every other check still ends at SRF_EWORKSPACE, never in a launch."""
    return _lib.lib().srf_dvfe_fwd(points, n, nf, p2v, order, offsets, counts, num_voxels, vcoors, rows, vs, off, centre, W1, s1, h1, W2, s2, h2,
                                   d, Wa, sa, ha, C0, Wb, sb, hb, C1, out, ws, ws_bytes, None)


@pytest.mark.parametrize("name", POINTERS)
def test_null_pointers(name):
    assert fwd(**{name: None}) == EINVAL


@pytest.mark.parametrize("name", ["Wb", "sb", "hb"])
def test_second_layer_pointers_only_with_a_second_layer(name):
    assert fwd(**{name: None}) == EINVAL
    assert fwd(**{name: None, "C1": 0}) == EWORKSPACE     # one layer: they are not looked at, the call gets as far as the workspace


@pytest.mark.parametrize("kw", [dict(n=-1), dict(rows=-1), dict(nf=0), dict(nf=-4), dict(d=0), dict(d=-32), dict(C0=0), dict(C0=-5),
                                dict(C1=-1)])
def test_non_positive_sizes(kw):
    assert fwd(**kw) == EINVAL
    assert fwd(**kw, points=None, out=None) == EINVAL


@pytest.mark.parametrize("kw", [dict(nf=2), dict(nf=9), dict(d=8), dict(d=24), dict(d=48), dict(d=128), dict(C0=17), dict(C1=17),
                                dict(n=(1 << 29) // 5 + 1), dict(n=(1 << 29) // 16, C0=16, nf=3),
                                dict(n=1 << 26, rows=1 << 27, nf=3, C0=4, C1=4), dict(n=1 << 25, rows=1 << 26, nf=3, C0=8, C1=0)])
def test_limits(kw):
    assert fwd(**kw) == EUNSUPPORTED
    shape = dict(n=1000, rows=400, nf=5, d=32, C0=5, C1=5)
    shape.update(kw)
    assert not ops.dvfe_ok(shape["n"], shape["rows"], shape["nf"], shape["d"], shape["C0"], shape["C1"])    # the Python gate mirrors the code


@pytest.mark.parametrize("kw", [dict(), dict(nf=3), dict(nf=8), dict(d=16), dict(d=64), dict(C0=1, C1=1), dict(C0=16, C1=16), dict(C1=0),
                                dict(n=(1 << 29) // 16 - 1, C0=16, nf=3)])
def test_inside_the_limits_the_python_gate_agrees(kw):
    """Every argument check passes; what stops the call is the workspace, one byte short: still no launch."""
    shape = dict(n=1000, rows=400, nf=5, d=32, C0=5, C1=5)
    shape.update(kw)
    assert ops.dvfe_ok(shape["n"], shape["rows"], shape["nf"], shape["d"], shape["C0"], shape["C1"])
    need = _lib.lib().srf_dvfe_workspace_bytes(shape["n"], shape["C0"])
    assert need >= shape["n"] * shape["C0"] * 4 and need % 256 == 0
    assert fwd(**kw, ws_bytes=need - 1) == EWORKSPACE


def test_empty_is_ok_without_a_launch():
    nothing = dict(points=None, p2v=None, order=None, offsets=None, counts=None, vcoors=None, out=None, ws=None)
    assert fwd(n=0, **nothing) == OK
    assert fwd(rows=0, **nothing) == OK
    assert fwd(n=0, nf=9, d=24) == OK              # the limits come after the empty input ...
    assert fwd(n=0, nf=0) == EINVAL                # ... the sizes before it


def test_the_order_of_the_checks():
    assert fwd(nf=9, points=None) == EINVAL                      # null pointers before the limits
    assert fwd(nf=9) == EUNSUPPORTED                             # the limits before the workspace
    assert fwd() == EWORKSPACE


def test_workspace_size():
    L = _lib.lib()
    assert L.srf_dvfe_workspace_bytes(0, 5) == 0 and L.srf_dvfe_workspace_bytes(-3, 5) == 0 and L.srf_dvfe_workspace_bytes(10, 0) == 0
    assert L.srf_dvfe_workspace_bytes(180000, 5) == (180000 * 5 * 4 + 255) // 256 * 256


def test_both_are_declared_and_bound():
    assert {"srf_dvfe_fwd", "srf_dvfe_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert _lib.lib().srf_abi_version() == 1
