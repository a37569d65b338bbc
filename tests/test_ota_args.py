"""Return codes of `srf_ota_assign`, `srf_ota_cost` and `srf_ota_match`, in the order the entry points check: non-positive sizes are
SRF_EINVAL, null pointers SRF_EINVAL, a shape outside the limits SRF_EUNSUPPORTED, a workspace too small SRF_EWORKSPACE -- all before any HIP
call: the library loads and answers on a machine without a GPU, and every pointer handed in here is a made-up address that no kernel may
ever see.  `ops.ota_assign_ok` states the same limits as integers."""
import ctypes

import pytest

from srfdet3d_amd import _lib, ops

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
PTR = ctypes.c_void_p(0x1000)        # never dereferenced: not a device address
SHAPE = dict(S=6, B=2, P=900, D=10, C=10, G=40)
ASSIGN_POINTERS = ["boxes", "logits", "gt", "labels", "n_gt", "heads", "count", "pred_idx", "gt_idx", "status", "ws"]
COST_POINTERS = ["boxes", "logits", "gt", "labels", "n_gt", "cost", "iou"]
MATCH_POINTERS = ["cost", "iou", "n_gt", "heads", "count", "pred_idx", "gt_idx", "status", "ws"]


def assign(boxes=PTR, logits=PTR, gt=PTR, labels=PTR, n_gt=PTR, heads=PTR, S=6, B=2, P=900, D=10, C=10, G=40, topk=8, count=PTR, pred_idx=PTR,
           gt_idx=PTR, status=PTR, ws=PTR, ws_bytes=0):
    """ws_bytes = 0 by default: a call that passes every other check still ends at SRF_EWORKSPACE, never in a launch."""
    return _lib.lib().srf_ota_assign(boxes, logits, gt, labels, n_gt, heads, S, B, P, D, C, G, 2.0, 0.25, 0.25, 0.25, 2.0, 1e-8, 2.5, topk, 6,
                                     count, pred_idx, gt_idx, status, ws, ws_bytes, None)


def cost(boxes=PTR, logits=PTR, gt=PTR, labels=PTR, n_gt=PTR, S=6, B=2, P=900, D=10, C=10, G=40, cost=PTR, iou=PTR):
    """No workspace to stop a valid call: only calls that fail a check are made."""
    return _lib.lib().srf_ota_cost(boxes, logits, gt, labels, n_gt, S, B, P, D, C, G, 2.0, 0.25, 0.25, 0.25, 2.0, 1e-8, 2.5, cost, iou, None)


def match(cost=PTR, iou=PTR, n_gt=PTR, heads=PTR, S=6, B=2, P=900, G=40, topk=8, count=PTR, pred_idx=PTR, gt_idx=PTR, status=PTR, ws=PTR,
          ws_bytes=0):
    return _lib.lib().srf_ota_match(cost, iou, n_gt, heads, S, B, P, G, topk, 6, count, pred_idx, gt_idx, status, ws, ws_bytes, None)


@pytest.mark.parametrize("name", ASSIGN_POINTERS)
def test_assign_null_pointers(name):
    assert assign(**{name: None}) == EINVAL


@pytest.mark.parametrize("name", COST_POINTERS)
def test_cost_null_pointers(name):
    assert cost(**{name: None}) == EINVAL


@pytest.mark.parametrize("name", MATCH_POINTERS)
def test_match_null_pointers(name):
    assert match(**{name: None}) == EINVAL


NON_POSITIVE = [dict(S=0), dict(S=-1), dict(B=0), dict(B=-2), dict(P=0), dict(P=-900), dict(G=0), dict(G=-8), dict(D=0), dict(D=-8), dict(C=0),
                dict(C=-10), dict(topk=0), dict(topk=-8)]


@pytest.mark.parametrize("kw", NON_POSITIVE)
def test_non_positive_sizes(kw):
    assert assign(**kw) == EINVAL
    assert assign(**kw, boxes=None, count=None) == EINVAL
    shape = {**SHAPE, **{k: v for k, v in kw.items() if k != "topk"}}
    assert not ops.ota_assign_ok(shape["S"], shape["B"], shape["P"], shape["D"], shape["C"], shape["G"], kw.get("topk", 8))
    if "topk" not in kw:
        assert cost(**kw) == EINVAL
    if "D" not in kw and "C" not in kw:
        assert match(**kw) == EINVAL


# every limit, one row each: (arguments, whether the matching stage alone has the limit too)
LIMITS = [(dict(P=4097), True), (dict(G=513), True), (dict(S=256, B=256), True), (dict(S=65536, B=1, P=1, G=1), True),
          (dict(D=7), False), (dict(D=9), False), (dict(D=11), False), (dict(C=65), False),
          (dict(S=64, B=64, P=4096, G=32), True),                 # the cost matrix reaches 2^31 bytes
          (dict(S=32, B=32, P=4096, G=512), True),
          (dict(S=128, B=128, P=4096, G=8, C=8), True)]


@pytest.mark.parametrize("kw,in_match", LIMITS)
def test_limits(kw, in_match):
    assert assign(**kw) == EUNSUPPORTED
    assert cost(**kw) == EUNSUPPORTED
    shape = {**SHAPE, **kw}
    assert not ops.ota_assign_ok(shape["S"], shape["B"], shape["P"], shape["D"], shape["C"], shape["G"], 8)     # the Python gate mirrors the code
    assert _lib.lib().srf_ota_workspace_bytes(shape["S"], shape["B"], shape["P"], shape["G"]) == (0 if in_match else
                                                                                                  workspace(shape["S"], shape["B"], shape["P"], shape["G"]))
    if in_match:
        assert match(**{k: v for k, v in kw.items() if k not in ("D", "C")}) == EUNSUPPORTED


def test_logits_past_2gb():
    kw = dict(S=64, B=64, P=4096, G=8, C=64)          # cost matrix 2^29 bytes, logits 2^32
    assert assign(**kw) == EUNSUPPORTED and cost(**kw) == EUNSUPPORTED
    assert not ops.ota_assign_ok(64, 64, 4096, 10, 64, 8)
    assert ops.ota_assign_ok(64, 64, 4096, 10, 8, 8 - 1) and ops.ota_assign_ok(64, 64, 4096 - 1, 10, 8, 8)


def workspace(S, B, P, G):
    mat = (S * B * P * G * 4 + 255) // 256 * 256
    return 2 * mat + (S * B * P * G + 255) // 256 * 256


INSIDE = [dict(), dict(P=1, G=1), dict(P=4096), dict(G=512), dict(D=8), dict(C=1), dict(C=64), dict(topk=1), dict(topk=900), dict(S=1, B=1),
          dict(S=255, B=257, P=8, G=8), dict(S=8, B=8, P=4096, G=512 - 8)]


@pytest.mark.parametrize("kw", INSIDE)
def test_inside_the_limits_the_python_gate_agrees(kw):
    """Every argument check passes; what stops the call is the workspace, one byte short: still no launch."""
    shape = {**SHAPE, **{k: v for k, v in kw.items() if k != "topk"}}
    assert ops.ota_assign_ok(shape["S"], shape["B"], shape["P"], shape["D"], shape["C"], shape["G"], kw.get("topk", 8))
    L = _lib.lib()
    need = L.srf_ota_workspace_bytes(shape["S"], shape["B"], shape["P"], shape["G"])
    assert need == workspace(shape["S"], shape["B"], shape["P"], shape["G"]) and need % 256 == 0
    assert assign(**kw, ws_bytes=need - 1) == EWORKSPACE
    need_m = L.srf_ota_match_workspace_bytes(shape["S"], shape["B"], shape["P"], shape["G"])
    assert need_m == (shape["S"] * shape["B"] * shape["P"] * shape["G"] + 255) // 256 * 256
    assert match(**{k: v for k, v in kw.items() if k not in ("D", "C")}, ws_bytes=need_m - 1) == EWORKSPACE


def test_the_order_of_the_checks():
    assert assign(P=0, D=9) == EINVAL                            # sizes first
    assert assign(D=9, boxes=None) == EINVAL                     # null pointers before the limits
    assert assign(D=9) == EUNSUPPORTED                           # the limits before the workspace
    assert assign() == EWORKSPACE
    assert match(P=5000, cost=None) == EINVAL and match(P=5000) == EUNSUPPORTED and match() == EWORKSPACE
    assert cost(D=9, cost=None) == EINVAL and cost(D=9) == EUNSUPPORTED


def test_workspace_size():
    L = _lib.lib()
    assert L.srf_ota_workspace_bytes(0, 2, 900, 40) == 0 and L.srf_ota_workspace_bytes(6, 2, -1, 40) == 0
    assert L.srf_ota_match_workspace_bytes(6, 2, 900, 0) == 0 and L.srf_ota_match_workspace_bytes(6, 2, 4097, 8) == 0
    assert L.srf_ota_workspace_bytes(6, 2, 900, 40) == workspace(6, 2, 900, 40)


def test_the_limits_as_integers():
    assert (ops.OTA_MAX_P, ops.OTA_MAX_G, ops.OTA_MAX_C, ops.OTA_MAX_PAIRS) == (4096, 512, 64, 65535)


def test_all_are_declared_and_bound():
    assert {"srf_ota_assign", "srf_ota_cost", "srf_ota_match", "srf_ota_workspace_bytes", "srf_ota_match_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert _lib.lib().srf_abi_version() == 1


def test_srf_ota_switch(monkeypatch):
    monkeypatch.delenv("SRF_OTA", raising=False)
    assert ops.ota_enabled()
    monkeypatch.setenv("SRF_OTA", "0")
    assert not ops.ota_enabled()                     # read at every call
    monkeypatch.setenv("SRF_OTA", "1")
    assert ops.ota_enabled()
