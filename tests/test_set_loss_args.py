"""Return codes of `srf_set_loss` in the order the entry point checks: non-positive sizes and divisors that are not positive finite numbers are
SRF_EINVAL, null pointers SRF_EINVAL, arguments outside the limits SRF_EUNSUPPORTED, a workspace too small SRF_EWORKSPACE -- all before any
HIP call: the library answers on a machine without a GPU, and every pointer handed in here is a made-up address that no kernel may ever
see.  `ops.set_loss_ok` states the same limits as integers and agrees row by row; `training.set_loss_route` gives its verdicts on
stand-ins for GPU tensors."""
import ctypes
import math
import types

import pytest
import torch

from srfdet3d_amd import _lib, ops
from srfdet3d_amd.plugin import training

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
PTR = ctypes.c_void_p(0x1000)        # never dereferenced: not a device address
SHAPE = dict(S=6, B=2, P=900, C=10, D=10, Dw=10, G=40, Dg=9)
POINTERS = ["logits", "boxes", "count", "pred_idx", "gt_idx", "gt", "labels", "cw", "loss", "grad_logits", "grad_boxes", "ws"]


def call(logits=PTR, boxes=PTR, count=PTR, pred_idx=PTR, gt_idx=PTR, gt=PTR, labels=PTR, cw=PTR, num="ones", S=6, B=2, P=900, C=10, D=10, Dw=10,
         G=40, Dg=9, alpha=0.25, gamma=2.0, loss=PTR, grad_logits=PTR, grad_boxes=PTR, ws=PTR, ws_bytes=0):
    """ws_bytes = 0 by default: a call that passes every other check still ends at SRF_EWORKSPACE, never in a launch."""
    if num == "ones":
        num = [1.0] * (2 * max(S, 1))
    return _lib.lib().srf_set_loss(logits, boxes, count, pred_idx, gt_idx, gt, labels, cw, None if num is None else _lib.hf(num), S, B, P, C, D,
                                   Dw, G, Dg, alpha, gamma, 2.0, 0.25, loss, grad_logits, grad_boxes, ws, ws_bytes, None)


def gate(kw):
    s = {**SHAPE, **{k: v for k, v in kw.items() if k in SHAPE}}
    return ops.set_loss_ok(s["S"], s["B"], s["P"], s["C"], s["D"], s["Dw"], s["G"], s["Dg"], kw.get("gamma", 2.0), kw.get("alpha", 0.25))


def workspace(S, B, P):
    return (S * B * ((P + 63) // 64) * 2 * 8 + 255) // 256 * 256


@pytest.mark.parametrize("name", POINTERS + ["num"])
def test_null_pointers(name):
    assert call(**{name: None}) == EINVAL


NON_POSITIVE = [dict(S=0), dict(S=-1), dict(B=0), dict(B=-2), dict(P=0), dict(P=-900), dict(C=0), dict(C=-10), dict(D=0), dict(D=-8), dict(Dw=0),
                dict(Dw=-8), dict(G=0), dict(G=-8), dict(Dg=0), dict(Dg=-7)]


@pytest.mark.parametrize("kw", NON_POSITIVE)
def test_non_positive_sizes(kw):
    assert call(**kw) == EINVAL
    assert call(**kw, logits=None, loss=None) == EINVAL
    assert not gate(kw)
    s = {**SHAPE, **kw}
    assert _lib.lib().srf_set_loss_workspace_bytes(s["S"], s["B"], s["P"], s["C"], s["D"]) == (0 if set(kw) & set("SBPCD") else workspace(6, 2, 900))


@pytest.mark.parametrize("bad", [0.0, -1.0, math.inf, -math.inf, math.nan])
@pytest.mark.parametrize("at", [0, 1, 11])
def test_divisors(bad, at):
    num = [1.0] * 12
    num[at] = bad
    assert call(num=num) == EINVAL
    assert call(num=num, D=9) == EINVAL                          # before the limits
    with pytest.raises((ValueError, RuntimeError)):                 # the wrapper refuses them as well (and CPU tensors before that)
        ops.set_loss(*[torch.zeros(1)] * 8, [num[0:2]], 0.25, 2.0, 2.0, 0.25)


# every limit, one row each; the last column: whether the workspace size, which sees S, B, P, C and D only, is 0 too
LIMITS = [(dict(P=4097), True), (dict(G=513), False), (dict(S=256, B=256, P=8), True), (dict(S=65536, B=1, P=1), True), (dict(C=65), True),
          (dict(D=7), True), (dict(D=9), True), (dict(D=11), True), (dict(D=8), False), (dict(D=8, Dw=8, Dg=9), False),
          (dict(D=8, Dw=10, Dg=7), False), (dict(Dw=8, Dg=8), False), (dict(Dw=9), False), (dict(Dw=10, Dg=7), False), (dict(Dw=7, Dg=7), False),
          (dict(gamma=0.5), False), (dict(gamma=0.999), False), (dict(gamma=math.inf), False), (dict(gamma=math.nan), False),
          (dict(alpha=-0.01), False), (dict(alpha=1.01), False), (dict(alpha=math.nan), False),
          (dict(S=8, B=1024, P=4096, C=16), True),                # the logits reach 2^31 bytes
          (dict(S=16, B=4095, P=2048, C=64), True),
          (dict(S=13, B=1009, P=4096, C=1), True)]                # the boxes do (D = 10)


@pytest.mark.parametrize("kw,in_workspace", LIMITS)
def test_limits(kw, in_workspace):
    assert call(**kw) == EUNSUPPORTED
    assert call(**kw, ws_bytes=1 << 40) == EUNSUPPORTED
    assert not gate(kw)                                           # the Python gate mirrors the code
    s = {**SHAPE, **{k: v for k, v in kw.items() if k in SHAPE}}
    got = _lib.lib().srf_set_loss_workspace_bytes(s["S"], s["B"], s["P"], s["C"], s["D"])
    assert got == (0 if in_workspace else workspace(s["S"], s["B"], s["P"]))


INSIDE = [dict(), dict(P=1, G=1), dict(P=4096), dict(G=512), dict(C=1), dict(C=64), dict(S=1, B=1), dict(S=255, B=257, P=8), dict(S=65535, B=1, P=1),
          dict(D=8, Dw=8, Dg=7), dict(D=10, Dw=8, Dg=7), dict(D=10, Dw=8, Dg=9), dict(D=10, Dw=10, Dg=9), dict(gamma=1.0), dict(gamma=1.5),
          dict(gamma=5.0), dict(alpha=0.0), dict(alpha=1.0), dict(S=8, B=1024, P=4095, C=16), dict(S=13, B=1008, P=4096, C=1)]


@pytest.mark.parametrize("kw", INSIDE)
def test_inside_the_limits_the_python_gate_agrees(kw):
    """Every argument check passes; what stops the call is the workspace, one byte short: still no launch."""
    assert gate(kw)
    s = {**SHAPE, **{k: v for k, v in kw.items() if k in SHAPE}}
    need = _lib.lib().srf_set_loss_workspace_bytes(s["S"], s["B"], s["P"], s["C"], s["D"])
    assert need == workspace(s["S"], s["B"], s["P"]) and need % 256 == 0 and need > 0
    assert call(**kw, ws_bytes=need - 1) == EWORKSPACE


def test_the_order_of_the_checks():
    assert call(P=0, D=9) == EINVAL                              # sizes first
    assert call(num=[1.0] * 11 + [0.0], logits=None, D=9) == EINVAL
    assert call(D=9, logits=None) == EINVAL                      # null pointers before the limits
    assert call(D=9) == EUNSUPPORTED                             # the limits before the workspace
    assert call(gamma=0.5, ws_bytes=0) == EUNSUPPORTED
    assert call() == EWORKSPACE


def test_workspace_size_and_the_limits_as_integers():
    L = _lib.lib()
    assert L.srf_set_loss_workspace_bytes(0, 2, 900, 10, 10) == 0 and L.srf_set_loss_workspace_bytes(6, 2, -1, 10, 10) == 0
    assert L.srf_set_loss_workspace_bytes(6, 2, 900, 10, 10) == workspace(6, 2, 900) == 3072      # 180 workgroups x 2 doubles = 2880 bytes
    assert (ops.SET_LOSS_MAX_P, ops.SET_LOSS_MAX_G, ops.SET_LOSS_MAX_C, ops.SET_LOSS_MAX_PAIRS) == (4096, 512, 64, 65535)
    assert ops.SET_LOSS_BOX_COLUMNS == ((8, 8, 7), (10, 8, 7), (10, 8, 9), (10, 10, 9))
    assert {"srf_set_loss", "srf_set_loss_workspace_bytes"} <= set(_lib.SIGNATURES)


def test_srf_set_loss_switch(monkeypatch):
    monkeypatch.delenv("SRF_SET_LOSS", raising=False)
    assert not ops.set_loss_enabled()                            # off by default
    monkeypatch.setenv("SRF_SET_LOSS", "1")
    assert ops.set_loss_enabled()                                # read at every call
    monkeypatch.setenv("SRF_SET_LOSS", "0")
    assert not ops.set_loss_enabled()


def test_set_loss_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.set_loss(*[torch.zeros(1)] * 8, [(1.0, 1.0)], 0.25, 2.0, 2.0, 0.25)


# ---- the route predicate, on stand-ins: it reads is_cuda / dtype / shape / dim() / numel() and nothing else of a tensor
def fake(*shape, cuda=True, dtype=torch.float32):
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, shape=torch.Size(shape), dim=lambda: len(shape), numel=lambda: math.prod(shape))


def route_case(S=3, B=2, P=64, C=10, D=10, Dg=9, cuda=True, dtype=torch.float32, loss_cls=None, loss_bbox=None, rows=True, raw=True):
    head = types.SimpleNamespace(
        loss_cls=loss_cls if loss_cls is not None else training.FocalLoss(gamma=2.0, alpha=0.25, reduction="sum", loss_weight=2.0),
        loss_bbox=loss_bbox if loss_bbox is not None else training.L1Loss(reduction="sum", loss_weight=0.25), code_weights=fake(D, cuda=cuda))
    outs = [dict(pred_logits=fake(B, P, C, cuda=cuda, dtype=dtype), pred_boxes=fake(B, P, D, cuda=cuda, dtype=dtype)) for _ in range(S)]
    one = lambda r: training.Assigned(None, None, rows=object() if r else None)
    assigned = training.AssignedLayers([one(True) for _ in range(B)] for _ in range(S))
    if not rows:
        assigned[1][0] = one(False)
    if raw:
        assigned.raw = dict(gt_boxes=fake(B, 8, Dg, cuda=cuda))
    return head, outs, assigned, [fake(5, Dg, cuda=cuda) for _ in range(B)]


class OtherFocal(training.FocalLoss):
    pass


def test_the_route_predicate(monkeypatch):
    monkeypatch.setenv("SRF_SET_LOSS", "1")
    assert training.set_loss_route(*route_case())
    assert training.set_loss_route(*route_case(D=8, Dg=7)) and training.set_loss_route(*route_case(S=1, P=1, C=1))
    verdicts = {
        "cpu tensors": route_case(cuda=False),
        "float64": route_case(dtype=torch.float64),
        "reduction mean": route_case(loss_cls=training.FocalLoss(gamma=2.0, alpha=0.25, reduction="mean")),
        "L1 reduction mean": route_case(loss_bbox=training.L1Loss(reduction="mean")),
        "a subclass of FocalLoss": route_case(loss_cls=OtherFocal(reduction="sum")),
        "a pair without rows": route_case(rows=False),
        "the torch assignment": route_case(raw=False),
        "gamma below 1": route_case(loss_cls=training.FocalLoss(gamma=0.5, reduction="sum")),
        "too many rows": route_case(P=4097),
        "box columns": route_case(D=8, Dg=9),
    }
    for why, args in verdicts.items():
        assert not training.set_loss_route(*args), why
    head, outs, assigned, gts = route_case()
    outs[2]["pred_logits"] = fake(2, 65, 10)
    assert not training.set_loss_route(head, outs, assigned, gts)             # one shape for all stages
    assert not training.set_loss_route(head, outs[:2], assigned, gts)
    assert not training.set_loss_route(*route_case()[:2], [[None, None]] * 3, gts)   # a plain list: another assigner
    monkeypatch.setenv("SRF_SET_LOSS", "0")
    assert not training.set_loss_route(*route_case())                         # the switch
    monkeypatch.delenv("SRF_SET_LOSS")
    assert not training.set_loss_route(*route_case())                         # off by default
