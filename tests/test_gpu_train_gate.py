"""The gate of srfdet3d_amd/train_conv.py: the verdict of each of its seven predicates (and of `dense._train_fusable`) over a table of
layers and tensors -- one accepted row per predicate, one row per refusal reason, and one row per difference between the predicates
(which of them look at autocast, dim(), the memory format and which switch).  The tensors are `torch.empty` on the device and the
modules stay on the host (no predicate looks at where the weights are), so nothing is launched, except by the `bn_eval` rows, whose
accepted route is three elementwise kernels on 256 floats.

The expected verdicts are those of the predicates as they were BEFORE they were rewritten over one base predicate and a route table:
`verdict` below was run once with that commit's modules on these rows and the results are the last column.  They are not taken from
the code under test."""
import contextlib
import os

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


def _x(dev, shape=(2, 32, 8, 8), cl=True, grad=True):
    fmt = torch.channels_last if cl and len(shape) == 4 else torch.contiguous_format
    return torch.empty(shape, device=dev, memory_format=fmt).requires_grad_(grad)


def _conv(cin=32, cout=32, k=3, frozen=False, **kw):
    conv = nn.Conv2d(cin, cout, k, padding=k // 2, **kw)
    return conv.requires_grad_(not frozen)


def _bn(c=32, train=False, **kw):
    return nn.BatchNorm2d(c, **kw).train(train)


def _osa(cin=32, width=32, cout=64, train=False, biased=False, depthwise=False, frozen=False):
    from srfdet3d_amd.plugin.vovnet import OSAModule
    blk = OSAModule(cin, width, cout, 2, "b", depthwise=depthwise).train(train)
    if biased:
        blk.layers[0][0] = nn.Conv2d(cin, width, 3, 1, 1, bias=True)
    return blk.requires_grad_(not frozen)


def _ese(c=32):
    from srfdet3d_amd.plugin.vovnet import eSEModule
    return eSEModule(c)


NOGRAD, AUTOCAST = "no_grad", "autocast"

# (id, predicate, layer(s) -> tuple, tensor keywords, environment, context, verdict of the parent commit)
ROWS = [
    # eligible: 3x3 / stride 1 on `_Wino43Conv`
    ("eligible/accepted", "eligible", lambda: (_conv(),), {}, {}, None, True),
    ("eligible/no_grad_mode", "eligible", lambda: (_conv(),), {}, {}, NOGRAD, False),
    ("eligible/nothing_requires_grad", "eligible", lambda: (_conv(frozen=True),), dict(grad=False), {}, None, False),
    ("eligible/autocast", "eligible", lambda: (_conv(),), {}, {}, AUTOCAST, False),
    ("eligible/nchw_is_taken", "eligible", lambda: (_conv(),), dict(cl=False), {}, None, True),           # difference: no stride(1) == 1
    ("eligible/cin24", "eligible", lambda: (_conv(24),), dict(shape=(2, 24, 8, 8)), {}, None, False),
    ("eligible/hw1_is_taken", "eligible", lambda: (_conv(),), dict(shape=(2, 32, 1, 1)), {}, None, True),
    ("eligible/CONV=0", "eligible", lambda: (_conv(),), {}, dict(SRF_TRAIN_CONV="0"), None, False),
    ("eligible/FUSED=0_not_consulted", "eligible", lambda: (_conv(),), {}, dict(SRF_TRAIN_FUSED="0"), None, True),
    ("eligible/WGRAD=0_not_consulted", "eligible", lambda: (_conv(),), {}, dict(SRF_TRAIN_WGRAD="0"), None, True),   # `_weight_grad`'s alone
    # eligible_1x1
    ("eligible_1x1/accepted", "eligible_1x1", lambda: (_conv(k=1),), {}, {}, None, True),
    ("eligible_1x1/no_grad_mode", "eligible_1x1", lambda: (_conv(k=1),), {}, {}, NOGRAD, False),
    ("eligible_1x1/nothing_requires_grad", "eligible_1x1", lambda: (_conv(k=1, frozen=True),), dict(grad=False), {}, None, False),
    ("eligible_1x1/autocast", "eligible_1x1", lambda: (_conv(k=1),), {}, {}, AUTOCAST, False),
    ("eligible_1x1/nchw", "eligible_1x1", lambda: (_conv(k=1),), dict(cl=False), {}, None, False),
    ("eligible_1x1/hw1", "eligible_1x1", lambda: (_conv(k=1),), dict(shape=(2, 32, 1, 1)), {}, None, False),
    ("eligible_1x1/cin24_is_taken", "eligible_1x1", lambda: (_conv(24, k=1),), dict(shape=(2, 24, 8, 8)), {}, None, True),   # `linear` route
    ("eligible_1x1/CONV=0", "eligible_1x1", lambda: (_conv(k=1),), {}, dict(SRF_TRAIN_CONV="0"), None, False),
    ("eligible_1x1/CONV1X1=0_not_consulted", "eligible_1x1", lambda: (_conv(k=1),), {}, dict(SRF_TRAIN_CONV1X1="0"), None, True),
    # eligible_depthwise
    ("eligible_depthwise/accepted", "eligible_depthwise", lambda: (_conv(groups=32, stride=2),), {}, {}, None, True),
    ("eligible_depthwise/no_grad_mode", "eligible_depthwise", lambda: (_conv(groups=32, stride=2),), {}, {}, NOGRAD, False),
    ("eligible_depthwise/nothing_requires_grad", "eligible_depthwise", lambda: (_conv(groups=32, frozen=True),), dict(grad=False), {}, None, False),
    ("eligible_depthwise/autocast_not_looked_at", "eligible_depthwise", lambda: (_conv(groups=32, stride=2),), {}, {}, AUTOCAST, True),   # difference
    ("eligible_depthwise/nchw_is_taken", "eligible_depthwise", lambda: (_conv(groups=32),), dict(cl=False), {}, None, True),
    ("eligible_depthwise/dense_conv", "eligible_depthwise", lambda: (_conv(),), {}, {}, None, False),
    ("eligible_depthwise/CONV=0", "eligible_depthwise", lambda: (_conv(groups=32),), {}, dict(SRF_TRAIN_CONV="0"), None, False),
    # fused_eligible: conv -> eval BatchNorm (-> ReLU) on `_ConvAffineRelu`
    ("fused/accepted_3x3", "fused_eligible", lambda: (_conv(), _bn()), {}, {}, None, True),
    ("fused/accepted_1x1", "fused_eligible", lambda: (_conv(k=1), _bn()), {}, {}, None, True),
    ("fused/no_grad_mode", "fused_eligible", lambda: (_conv(), _bn()), {}, {}, NOGRAD, False),
    ("fused/nothing_requires_grad", "fused_eligible", lambda: (_conv(frozen=True), _bn()), dict(grad=False), {}, None, False),
    ("fused/autocast", "fused_eligible", lambda: (_conv(), _bn()), {}, {}, AUTOCAST, False),
    ("fused/nchw_3x3", "fused_eligible", lambda: (_conv(), _bn()), dict(cl=False), {}, None, False),
    ("fused/nchw_1x1", "fused_eligible", lambda: (_conv(k=1), _bn()), dict(cl=False), {}, None, False),
    ("fused/train_mode_bn", "fused_eligible", lambda: (_conv(), _bn(train=True)), {}, {}, None, False),
    ("fused/bn_without_affine", "fused_eligible", lambda: (_conv(), _bn(affine=False)), {}, {}, None, False),
    ("fused/cin24_3x3", "fused_eligible", lambda: (_conv(24), _bn()), dict(shape=(2, 24, 8, 8)), {}, None, False),
    ("fused/cin24_1x1", "fused_eligible", lambda: (_conv(24, k=1), _bn()), dict(shape=(2, 24, 8, 8)), {}, None, False),
    ("fused/cout1056_1x1", "fused_eligible", lambda: (_conv(32, 1056, k=1), _bn(1056)), {}, {}, None, False),
    ("fused/cout48_1x1", "fused_eligible", lambda: (_conv(32, 48, k=1), _bn(48)), {}, {}, None, False),
    ("fused/hw1_1x1", "fused_eligible", lambda: (_conv(k=1), _bn()), dict(shape=(2, 32, 1, 1)), {}, None, False),
    ("fused/hw1_3x3_is_taken", "fused_eligible", lambda: (_conv(), _bn()), dict(shape=(2, 32, 1, 1)), {}, None, True),
    ("fused/CONV=0", "fused_eligible", lambda: (_conv(), _bn()), {}, dict(SRF_TRAIN_CONV="0"), None, False),
    ("fused/FUSED=0_left_to_the_caller", "fused_eligible", lambda: (_conv(), _bn()), {}, dict(SRF_TRAIN_FUSED="0"), None, True),
    # dense._train_fusable, that caller
    ("dense/accepted", "_train_fusable", lambda: (), {}, {}, None, True),
    ("dense/no_grad_mode", "_train_fusable", lambda: (), {}, {}, NOGRAD, False),
    ("dense/autocast", "_train_fusable", lambda: (), {}, {}, AUTOCAST, False),
    ("dense/FUSED=0", "_train_fusable", lambda: (), {}, dict(SRF_TRAIN_FUSED="0"), None, False),
    ("dense/CONV=0_not_consulted", "_train_fusable", lambda: (), {}, dict(SRF_TRAIN_CONV="0"), None, True),                    # difference
    ("dense/nchw_and_3d_are_taken", "_train_fusable", lambda: (), dict(shape=(2, 32, 8), cl=False), {}, None, True),
    # osa_eligible: an OSA block on `_OSAChain`
    ("osa/accepted", "osa_eligible", lambda: (_osa(),), {}, {}, None, True),
    ("osa/no_grad_mode", "osa_eligible", lambda: (_osa(),), {}, {}, NOGRAD, False),
    ("osa/nothing_requires_grad", "osa_eligible", lambda: (_osa(frozen=True),), dict(grad=False), {}, None, False),
    ("osa/frozen_block_behind_a_gradient", "osa_eligible", lambda: (_osa(frozen=True),), {}, {}, None, True),
    ("osa/autocast", "osa_eligible", lambda: (_osa(),), {}, {}, AUTOCAST, False),
    ("osa/nchw", "osa_eligible", lambda: (_osa(),), dict(cl=False), {}, None, False),
    ("osa/train_mode_bn", "osa_eligible", lambda: (_osa(train=True),), {}, {}, None, False),
    ("osa/biased_layer", "osa_eligible", lambda: (_osa(biased=True),), {}, {}, None, False),
    ("osa/depthwise_reduction_block", "osa_eligible", lambda: (_osa(32, 64, depthwise=True),), {}, {}, None, False),
    ("osa/cin24", "osa_eligible", lambda: (_osa(24, 32),), dict(shape=(2, 24, 8, 8)), {}, None, False),
    ("osa/width36", "osa_eligible", lambda: (_osa(32, 36, 64),), {}, {}, None, False),
    ("osa/concat_cout48_no_multiple_of_32", "osa_eligible", lambda: (_osa(32, 32, 48),), {}, {}, None, False),
    ("osa/hw1", "osa_eligible", lambda: (_osa(),), dict(shape=(2, 32, 1, 1)), {}, None, False),
    ("osa/OSA=0", "osa_eligible", lambda: (_osa(),), {}, dict(SRF_TRAIN_OSA="0"), None, False),
    ("osa/FUSED=0", "osa_eligible", lambda: (_osa(),), {}, dict(SRF_TRAIN_FUSED="0"), None, False),
    ("osa/CONV=0_left_to_the_caller", "osa_eligible", lambda: (_osa(),), {}, dict(SRF_TRAIN_CONV="0"), None, True),            # difference
    # ese_eligible: (module, x, identity); identity rows build it from the same tensor keywords
    ("ese/accepted", "ese_eligible", lambda: (_ese(),), {}, {}, None, True),
    ("ese/accepted_with_identity", "ese_eligible", lambda: (_ese(), dict()), {}, {}, None, True),
    ("ese/no_grad_mode", "ese_eligible", lambda: (_ese(),), {}, {}, NOGRAD, False),
    ("ese/nothing_requires_grad", "ese_eligible", lambda: (_ese().requires_grad_(False),), dict(grad=False), {}, None, False),
    ("ese/autocast", "ese_eligible", lambda: (_ese(),), {}, {}, AUTOCAST, False),
    ("ese/nchw", "ese_eligible", lambda: (_ese(),), dict(cl=False), {}, None, False),
    ("ese/nchw_identity", "ese_eligible", lambda: (_ese(), dict(cl=False)), {}, {}, None, False),
    ("ese/cin24_is_taken", "ese_eligible", lambda: (_ese(24),), dict(shape=(2, 24, 8, 8)), {}, None, True),
    ("ese/c30", "ese_eligible", lambda: (_ese(30),), dict(shape=(2, 30, 8, 8)), {}, None, False),
    ("ese/hw1_is_taken", "ese_eligible", lambda: (_ese(),), dict(shape=(2, 32, 1, 1)), {}, None, True),
    ("ese/CONV=0", "ese_eligible", lambda: (_ese(),), {}, dict(SRF_TRAIN_CONV="0"), None, False),
    ("ese/ESE=0", "ese_eligible", lambda: (_ese(),), {}, dict(SRF_TRAIN_ESE="0"), None, False),
    # bn_eval: the verdict is which of its two routes runs
    ("bn_eval/accepted", "bn_eval", lambda: (_bn(8),), dict(shape=(2, 8, 4, 4)), {}, None, True),
    ("bn_eval/no_grad_mode", "bn_eval", lambda: (_bn(8),), dict(shape=(2, 8, 4, 4)), {}, NOGRAD, False),
    ("bn_eval/requires_grad_not_looked_at", "bn_eval", lambda: (_bn(8).requires_grad_(False),), dict(shape=(2, 8, 4, 4), grad=False), {}, None, True),
    ("bn_eval/autocast", "bn_eval", lambda: (_bn(8),), dict(shape=(2, 8, 4, 4)), {}, AUTOCAST, False),
    ("bn_eval/nchw_is_taken", "bn_eval", lambda: (_bn(8),), dict(shape=(2, 8, 4, 4), cl=False), {}, None, True),
    ("bn_eval/dim_not_looked_at", "bn_eval", lambda: (_bn(8),), dict(shape=(8, 4, 4)), {}, None, True),                        # difference
    ("bn_eval/train_mode_bn", "bn_eval", lambda: (_bn(8, train=True),), dict(shape=(2, 8, 4, 4)), {}, None, False),
    ("bn_eval/no_running_stats", "bn_eval", lambda: (_bn(8, track_running_stats=False),), dict(shape=(2, 8, 4, 4)), {}, None, False),
    ("bn_eval/CONV=0", "bn_eval", lambda: (_bn(8),), dict(shape=(2, 8, 4, 4)), dict(SRF_TRAIN_CONV="0"), None, False),
]

_SWITCHES = ("SRF_TRAIN_CONV", "SRF_TRAIN_FUSED", "SRF_TRAIN_OSA", "SRF_TRAIN_ESE", "SRF_TRAIN_CONV1X1", "SRF_TRAIN_WGRAD")


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.pop(k, None) for k in _SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in _SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class _Fallback(Exception):
    pass


def _bn_eval_route(tc, bn, y):
    """True: bn_eval ran its affine map; False: it went on to the module (stopped at `bn_train_input`, before any BatchNorm kernel)."""
    def stop(bn, y):
        raise _Fallback
    keep, tc.bn_train_input = tc.bn_train_input, stop
    try:
        tc.bn_eval(bn.to(y.device), y)
        return True
    except _Fallback:
        return False
    finally:
        tc.bn_train_input = keep


def verdict(tc, dense, dev, row):
    """The verdict of row's predicate, taken from the modules `tc` (train_conv) and `dense`."""
    _, pred, layers, tensor, env, ctx, _ = row
    torch.manual_seed(0)
    mods = layers()
    x = _x(dev, **tensor)
    with _environment(env), (torch.no_grad() if ctx == NOGRAD else torch.autocast("cuda") if ctx == AUTOCAST else contextlib.nullcontext()):
        if pred == "_train_fusable":
            return bool(dense._train_fusable(x))
        if pred == "bn_eval":
            return _bn_eval_route(tc, mods[0], x)
        if pred == "ese_eligible":
            identity = _x(dev, **{**tensor, **mods[1]}) if len(mods) > 1 else None
            return bool(tc.ese_eligible(mods[0], x, identity))
        return bool(getattr(tc, pred)(*mods, x))


def test_every_predicate_has_an_accepted_row_and_the_ids_are_unique():
    assert len({r[0] for r in ROWS}) == len(ROWS)
    for pred in ("eligible", "eligible_1x1", "eligible_depthwise", "fused_eligible", "osa_eligible", "ese_eligible", "bn_eval", "_train_fusable"):
        assert any(r[1] == pred and r[6] for r in ROWS) and any(r[1] == pred and not r[6] for r in ROWS), pred


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_gate_verdict(dev, row):
    from srfdet3d_amd import dense, train_conv
    assert verdict(train_conv, dense, dev, row) is row[6]
