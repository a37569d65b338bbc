"""Every route that runs on a tensor derived from a module's weights (derived.py), held to one statement: the cache is a cache until
`nhwc.invalidate_caches`, and after it the route computes what a fresh copy of the updated module computes, bit for bit.  Then the
same through `SRFDet.weights_changed()` on a graphed model."""
import copy
import gc

import numpy as np
import pytest
import torch
from torch import nn

from srfdet3d_amd import dense, derived, nhwc, sparse, synthetic as S, workloads
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
from srfdet3d_amd.compat.dcn import ModulatedDeformConv2dPack

pytestmark = pytest.mark.gpu


def _bn(cls, c, seed):
    g = torch.Generator().manual_seed(seed)
    bn = cls(c, eps=1e-3).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


def _scale(p):
    p.data.mul_(2.0)


# Each case: dev -> (holder: the modules of the route, run(holder) -> output, param(holder): the tensor to update, update(param)).
def _wino(dev):
    x = torch.randn(1, 8, 12, 8, device=dev)
    return nn.ModuleList([nn.Conv2d(8, 8, 3, padding=1)]), lambda h: nhwc.conv3x3(x, h[0]), lambda h: h[0].weight, _scale


def _wino43(dev):
    x = torch.randn(1, 8, 12, 96, device=dev)
    return nn.ModuleList([nn.Conv2d(96, 32, 3, padding=1, bias=False)]), lambda h: nhwc.conv3x3(x, h[0]), lambda h: h[0].weight, _scale


def _gemm(dev):
    x = torch.randn(1, 8, 12, 32, device=dev)
    return nn.ModuleList([nn.Conv2d(32, 32, 1)]), lambda h: nhwc.conv1x1(x, h[0]), lambda h: h[0].weight, _scale


def _cgemm(dev):
    x = torch.randn(1, 8, 12, 32, device=dev)
    return nn.ModuleList([nn.Conv2d(32, 32, 3, stride=2, padding=1)]), lambda h: nhwc.conv_strided(x, h[0]), lambda h: h[0].weight, _scale


def _conv1x1_nchw(dev):
    xs = [torch.randn(1, 32, 4, 4, device=dev) for _ in range(2)]
    holder = nn.ModuleList([nn.Conv2d(64, 128, 1, bias=False), _bn(nn.BatchNorm2d, 128, 1)])
    return holder, lambda h: dense.conv1x1_cat_bn_act(h[0], h[1], False, xs), lambda h: h[0].weight, _scale


def _bn_fold_2d(dev):
    x = torch.randn(1, 8, 6, 6, device=dev)
    holder = nn.ModuleList([nn.Conv2d(8, 8, 3, padding=1, bias=False), _bn(nn.BatchNorm2d, 8, 2)])
    return holder, lambda h: dense.conv_bn_act(h[0], h[1], False, x), lambda h: h[1].weight, _scale


def _sparse(dev, cout, param):
    rng = np.random.default_rng(0)
    shape = [9, 24, 20]                                      # the small grid of test_gpu_spconv.py
    idx = torch.from_numpy(np.argwhere(rng.random((2, *shape)) < 0.15).astype(np.int32)).to(dev)
    feats = torch.randn(idx.shape[0], 16, device=dev)
    holder = nn.ModuleList([sparse.SubMConv3d(16, cout, 3), _bn(nn.BatchNorm1d, cout, 3)]).eval()
    return holder, lambda h: h[0](sparse.SparseConvTensor(feats, idx, shape, 2), bn=h[1], relu=False).features, param, _scale


def _bn_fold_1d(dev):
    return _sparse(dev, 16, lambda h: h[1].weight)


def _spconv(dev):
    """A layer shape that has a packed weight (16 -> 32), updating the weight."""
    return _sparse(dev, 32, lambda h: h[0].weight)


def _linear_padded(dev):
    x = torch.randn(2, 6, device=dev)
    return nn.ModuleList([nn.Linear(6, 8)]), lambda h: dense.linear_graph_safe(h[0], x), lambda h: h[0].weight, _scale


def _dcn(dev, which):
    x = torch.randn(1, 64, 10, 12, device=dev)               # the small shape of test_gpu_dcn.py's routing test
    holder = nn.ModuleList([ModulatedDeformConv2dPack(64, 64, 3, 1, 1).eval()])
    if which == "dcn":
        return holder, lambda h: h[0].forward_hip(x), lambda h: h[0].weight, _scale
    return holder, lambda h: h[0].forward_hip(x), lambda h: h[0].conv_offset.weight, lambda p: p.data.normal_()   # zero-initialised


CASES = {"wino": _wino, "wino43": _wino43, "gemm": _gemm, "cgemm": _cgemm, "conv1x1_nchw": _conv1x1_nchw, "bn_fold_2d": _bn_fold_2d,
         "bn_fold_1d": _bn_fold_1d, "spconv": _spconv, "linear_padded": _linear_padded, "dcn": lambda dev: _dcn(dev, "dcn"),
         "dcn_offset": lambda dev: _dcn(dev, "dcn_offset")}
# the entry the updated tensor feeds, where the case's name is not that entry
ENTRY = {"gemm": {"gemm", "gemm_direct", "gemm_split"}, "cgemm": {"cgemm", "cgemm_split"}, "bn_fold_2d": {"bn_fold"}, "bn_fold_1d": {"bn_fold"}}


@pytest.mark.parametrize("case", list(CASES))
def test_route_is_stale_until_invalidated_then_equals_a_fresh_copy(dev, case):
    torch.manual_seed(5)
    holder, run, param, update = CASES[case](dev)
    holder = holder.to(dev)
    with torch.no_grad():
        y0 = run(holder).clone()
        assert any(derived.names(m) & ENTRY.get(case, {case}) for m in holder.modules())    # the route went through the cache
        update(param(holder))                               # through `.data`: neither version nor pointer changes
        assert torch.equal(run(holder), y0)                 # the cache is a cache
        fresh = copy.deepcopy(holder)                       # new pointers: nothing cached applies to it
        nhwc.invalidate_caches(holder)
        y1 = run(holder).clone()
        want = run(fresh)
    assert torch.isfinite(y1).all()
    assert torch.equal(y1, want)
    assert not torch.equal(y1, y0)


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def test_weights_changed_reaches_the_batchnorm_folds_of_a_graphed_model(dev):
    """The model and sweep of test_graphs_are_recaptured_when_the_packed_weights_are_dropped.  Gamma of one BatchNorm1d of the sparse
    encoder and of one BatchNorm2d of SECOND halved through `.data`, then `weights_changed()`: the recaptured frame is the eager frame
    of a copy of the updated model (that test's bars), not the frame before the update."""
    torch.manual_seed(0)
    cpu = workloads.build("srfdet_voxel_nusc_L", 32).eval()
    _randomize_bn(cpu, 0)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 8000)).to(dev)
    g = copy.deepcopy(cpu).to(dev).enable_hip_graphs(whole_frame=True)
    with torch.no_grad():
        for _ in range(3):
            g.simple_test(None, [pts], copy.deepcopy(metas))
        first = g._graphed_frame
        assert first.stats["replays"] >= 1
        before = [first.entry["scores"].clone(), first.entry["boxes"].clone()]
        bn1 = next(m for m in g.pts_middle_encoder.modules() if isinstance(m, nn.BatchNorm1d))
        bn2 = next(m for m in g.pts_backbone.modules() if isinstance(m, nn.BatchNorm2d))
        assert "bn_fold" in derived.names(bn1) and "bn_fold" in derived.names(bn2)
        bn1.weight.data.mul_(0.5)
        bn2.weight.data.mul_(0.5)
        g.weights_changed()
        assert g._graphed_frame is not first and g._graphed_frame.entry is None
        assert not any(derived.names(m) for m in g.modules())
        eager = copy.deepcopy(cpu).to(dev)                  # a copy of the updated model: new tensors, nothing derived yet
        eager.load_state_dict(g.state_dict())
        f = eager.extract_point_features([pts])
        want = [t.clone() for t in eager.bbox_head.decode(*eager.bbox_head(None, f, metas))]
        del eager
        for _ in range(3):
            g.simple_test(None, [pts], copy.deepcopy(metas))
        e = g._graphed_frame.entry
        assert g._graphed_frame.stats["replays"] >= 1
        torch.testing.assert_close(e["scores"], want[0], rtol=0, atol=1e-5)
        torch.testing.assert_close(e["boxes"], want[1], rtol=2e-5, atol=1e-4)
        moved = (e["scores"] - before[0]).abs().max().item()
        print(f"\nscores moved by {moved:.3e} with the two halved gammas")
        assert moved > 1e-5                                 # not vacuous: the update is visible in the frame at that test's bar
        stray = sorted({k for m in g.modules() for k in m.__dict__ if k.startswith("_srf_")} - {"_srf_derived", "_srf_level_consumer"})
        assert stray == []
    g._graphed_frame = g._graphed_img = g._graphed_tail = None
    del g
    gc.collect()
    torch.cuda.empty_cache()
