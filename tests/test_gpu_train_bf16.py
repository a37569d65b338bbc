"""The bf16-product mode of the training convolutions (train_conv.mfma_dtype, SRFDet.train_mfma_dtype): the nodes of train_conv.py in
the mode against tests/train_bf16_ref.py -- float64 with every convolution operand rounded to bf16 in all three directions -- on the
shapes and within the figures tests/test_gpu_training.py uses for the f32 nodes; the record a node keeps of the mode; the reports; the
switch on the LiDAR + camera model."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import train_bf16_ref as R
from srfdet3d_amd import dense, ops, synthetic as S, train_conv, training, workloads
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _conv_bn(dev, k, Cin, Cout, bias):
    g = torch.Generator().manual_seed(k * 100 + Cin)
    torch.manual_seed(k * 100 + Cin)
    conv = nn.Conv2d(Cin, Cout, k, padding=k // 2, bias=bias).to(dev)
    bn = nn.BatchNorm2d(Cout, eps=1e-3).to(dev)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Cout, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(Cout, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.5)
    return conv, bn.eval(), g


def _d(t):
    return t.detach().double().cpu()


@pytest.mark.parametrize("k,N,Cin,Cout,H,W,relu,bias", [(3, 2, 192, 192, 29, 50, True, False), (3, 1, 160, 224, 13, 21, False, True),
                                                        (1, 2, 1472, 768, 29, 25, True, False), (1, 3, 64, 96, 17, 9, True, True)])
def test_conv_affine_relu_node_in_the_mode(dev, k, N, Cin, Cout, H, W, relu, bias):
    """`_ConvAffineRelu` (the shapes of test_gpu_training.py:313): y, dx, dW, d gamma, d beta, d bias within 2e-5 of the largest reference
    value.  Two places where float64 cannot say what the f32 node must do are taken from the node, each only within f32 rounding
    (tests/train_bf16_ref.py): the side of the ReLU where the reference's output lies within those 2e-5 of zero, and the f32 gradient the
    BatchNorm / ReLU backward pass hands the convolution, which the mode rounds ONCE to bf16.  Rounded from the reference's float64
    gradient instead, dx and dW of 1472 -> 768 were 1.25e-4 and 1.09e-4 off (a value one f32 ulp beside a bf16 rounding boundary moves
    by 2^-9, and the gradient sums 1450 pixels), every other figure of the four cases below 1.4e-6."""
    conv, bn, g = _conv_bn(dev, k, Cin, Cout, bias)
    x = torch.randn(N, Cin, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = torch.randn(N, Cout, H, W, generator=g).to(dev)
    routes = []
    with train_conv.mfma_dtype(BF16, routes=routes):
        y = dense.conv_bn_act(conv, bn, relu, x)
    assert type(y.grad_fn).__name__ == "_ConvAffineReluBackward"
    y.backward(gy)
    assert [(r["direction"], r["route"]) for r in routes] == [("fwd", "bf16"), ("dgrad", "bf16"), ("wgrad", "bf16")]
    got = [y.detach(), x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad] + ([conv.bias.grad] if bias else [])
    xd, wd = _d(x).requires_grad_(True), _d(conv.weight).requires_grad_(True)
    bd = _d(conv.bias).requires_grad_(True) if bias else None
    gam, bet = _d(bn.weight).requires_grad_(True), _d(bn.bias).requires_grad_(True)
    # the f32 tensor the convolution's two gradient products receive: the unchanged f32 head of the backward pass on the node's output
    fold = ops.bn_eval_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
    gz = ops.nhwc_affine_relu_bwd(train_conv._nhwc(gy), y.detach().permute(0, 2, 3, 1), fold[0], relu)[0].permute(0, 3, 1, 2)
    yr = R.conv_bn_relu(xd, wd, bd, gam, bet, _d(bn.running_mean), _d(bn.running_var), bn.eps, relu, got=_d(y), tol=2e-5, g_operand=_d(gz))
    yr.backward(_d(gy))
    ref = [yr.detach(), xd.grad, wd.grad, gam.grad, bet.grad] + ([bd.grad] if bias else [])
    errs = {name: _rel(a, b) for name, a, b in zip(["y", "dx", "dW", "dgamma", "dbeta", "dbias"], got, ref)}
    print(f"_ConvAffineRelu {k}x{k} {Cin}->{Cout} @{N}x{H}x{W}: {errs}")
    for name, err in errs.items():
        assert err < 2e-5, (name, err)


@pytest.mark.parametrize("N,Cin,Cout,H,W,bias", [(2, 256, 128, 29, 50, True), (1, 512, 256, 13, 40, False)])
def test_conv1x1_node_in_the_mode(dev, N, Cin, Cout, H, W, bias):
    """`_Conv1x1` (the shapes of test_gpu_training.py:539) within 2e-5 of the largest reference value"""
    torch.manual_seed(Cin + Cout)
    conv = nn.Conv2d(Cin, Cout, 1, bias=bias).to(dev)
    x = torch.randn(N, Cin, H, W, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    g = torch.randn(N, Cout, H, W, device=dev)
    routes = []
    with train_conv.mfma_dtype(BF16, routes=routes):
        y = train_conv.conv2d(conv, x)
    assert type(y.grad_fn).__name__ == "_Conv1x1Backward" and y.stride(1) == 1
    y.backward(g)
    assert [(r["direction"], r["route"]) for r in routes] == [("fwd", "bf16"), ("dgrad", "bf16"), ("wgrad", "bf16")]
    got = [y.detach(), x.grad, conv.weight.grad] + ([conv.bias.grad] if bias else [])
    xd, wd = _d(x).requires_grad_(True), _d(conv.weight).requires_grad_(True)
    bd = _d(conv.bias).requires_grad_(True) if bias else None
    yr = R.conv(xd, wd, bd)
    yr.backward(_d(g))
    ref = [yr.detach(), xd.grad, wd.grad] + ([bd.grad] if bias else [])
    for name, a, b in zip(["y", "dx", "dW", "db"], got, ref):
        err = _rel(a, b)
        print(f"_Conv1x1 {Cin}->{Cout}: {name} {err:.3e}")
        assert err < 2e-5, (name, err)


def test_wino43_node_in_the_mode(dev):
    """`_Wino43Conv` (a 3x3 layer without a BatchNorm behind it) takes the mode too: no Winograd in it"""
    torch.manual_seed(5)
    conv = nn.Conv2d(64, 96, 3, padding=1).to(dev)
    x = torch.randn(2, 64, 13, 21, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    g = torch.randn(2, 96, 13, 21, device=dev)
    with train_conv.mfma_dtype(BF16) as m:
        y = train_conv.conv2d(conv, x)
    assert type(y.grad_fn).__name__ == "_Wino43ConvBackward"
    y.backward(g)
    assert m.launches == 3
    xd, wd, bd = _d(x).requires_grad_(True), _d(conv.weight).requires_grad_(True), _d(conv.bias).requires_grad_(True)
    yr = R.conv(xd, wd, bd)
    yr.backward(_d(g))
    for name, a, b in zip(["y", "dx", "dW", "db"], [y.detach(), x.grad, conv.weight.grad, conv.bias.grad], [yr.detach(), xd.grad, wd.grad, bd.grad]):
        assert _rel(a, b) < 2e-5, (name, _rel(a, b))


@pytest.mark.parametrize("cin,width,cout,L,N,H,W,identity", [(64, 32, 96, 3, 2, 21, 34, False), (96, 64, 96, 2, 1, 17, 40, True)])
def test_osa_chain_in_the_mode(dev, cin, width, cout, L, N, H, W, identity):
    """`_OSAChain` in the mode and the per-layer nodes in the mode (SRF_TRAIN_OSA=0), both against the rounding reference, under the rule
    of test_gpu_training.py:508: an element within rounding of zero takes the other side of a ReLU than float64 does and the chained
    layers pass that on, so the node must not be worse than the per-layer nodes are on the same data."""
    from srfdet3d_amd.plugin.vovnet import OSAModule
    g = torch.Generator().manual_seed(cin + 7 * L)
    torch.manual_seed(cin + 7 * L)
    blk = OSAModule(cin, width, cout, L, "OSAt_1", identity=identity).to(dev)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.3 + 0.1)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            elif isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (m.in_channels * m.kernel_size[0] ** 2)) ** 0.5)
    blk.train()
    for m in blk.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    x = torch.randn(N, cin, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = torch.randn(N, cout, H, W, generator=g).to(dev)
    params = list(blk.parameters())
    names = [n for n, _ in blk.named_parameters()]

    def run(nodes):
        for p in params:
            p.grad = None
        x.grad = None
        routes = []
        with train_conv.mfma_dtype(BF16, routes=routes):
            y = blk(x)
        y.backward(gy)                       # outside the context
        assert nodes in {type(f[0]).__name__ for f in _graph(y.grad_fn)}
        assert routes and all(r["route"] == "bf16" for r in routes), routes
        assert {r["direction"] for r in routes} == {"fwd", "dgrad", "wgrad"} and len(routes) == 3 * (L + 1)
        return [y.detach(), x.grad.clone()] + [p.grad.clone() for p in params]

    got = run("_OSAChainBackward")
    os.environ["SRF_TRAIN_OSA"] = "0"
    try:
        per_layer = run("_ConvAffineReluBackward")
    finally:
        del os.environ["SRF_TRAIN_OSA"]
    # the rounding reference: float64, every convolution through train_bf16_ref
    xd = _d(x).requires_grad_(True)
    named = {n: _d(p).requires_grad_(True) for n, p in zip(names, params)}

    def cbr(seq, prefix, inp):
        bn = seq[1]
        pick = lambda tail: named[[n for n in names if n.startswith(prefix) and n.endswith(tail)][0]]
        return R.conv_bn_relu(inp, pick("conv.weight"), None, pick("norm.weight"), pick("norm.bias"), _d(bn.running_mean), _d(bn.running_var), bn.eps, True)

    feats, cur = [xd], xd
    for i, seq in enumerate(blk.layers):
        cur = cbr(seq, f"layers.{i}.", cur)
        feats.append(cur)
    out = cbr(blk.concat, "concat.", torch.cat(feats, 1))
    gate = F.relu6(F.conv2d(out.mean(dim=(2, 3), keepdim=True), named["ese.fc.weight"], named["ese.fc.bias"]) + 3.0) / 6.0
    yr = out * gate + (xd if identity else 0.0)
    yr.backward(_d(gy))
    ref = [yr.detach(), xd.grad] + [named[n].grad for n in names]
    for name, a, b, c in zip(["y", "dx"] + names, got, ref, per_layer):
        err, err_pl = _rel(a, b), _rel(c, b)
        print(f"_OSAChain {name}: node {err:.3e}, per-layer nodes {err_pl:.3e}")
        assert err < 2e-2 and err < max(1.5 * err_pl, 5e-4), (name, err, err_pl)


def _graph(fn, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return []
    seen.add(fn)
    out = [(fn,)]
    for nxt, _ in fn.next_functions:
        out += _graph(nxt, seen)
    return out


def _layer(dev, Cin=64, Cout=96, k=3, N=2, H=9, W=40):
    conv, bn, g = _conv_bn(dev, k, Cin, Cout, False)
    x = torch.randn(N, Cin, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = torch.randn(N, Cout, H, W, generator=g).to(dev)
    return conv, bn, x, gy


def _step(conv, bn, x, gy, ctx=None, backward_inside=False):
    conv.weight.grad = bn.weight.grad = bn.bias.grad = x.grad = None
    if ctx is None:
        y = dense.conv_bn_act(conv, bn, True, x)
        y.backward(gy)
    else:
        with ctx:
            y = dense.conv_bn_act(conv, bn, True, x)
            if backward_inside:
                y.backward(gy)
        if not backward_inside:
            y.backward(gy)
    return [y.detach().clone(), x.grad.clone(), conv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()]


def test_backward_follows_the_mode_of_its_forward_and_a_closed_context_leaves_no_trace(dev):
    layer = _layer(dev)
    never = _step(*layer)                                                   # before any context was opened
    r_in, r_out = [], []
    inside = _step(*layer, ctx=train_conv.mfma_dtype(BF16, routes=r_in), backward_inside=True)
    outside = _step(*layer, ctx=train_conv.mfma_dtype(BF16, routes=r_out))  # backward after the context has closed
    assert r_in == r_out and [(r["direction"], r["route"]) for r in r_out] == [("fwd", "bf16"), ("dgrad", "bf16"), ("wgrad", "bf16")]
    for a, b in zip(inside, outside):
        assert torch.equal(a, b)
    assert not torch.equal(inside[0], never[0]) and not torch.equal(inside[2], never[2])     # it IS another arithmetic
    # a forward pass outside the context inside whose backward ... a context is open: f32 all the way
    conv, bn, x, gy = layer
    y = dense.conv_bn_act(conv, bn, True, x)
    conv.weight.grad = bn.weight.grad = bn.bias.grad = x.grad = None
    with train_conv.mfma_dtype(BF16) as m:
        y.backward(gy)
    assert m.launches == 0 and torch.equal(conv.weight.grad, never[2]) and torch.equal(x.grad, never[1])
    after = _step(*layer)
    for a, b in zip(after, never):
        assert torch.equal(a, b)                                            # bit for bit the run that never opened it
    assert train_conv.mfma_dtype.active() is None


def test_routes_of_a_layer_the_bf16_gemms_refuse(dev):
    """48 input channels: forward (K = 48) and with it the data gradient keep the f32 route; the weight-gradient kernel takes the layer"""
    conv, bn, x, gy = _layer(dev, Cin=48, Cout=64)
    f32 = _step(conv, bn, x, gy)
    routes = []
    got = _step(conv, bn, x, gy, ctx=train_conv.mfma_dtype(BF16, routes=routes))
    name = "48->64 3x3 @2x9x40"
    why = "input or output channels are no multiple of 32"
    assert routes == [dict(layer=name, direction="fwd", route="f32", why=why), dict(layer=name, direction="dgrad", route="f32", why=why),
                      dict(layer=name, direction="wgrad", route="bf16", why=None)]
    assert torch.equal(got[0], f32[0]) and torch.equal(got[1], f32[1]) and not torch.equal(got[2], f32[2])
    assert not train_conv.bf16_layer_ok(3, 2, 9, 40, 48, 64) and train_conv.bf16_layer_ok(3, 2, 9, 40, 64, 64)


# ---- the switch on the model ------------------------------------------------------------------------------------------
def _gt(dev, n=12, seed=0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-40, 40, (n, 2))
    z = rng.uniform(-2.5, 0.0, (n, 1))
    size = rng.uniform(1.0, 5.0, (n, 3))
    t = torch.tensor(np.concatenate([xy, z, size, rng.uniform(-3.1, 3.1, (n, 1)), rng.normal(0, 1, (n, 2))], 1), dtype=torch.float32, device=dev)
    return LiDARInstance3DBoxes(t, box_dim=9), torch.from_numpy(rng.integers(0, 10, n)).to(dev)


def _lc_inputs(dev):
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 8000)).to(dev)
    img = torch.from_numpy(S.camera_images(3000, h=128, w=224)).to(dev)
    gtb, gtl = _gt(dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig(f=177.0, cx=112.0, cy=64.0)])]
    return dict(img=img, points=[pts], img_metas=metas, gt_bboxes_3d=[gtb], gt_labels_3d=[gtl])


CHECKED = ("bbox_head.head_series_lidar.0.output_fused_proj.weight", "bbox_head.img_convs.0.weight", "img_neck.fpn_convs.0.conv.weight",
           "img_backbone.stage5.OSA5_3.concat.OSA5_3_concat/conv.weight", "bbox_head.dpg_fc1_img.weight")


def test_train_mfma_dtype_on_the_lidar_camera_model(dev):
    """`test_lc_training_step` with the switch, on its 128 x 224 images (the weight-gradient kernel takes maps of any width, so the report
    shows bf16 in all three directions there).  The bit-for-bit comparisons drive the image backbone + neck -- the scope of the switch --
    with fixed output gradients: the whole step feeds them through the RoI gather's float-atomic backward pass, whose bits differ from
    run to run in f32 as well.  A parameter whose gradient already differs between two f32 passes that never saw the switch (48 of 256
    when this was written; in f32, maps narrower than 32 pixels take the library's weight gradient, which adds with float atomics) cannot
    be compared bit for bit and is left out by that measurement."""
    torch.manual_seed(0)
    model = workloads.build("srfdet_voxel_nusc_LC", 64, train=True)
    training.freeze_lidar_components(model)
    model = model.to(dev).train()
    assert model.train_mfma_dtype is None
    inp = _lc_inputs(dev)
    named = dict(model.named_parameters())
    branch = {n: p for n, p in named.items() if p.requires_grad and n.startswith(("img_backbone.", "img_neck."))}
    gen = torch.Generator().manual_seed(1)

    def branch_grads():
        model.zero_grad(set_to_none=True)
        np.random.seed(0)                       # GridMask draws from numpy
        feats = model.extract_img_feat(inp["img"], inp["img_metas"])
        if not hasattr(branch_grads, "w"):
            branch_grads.w = [torch.randn(f.shape, generator=gen).to(dev) for f in feats]
        sum((f * w).sum() for f, w in zip(feats, branch_grads.w)).backward()
        return [f.detach().clone() for f in feats], {n: p.grad.clone() for n, p in branch.items() if p.grad is not None}

    f_a, g_a = branch_grads()
    f_a2, g_a2 = branch_grads()
    stable = [n for n in g_a if torch.equal(g_a[n], g_a2[n])]
    assert all(torch.equal(a, b) for a, b in zip(f_a, f_a2)) and len(stable) > 0, (len(stable), len(g_a))
    print(f"f32 gradients that repeat bit for bit: {len(stable)} of {len(g_a)} parameters")

    # the four error cases of the switch
    with pytest.raises(ValueError):
        model.train_mfma_dtype = torch.float16
    model.img_autocast_dtype = torch.bfloat16
    with pytest.raises(ValueError):
        model.train_mfma_dtype = BF16
    model.img_autocast_dtype = None
    model.train_mfma_dtype = BF16
    model.img_autocast_dtype = torch.bfloat16
    with pytest.raises(ValueError):
        model.extract_img_feat(inp["img"], inp["img_metas"])
    model.img_autocast_dtype = None
    os.environ["SRF_TRAIN_CONV"] = "0"          # no node of train_conv.py runs: nothing can take a bf16 route
    try:
        with pytest.raises(RuntimeError):
            model.extract_img_feat(inp["img"], inp["img_metas"])
    finally:
        del os.environ["SRF_TRAIN_CONV"]
    with torch.no_grad():                       # a no-grad pass ignores the switch
        np.random.seed(0)
        model.train_mfma_routes = []
        model.extract_img_feat(inp["img"], inp["img_metas"])
        assert model.train_mfma_routes == []

    # in the mode: the report, two identical passes, the whole step
    f_b, g_b = branch_grads()
    report = list(model.train_mfma_routes)
    f_b2, g_b2 = branch_grads()
    took = {(r["direction"], r["route"]) for r in report}
    assert {("fwd", "bf16"), ("dgrad", "bf16"), ("wgrad", "bf16")} <= took, took
    assert set(g_b) == set(g_a) and all(torch.equal(a, b) for a, b in zip(f_b, f_b2))
    for n in stable:
        assert torch.equal(g_b[n], g_b2[n]), n
    assert not all(torch.equal(g_a[n], g_b[n]) for n in stable)
    groups = {}
    for n in g_a:
        key = ".".join(n.split(".")[:2])
        d, r = groups.setdefault(key, [0.0, 0.0])
        groups[key] = [d + float((g_b[n] - g_a[n]).double().pow(2).sum()), r + float(g_a[n].double().pow(2).sum())]
    for key, (d, r) in sorted(groups.items()):
        print(f"train_mfma_dtype: relative RMS difference of the gradients to f32, {key}: {(d / max(r, 1e-300)) ** 0.5:.3e}")
    print("train_mfma_dtype routes:", {k: sum(1 for r in report if (r["direction"], r["route"]) == k) for k in sorted(took)})

    model.zero_grad(set_to_none=True)
    np.random.seed(0)
    losses = model(return_loss=True, **inp)
    total = sum(losses.values())
    assert torch.isfinite(total) and all(torch.isfinite(v).all() for v in losses.values())
    total.backward()
    for k in CHECKED:
        gk = named[k].grad
        assert gk is not None and torch.isfinite(gk).all() and gk.abs().sum() > 0, k

    # off again: the f32 pass, bit for bit
    model.train_mfma_dtype = None
    f_c, g_c = branch_grads()
    assert all(torch.equal(a, b) for a, b in zip(f_a, f_c))
    for n in stable:
        assert torch.equal(g_c[n], g_a[n]), n
