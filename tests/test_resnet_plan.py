"""The plan of the channels-last executor for the bottleneck ResNets (`nhwc.resnet_plan`, `resnet_shapes`) and its verdicts, in the
form tests/test_nhwc_gate.py uses: meta tensors, `fusable` stubbed to true, so that the structure of the network and the shape limits
decide.  CPU only."""
import functools

import pytest

import make_nhwc_gate as gen
from srfdet3d_amd import nhwc, ops
from srfdet3d_amd.compat.resnet import ResNet

DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)


@functools.lru_cache(maxsize=None)
def r50():
    return ResNet(50, style="pytorch", frozen_stages=1).eval()


@functools.lru_cache(maxsize=None)
def r101_dcn():
    return ResNet(101, style="caffe", dcn=DCN, stage_with_dcn=(False, False, True, True)).eval()


def _count(plan):
    kinds = [s.kind for s in plan]
    return {k: kinds.count(k) for k in set(kinds)}


def test_the_plan_of_r50():
    plan = nhwc.resnet_plan(r50())
    assert _count(plan) == dict(stem7=1, pool_p1=1, conv1=16, conv2=16, conv3=16, down=4, out=4)
    assert len([s for s in plan if s.kind != "out"]) == 1 + 1 + 16 * 3 + 4
    assert [s.kind for s in plan[:7]] == ["stem7", "pool_p1", "conv1", "conv2", "down", "conv3", "conv1"]
    assert [s.arg for s in plan if s.kind == "conv3"] == [True, False, False] + [True] + [False] * 3 + [True] + [False] * 5 + [True, False, False]
    # pytorch style: the stride sits on the 3x3
    assert [s.conv.stride for s in plan if s.kind == "conv1"] == [(1, 1)] * 16
    assert [s.conv.stride for s in plan if s.kind == "conv2"].count((2, 2)) == 3


def test_the_shape_walk_of_r50_at_928x1600():
    steps = nhwc.resnet_shapes(nhwc.resnet_plan(r50()), 928, 1600, 6)
    assert steps[0][1] == (464, 800, 64, 0, 64)
    assert steps[1][1] == (232, 400, 64, 0, 64)
    outs = [slot for s, slot in steps if s.kind == "out"]
    assert [tuple(o[:3]) for o in outs] == [(232, 400, 256), (116, 200, 512), (58, 100, 1024), (29, 50, 2048)]
    # a downsample branch and the conv3 it feeds write maps of one size
    for (a, sa), (b, sb) in zip(steps, steps[1:]):
        if a.kind == "down":
            assert b.kind == "conv3" and sa == sb
    # odd maps all the way down
    outs = [slot[:2] for s, slot in nhwc.resnet_shapes(nhwc.resnet_plan(r50()), 70, 102) if s.kind in ("stem7", "out")]
    assert outs == [(35, 51), (18, 26), (9, 13), (5, 7), (3, 4)]


def test_the_plan_of_r101_caffe_with_dcn():
    plan = nhwc.resnet_plan(r101_dcn())
    c = _count(plan)
    assert c["conv3"] == 33 and c["dcn"] == 26 and c["conv2"] == 7 and c["down"] == 4 and c["out"] == 4
    # caffe style: the stride sits on conv1, every 3x3 / DCN runs at stride 1
    assert [s.conv.stride for s in plan if s.kind == "conv1"].count((2, 2)) == 3
    assert all(s.conv.stride == (1, 1) for s in plan if s.kind == "conv2") and all(s.conv.stride == 1 for s in plan if s.kind == "dcn")
    stages = [i for i, s in enumerate(plan) if s.kind == "out"]
    assert all(s.kind != "dcn" for s in plan[:stages[1]]) and all(s.kind != "conv2" for s in plan[stages[1]:])


# (network, input shape or None for the plan alone, environment, verdict, reason)
VERDICTS = [
    ("R-50 1x3x64x96", r50, (1, 3, 64, 96), {}, True, ""),
    ("R-50 6x3x928x1600", r50, (6, 3, 928, 1600), {}, True, "one nuScenes frame"),
    ("R-101-DCN 5x3x64x96", r101_dcn, (5, 3, 64, 96), {}, True, "the last DCN map is 2 x 3"),
    ("R-101-DCN 1x3x32x48", r101_dcn, (1, 3, 32, 48), {}, False, "stage 4 would sample a 1 x 2 map (ops.dcnv2_supported: H >= 2)"),
    ("R-50 1x3x4096x8192", r50, (1, 3, 4096, 8192), {}, False, "the stem's output of one image is 2048 x 4096 x 64 x 4 = 2^31 bytes: srf_stem_conv7_nchw "
     "would refuse it (ops.stem7_range_ok; the 128-channel input of layer2's 3x3 reaches 2^30 bytes at the same size)"),
    ("R-50 1x3x4096x8184", r50, (1, 3, 4096, 8184), {}, True, "2048 x 4092 x 256 bytes < 2^31, 1024 x 2046 x 512 < 2^30"),
    ("depth 18", lambda: ResNet(18).eval(), (1, 3, 64, 96), {}, False, "BasicBlock nets are not planned"),
    ("in_channels=5", lambda: ResNet(50, in_channels=5).eval(), (1, 5, 64, 96), {}, False, "ops.stem7_channels_ok: Cin > 4"),
    ("norm_eval=False in train mode", lambda: ResNet(50, norm_eval=False).train(), (1, 3, 64, 96), {}, False, "a BatchNorm in train mode is not foldable"),
    ("norm_eval=True in train mode", lambda: ResNet(50).train(), (1, 3, 64, 96), {}, True, "`ResNet.train()` leaves the BatchNorms in eval mode"),
    ("SRF_IMG_NHWC=0", r50, (1, 3, 64, 96), dict(SRF_IMG_NHWC="0"), False, "the A/B switch"),
    ("SRF_DCN=0 with DCN", r101_dcn, (5, 3, 64, 96), dict(SRF_DCN="0"), False, "the plan of a DCN network is None"),
    ("SRF_DCN=0 without DCN", r50, (1, 3, 64, 96), dict(SRF_DCN="0"), True, "no DCN in the net"),
    ("R-50 3x64x96 (no batch dimension)", r50, (3, 64, 96), {}, False, ""),
    ("R-50 1x4x64x96", r50, (1, 4, 64, 96), {}, False, "four planes into a three-plane stem"),
]


@pytest.mark.parametrize("row", VERDICTS, ids=[r[0] for r in VERDICTS])
def test_verdict(row, monkeypatch):
    _, net, shape, env, want, why = row
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x = gen.meta(*shape)
    with gen.stubbed():
        # the gate `ResNet.forward` asks: the switch, the tensor, the plan and its shapes
        got = nhwc.takes(x) and nhwc.resnet_supported(net(), x)
    assert bool(got) is want, why


def test_a_cpu_tensor_is_not_taken():
    import torch
    assert nhwc.resnet(r50(), torch.zeros(1, 3, 64, 96)) is None
    with pytest.raises(ValueError, match="resnet_supported"):
        nhwc.resnet_forward(ResNet(18).eval(), torch.zeros(1, 3, 64, 96))


def test_the_stem_range_is_held_by_the_shape_walk(monkeypatch):
    """Where no 3x3 buffer objects, the stem's own descriptor range still does: the walk answers None, it does not leave the refusal to the kernel."""
    plan = nhwc.resnet_plan(r50())
    monkeypatch.setattr(nhwc, "_img_fits", lambda H, W, ld: True)
    monkeypatch.setattr(ops, "below_2gb", lambda pixels, ld: True)      # (the 256-channel input of layer2's strided downsample objects at this size too)
    assert nhwc.resnet_shapes(plan, 4096, 8192) is None and nhwc.resnet_shapes(plan, 4096, 8190) is not None


def test_structures_the_plan_refuses():
    import torch
    from torch import nn
    net = ResNet(50).eval()
    assert nhwc.resnet_plan(net) is not None
    net.layer2[1].conv2.bias = nn.Parameter(torch.zeros(128))      # a bias where the module has none
    assert nhwc.resnet_plan(net) is None
    net = ResNet(50, base_channels=24).eval()                      # 24 input channels of a 1x1: K & 31
    assert nhwc.resnet_plan(net) is None
    net = ResNet(101, style="caffe", dcn=DCN, stage_with_dcn=(False, False, False, True)).eval()
    assert nhwc.resnet_plan(net) is not None
    net.layer4[0].conv2.dilation = 2                               # srf_conv_gemm_nhwc (conv_offset) has no dilation
    assert nhwc.resnet_plan(net) is None


P31 = 1 << 31
# (function, arguments, verdict, reason)
LIMITS = [
    (ops.stem7_channels_ok, (3, 64), True, "csrc/conv.hip:1547"),
    (ops.stem7_channels_ok, (1, 64), True, "csrc/conv.hip:1547"),
    (ops.stem7_channels_ok, (4, 64), True, "Cin > 4 refuses (csrc/conv.hip:1547)"),
    (ops.stem7_channels_ok, (5, 64), False, "Cin > 4 (csrc/conv.hip:1547)"),
    (ops.stem7_channels_ok, (3, 32), False, "Cout != 64 (csrc/conv.hip:1547)"),
    (ops.stem7_channels_ok, (3, 128), False, "Cout != 64 (csrc/conv.hip:1547)"),
    (ops.stem7_range_ok, ((1 << 23) - 1, 64), True, "256 (2^23 - 1) < 2^31 (csrc/conv.hip:1551)"),
    (ops.stem7_range_ok, (1 << 23, 64), False, "256 * 2^23 = 2^31: `>=` refuses (csrc/conv.hip:1551)"),
    (ops.stem7_range_ok, (464 * 800, 64), True, "one 928 x 1600 view: 95 MB"),
]
EXTENTS = [(1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (7, 4), (8, 4), (9, 5), (464, 232), (465, 233), (35, 18), (51, 26)]


@pytest.mark.parametrize("fn,args,want,why", LIMITS, ids=[f"{r[0].__name__}{r[1]}" for r in LIMITS])
def test_limit(fn, args, want, why):
    assert fn(*args) is want, why


@pytest.mark.parametrize("h,ho", EXTENTS)
def test_pool_extent(h, ho):
    """`(H - 1) / 2 + 1` of csrc/nhwc.hip:257 = torch's floor-mode extent (h + 2 * 1 - 3) // 2 + 1."""
    assert ops.pool3s2p1_out(h) == ho == (h + 2 - 3) // 2 + 1


def _entry_of(lines, n):
    """The `extern "C"` entry point whose body holds line n (1-based)."""
    return next(l for l in reversed(lines[:n]) if l.startswith('extern "C"'))


def test_the_source_lines_say_what_the_limits_say():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conv = open(os.path.join(root, "srfdet3d_amd", "csrc", "conv.hip")).read().splitlines()
    pool = open(os.path.join(root, "srfdet3d_amd", "csrc", "nhwc.hip")).read().splitlines()
    assert "Cin > 4 || Cout != 64" in conv[1547 - 1] and "srf_stem_conv7_nchw(" in _entry_of(conv, 1547)
    assert "Ho = (H - 1) / 2 + 1" in pool[257 - 1] and "srf_nhwc_maxpool3s2_pad1(" in _entry_of(pool, 257)
    assert "Ho * Wo * y_ld * 4 >= (1ll << 31)" in conv[1551 - 1] and "conv.hip:1551" in ops.stem7_range_ok.__doc__
    assert "conv.hip:1547" in ops.stem7_channels_ok.__doc__ and "nhwc.hip:257" in ops.pool3s2p1_out.__doc__


def test_the_residual_column_of_the_gemm_kinds():
    assert {k: v["residual"] for k, v in ops._GEMM_KINDS.items()} == dict(
        lds="srf_conv1x1_nhwc_residual", direct="srf_conv1x1_nhwc_direct_residual", split="srf_conv1x1_nhwc_split_residual", bf16=None)
