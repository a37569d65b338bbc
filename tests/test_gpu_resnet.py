"""The bottleneck ResNet image backbones on the channels-last executor (`nhwc.resnet`) against the same module in float64 on the CPU.

Bound: every level within 2e-4 of that level's largest |value| -- the project's bound for an image backbone on these kernels
(tests/test_gpu_round3.py, tests/test_gpu_lc_parity.py).  Each test prints the worst |error| / max |value| per level, for the executor
and for the SRF_IMG_NHWC=0 route; measured on an MI355X ("Bottleneck ResNets"): 2.8e-7 ... 8.0e-7 on the executor,
1.9e-7 ... 5.5e-7 with the switch off, level maxima 0.97 ... 2.58."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from srfdet3d_amd import nhwc, synthetic as S, workloads
from srfdet3d_amd.compat import registry
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
from srfdet3d_amd.compat.resnet import ResNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
DCN = dict(type="DCNv2", deform_groups=1, fallback_on_stride=False)
CASES = {
    "r50 2x3x64x96": ("r50", (2, 3, 64, 96)),
    "r50 1x3x70x102": ("r50", (1, 3, 70, 102)),          # odd maps all the way down: 35x51 -> 18x26 -> 9x13 -> 5x7 -> 3x4
    "r101dcn 2x3x64x96": ("r101dcn", (2, 3, 64, 96)),
}
NECK = {"r50": "srfdet_voxel_r50_nusc_LC", "r101dcn": "srfdet_dvoxel_waymo_LC"}


def _randomize_bn(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


@functools.lru_cache(maxsize=None)
def _net(kind):
    torch.manual_seed(11)
    if kind == "r50":
        net = ResNet(50, style="pytorch", frozen_stages=1, norm_eval=True)
    else:
        net = ResNet(101, style="caffe", dcn=DCN, stage_with_dcn=(False, False, True, True), norm_eval=True)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for m in net.modules():
                if hasattr(m, "conv_offset"):      # offsets and mask logits that are not zero
                    m.conv_offset.weight.copy_(torch.randn(m.conv_offset.weight.shape, generator=g) * 0.01)
                    m.conv_offset.bias.copy_(torch.randn(m.conv_offset.bias.shape, generator=g) * 0.5)
    _randomize_bn(net, 3)
    return net.eval()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(the f32 net on the CPU, the input, the float64 levels): computed once, shared, never written."""
    kind, shape = CASES[name]
    net = _net(kind)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    with torch.no_grad():
        want = copy.deepcopy(net).double()(x.double())
    return net, x, want


@functools.lru_cache(maxsize=None)
def _gpu_net(kind):
    return copy.deepcopy(_net(kind)).to(DEV)


def _raise(name):
    def fn(*a, **kw):
        raise AssertionError(f"{name} was called: the layer left the HIP kernels")
    return fn


def _worst(got, want):
    return [((g.double().cpu() - w).abs().max() / w.abs().max()).item() for g, w in zip(got, want)]


@pytest.mark.parametrize("name", list(CASES))
def test_executor_matches_float64_and_runs_no_torch_layer(name, monkeypatch):
    net, x, want = _case(name)
    gpu = _gpu_net(CASES[name][0])
    monkeypatch.delenv("SRF_IMG_NHWC", raising=False)
    monkeypatch.delenv("SRF_DCN", raising=False)
    with monkeypatch.context() as mp:
        mp.setattr(nn.Conv2d, "forward", _raise("nn.Conv2d.forward"))
        for fn in ("conv2d", "max_pool2d", "batch_norm", "grid_sample"):
            mp.setattr(F, fn, _raise("F." + fn))
        with torch.no_grad():
            got = gpu(x.to(DEV))
            again = gpu(x.to(DEV))
    assert isinstance(got, tuple) and len(got) == len(want) == 4
    for g, a, w in zip(got, again, want):
        assert tuple(g.shape) == tuple(w.shape) and nhwc.is_channels_last(g) and g.dtype == torch.float32
        assert torch.equal(g, a)                                   # deterministic
    worst = _worst(got, want)
    print(f"{name}: executor, worst |error| / max |value| per level = {['%.2e' % v for v in worst]}, "
          f"level maxima {['%.2f' % w.abs().max().item() for w in want]}")
    assert max(worst) <= TOL, worst
    # the config's FPN takes these levels onto the executor
    neck = registry.build_neck(workloads.model_cfg(NECK[CASES[name][0]])["img_neck"]).eval().to(DEV)
    with torch.no_grad():      # the gate asks for inference mode (`dense.fusable`)
        assert nhwc.fpn_supported(neck, got)
        outs = neck(got)
    assert len(outs) == neck.num_outs and all(nhwc.is_channels_last(o) for o in outs)


@pytest.mark.parametrize("name", list(CASES))
def test_the_switch_gives_the_module_route_within_the_same_bound(name, monkeypatch):
    net, x, want = _case(name)
    gpu = _gpu_net(CASES[name][0])
    monkeypatch.setenv("SRF_IMG_NHWC", "0")
    with torch.no_grad():
        got = gpu(x.to(DEV))
    assert all(g.is_contiguous() and tuple(g.shape) == tuple(w.shape) for g, w in zip(got, want))
    worst = _worst(got, want)
    print(f"{name}: SRF_IMG_NHWC=0, worst |error| / max |value| per level = {['%.2e' % v for v in worst]}")
    assert max(worst) <= TOL, worst


def test_autograd_and_cpu_go_the_way_they_went():
    gpu = _gpu_net("r50")
    x = torch.randn(1, 3, 64, 96, device=DEV)
    assert nhwc.resnet(gpu, x) is None                             # grad mode is on: not the executor's call
    out = gpu(x)
    assert all(o.is_contiguous() for o in out)
    with torch.no_grad():
        assert nhwc.resnet(_net("r50"), x.cpu()) is None
        assert nhwc.resnet(gpu, x) is not None


@functools.lru_cache(maxsize=None)
def _detector():
    torch.manual_seed(4)
    cpu = workloads.build("srfdet_voxel_r50_nusc_LC", 32).eval()
    _randomize_bn(cpu, 4)
    return cpu


def _metas():
    return [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig(f=1266.0 * 256 / 1600, cx=128.0, cy=80.0)])]


def _eager_feats(model, img):
    """The image features as the camera graph computes them: the head's `img_convs` as the consumer of every FPN level."""
    with torch.no_grad(), nhwc.level_consumer(model.img_neck, model.bbox_head.img_level_consumer()):
        return [f.clone() for f in model.extract_img_feat(img, _metas())]


def test_r50_lc_image_graph_replays_the_eager_features():
    imgs = [torch.from_numpy(S.camera_images(3000 + i, h=160, w=256)).to(DEV) for i in range(2)]
    eager = copy.deepcopy(_detector()).to(DEV)
    want = [_eager_feats(eager, im) for im in imgs]
    assert len(want[0]) == 4 and not torch.equal(want[0][0], want[1][0])
    g = copy.deepcopy(_detector()).to(DEV).enable_hip_graphs(img_overlap=False)
    for im, w in zip(imgs, want):                                  # the first call captures and replays, the second replays
        feats, done = g._graphed_img(im, _metas())
        torch.cuda.current_stream().wait_event(done)
        assert len(g._graphed_img.entries) == 1
        assert all(torch.equal(f, e) for f, e in zip(feats, w))


def test_weights_changed_after_an_in_place_update_gives_the_features_of_a_fresh_copy():
    img = torch.from_numpy(S.camera_images(3002, h=160, w=256)).to(DEV)
    model = copy.deepcopy(_detector()).to(DEV)
    before = _eager_feats(model, img)

    def update(m):      # through .data: neither a version counter nor a pointer changes
        m.img_backbone.layer2[0].conv3.weight.data.mul_(1.25)
        m.img_backbone.layer3[1].bn2.running_var.data.mul_(0.8)
        m.img_backbone.conv1.weight.data.mul_(0.9)
    update(model)
    model.weights_changed()
    after = _eager_feats(model, img)
    fresh = copy.deepcopy(_detector())
    update(fresh)
    want = _eager_feats(fresh.to(DEV), img)
    assert all(torch.equal(a, w) for a, w in zip(after, want))
    assert not torch.equal(after[0], before[0])
