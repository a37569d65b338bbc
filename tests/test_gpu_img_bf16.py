"""The bf16-product mode of the image branch above the kernels: the routing of nhwc.conv3x3 / conv1x1 / conv_strided inside
`nhwc.mfma_dtype`, the accuracy of VoVNet-99 + image FPN in the mode against torch autocast (the yardstick is the torch route, not
the code under test), and the public switch `SRFDet.img_mfma_dtype` (caches, graphs, error cases, the LiDAR half untouched)."""
import copy
import os
import sys

import pytest
import torch
from torch import nn

if __name__ == "__main__":   # run as the child process of `switch_results`: what tests/conftest.py does for pytest
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

from srfdet3d_amd import derived, nhwc, ops, synthetic as S, workloads
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _bn(c, seed):
    bn = nn.BatchNorm2d(c).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.1)
    _randomize_bn(bn, seed)
    return bn


_PACKED = {"wino", "wino43", "gemm", "gemm_direct", "gemm_split", "gemm_bf16", "cgemm", "cgemm_split", "cgemm_bf16", "conv1x1_nchw", "spconv", "dcn"}


def _cache_keys(mod):
    """The packed operands held for `mod` (derived.py)."""
    return sorted(derived.names(mod) & _PACKED)


# ---- routing -------------------------------------------------------------------------------------------------------------------
def test_mode_routes_the_three_layer_kinds_to_the_bf16_kernels_and_leaves_them_alone_when_off(dev):
    torch.manual_seed(4)
    g = torch.Generator().manual_seed(4)
    x = torch.relu(torch.randn(2, 21, 27, 160, generator=g)).to(dev)
    c3, b3 = nn.Conv2d(64, 72, 3, padding=1, bias=False).to(dev), _bn(72, 1).to(dev)
    c1, b1 = nn.Conv2d(160, 96, 1, bias=False).to(dev), _bn(96, 2).to(dev)
    cs = nn.Conv2d(96, 136, 3, stride=2, padding=1, bias=True).to(dev)
    top = torch.randn(2, 11, 14, 96, generator=g).to(dev)
    dst = torch.zeros(2, 21, 27, 200, device=dev)

    def run():
        a = nhwc.conv3x3(x[..., 32:96], c3, b3, True, out=dst[..., 40:112]).clone()
        b = nhwc.conv1x1(x, c1, b1, True).clone()
        bp, mean = nhwc.conv1x1(x, c1, b1, True, pool=True)
        bt = nhwc.conv1x1(x, c1, None, False, top=top).clone()
        c = nhwc.conv_strided(x[..., 64:160], cs, None, False).clone()
        return [a, b, bp.clone(), mean.clone(), bt, c]

    with torch.no_grad():
        off0 = run()
        assert not any(k.endswith("bf16") for m in (c3, c1, cs) for k in _cache_keys(m))      # nothing of the mode without the switch
        routes = []
        with nhwc.mfma_dtype(BF16, routes=routes) as mode:
            assert nhwc.mfma_active()
            on = run()
            with nhwc.mfma_dtype(None):                                                        # the nested off-switch (the head's img_convs)
                inner = nhwc.conv3x3(x[..., 32:96], c3, b3, True).clone()
        assert not nhwc.mfma_active()
        off1 = run()
        # the kernels' own results, bit for bit
        s3, h3 = nhwc._affine_of(c3, b3)
        s1, h1 = nhwc._affine_of(c1, b1)
        want = [ops.conv_gemm_nhwc(x[..., 32:96], None, 72, (3, 3), 1, 1, s3, h3, True, packed_bf16=ops.pack_conv_gemm_bf16_weights(c3.weight)),
                ops.conv1x1_nhwc(x, None, 96, s1, h1, True, packed_bf16=ops.pack_conv1x1_nhwc_bf16_weights(c1.weight))]
        wp, wmean = ops.conv1x1_nhwc(x, None, 96, s1, h1, True, pool=True, packed_bf16=ops.pack_conv1x1_nhwc_bf16_weights(c1.weight))
        want += [wp, wmean, ops.conv1x1_nhwc(x, None, 96, None, None, False, top=top, packed_bf16=ops.pack_conv1x1_nhwc_bf16_weights(c1.weight)),
                 ops.conv_gemm_nhwc(x[..., 64:160], None, 136, (3, 3), 2, 1, None, cs.bias, False,
                                    packed_bf16=ops.pack_conv_gemm_bf16_weights(cs.weight))]
    for i, (a, b, w, o) in enumerate(zip(off0, off1, want, on)):
        assert torch.equal(a, b), i                       # off: today's results, before and after the mode was used
        assert torch.equal(o, w), i                       # on: the bf16 kernels' results
        assert not torch.equal(o, a), i                   # and another arithmetic than the f32 route
    assert torch.equal(inner, off0[0])
    assert mode.launches == 5 and [r["route"] for r in routes] == ["bf16"] * 5
    assert routes[0]["layer"] == "64->72 3x3/s1 @2x21x27" and routes[4]["layer"] == "96->136 3x3/s2 @2x21x27"
    assert "cgemm_bf16" in _cache_keys(c3) and "gemm_bf16" in _cache_keys(c1) and "cgemm_bf16" in _cache_keys(cs)
    for m in (c3, c1, cs):
        nhwc.invalidate_caches(m)
        assert _cache_keys(m) == []


def test_layers_the_family_cannot_take_keep_their_f32_route(dev):
    g = torch.Generator().manual_seed(6)
    c8 = nn.Conv2d(8, 64, 3, padding=1, bias=True).to(dev)                      # Cin % 32 != 0
    x8 = torch.randn(1, 19, 23, 8, generator=g).to(dev)
    stem = nn.Conv2d(3, 64, 3, stride=2, padding=1, bias=False).to(dev)         # VoVNet stem_1: srf_stem_conv_nchw, outside the mode's reach
    img = torch.randn(1, 3, 32, 48, generator=g).to(dev)
    with torch.no_grad():
        a = nhwc.conv3x3(x8, c8).clone()
        s = ops.stem_conv_nchw(img, stem.weight, None, None, True).clone()
        routes = []
        with nhwc.mfma_dtype(BF16, routes=routes) as mode:
            b = nhwc.conv3x3(x8, c8).clone()
            s2 = ops.stem_conv_nchw(img, stem.weight, None, None, True).clone()
    assert torch.equal(a, b) and torch.equal(s, s2)
    assert mode.launches == 0 and routes == [dict(layer="8->64 3x3/s1 @1x19x23", route="f32", why="input channels are no multiple of 32")]
    with pytest.raises(ValueError):
        nhwc.mfma_dtype(torch.float16)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _lc():
    torch.manual_seed(2)
    cpu = workloads.build("srfdet_voxel_nusc_LC", 48).eval()
    _randomize_bn(cpu, 2)
    cpu.bbox_head.test_cfg = dict(cpu.bbox_head.test_cfg, score_thr=0.02)      # random weights: let the NMS have work
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig(f=1266.0 * 256 / 1600, cx=128.0, cy=80.0)])]
    img = torch.from_numpy(S.camera_images(3000, h=160, w=256))
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 12000))
    return dict(cpu=cpu, metas=metas, img=img, pts=pts)


@pytest.fixture(scope="module")
def lc():
    return _lc()


def test_vovnet_fpn_in_the_mode_is_at_least_as_accurate_as_torch_autocast(lc, dev):
    """VoVNet-99 + image FPN, randomised BatchNorm statistics, one 160 x 256 camera.  Error of a level = RMS difference to the f32 route
    / RMS of the f32 level.  The mode commits a strict subset of autocast's roundings (operands of each GEMM, once; autocast also
    rounds every conv / BatchNorm / ReLU output), so per level err(img_mfma_dtype) <= err(img_autocast_dtype), without a margin."""
    m = copy.deepcopy(lc["cpu"]).to(dev)
    img = lc["img"][:, :1].to(dev)

    def feats():
        with torch.no_grad():
            return [f.float().clone() for f in m.extract_img_feat(img, copy.deepcopy(lc["metas"]))]

    f32 = feats()
    m.img_autocast_dtype = BF16
    auto = feats()
    m.img_autocast_dtype = None
    m.img_mfma_dtype = BF16
    mfma = feats()
    assert len(f32) == 4
    for lvl, (r, a, b) in enumerate(zip(f32, auto, mfma)):
        rms = r.double().pow(2).mean().sqrt().item()
        e_auto = (a.double() - r.double()).pow(2).mean().sqrt().item() / rms
        e_mfma = (b.double() - r.double()).pow(2).mean().sqrt().item() / rms
        print(f"\nlevel {lvl}: err(img_mfma_dtype=bf16) = {e_mfma:.4e}, err(img_autocast_dtype=bf16) = {e_auto:.4e}, ratio {e_mfma / e_auto:.3f}")
        assert rms > 1e-4 and e_mfma > 0
        assert e_mfma <= e_auto, (lvl, e_mfma, e_auto)
    # every GEMM-shaped layer of the branch with Cin % 32 == 0 ran on the bf16 kernels; the 3-channel stem_1 is not among the routed layers
    routes = []
    with torch.no_grad(), nhwc.mfma_dtype(BF16, routes=routes):
        m.img_neck(list(m.img_backbone(img[0]).values()))
    assert len(routes) > 60 and all(r["route"] == "bf16" for r in routes) and not any(r["layer"].startswith("3->") for r in routes)


def _same_det(a, b):
    return (torch.equal(a["scores_3d"], b["scores_3d"]) and torch.equal(a["labels_3d"], b["labels_3d"])
            and torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor))


def _switch_scenario(lc, dev):
    """The life of the switch on a graphed LC model -> dict of named checks (booleans) and counts.  Three capture cycles of the
    whole-frame and camera graphs: runs in the child process of `switch_results`."""
    img, pts, metas = lc["img"].to(dev), lc["pts"].to(dev), lc["metas"]
    g = copy.deepcopy(lc["cpu"]).to(dev).enable_hip_graphs()
    default = copy.deepcopy(lc["cpu"]).to(dev)
    r = {}

    def det(model):
        with torch.no_grad():
            return model.simple_test(img, [pts], copy.deepcopy(metas))[0]["pts_bbox"]

    det(g)                           # eager + capture
    d0 = det(g)                      # replay (detections are compared replay against replay: the eager first pass takes another NMS route)
    r["detections"] = int(d0["scores_3d"].numel())
    r["default_replays_repeat"] = _same_det(d0, det(g))
    old_img_graph = g._graphed_img
    r["default_captured_and_packed"] = bool(old_img_graph.entries) and any(_cache_keys(m) for m in g.img_backbone.modules())
    g.img_mfma_dtype = BF16
    r["setting_drops_packed_weights"] = not any(_cache_keys(m) for m in g.modules())        # packed weights of the other route: gone
    r["setting_drops_graphs"] = g._graphed_img is not old_img_graph and not g._graphed_img.entries   # and the graphs that held their addresses
    det(g)
    d1 = det(g)
    r["mode_captured"] = bool(g._graphed_img.entries)
    r["mode_replays_repeat"] = _same_det(d1, det(g))
    r["mode_changes_detections"] = not _same_det(d1, d0)
    r["mode_packed_bf16"] = any("cgemm_bf16" in _cache_keys(m) for m in g.img_backbone.modules())
    # graph replay == eager, bit for bit, in the mode: the camera graph's feature buffers against the same chain run eagerly
    replayed = [f.clone() for f in next(iter(g._graphed_img.entries.values()))["feats"]]
    with torch.no_grad(), nhwc.level_consumer(g.img_neck, g.bbox_head.img_level_consumer()):
        eager = g.extract_img_feat(img, copy.deepcopy(metas))
    r["replay_equals_eager_bitwise"] = len(eager) == len(replayed) and all(torch.equal(a, b) for a, b in zip(eager, replayed))
    # the head's img_convs stayed f32 inside the neck's chains: none of them holds a bf16 pack
    r["img_convs_stay_f32"] = not any(k.endswith("bf16") for c in g.bbox_head.img_convs for m in c.modules() for k in _cache_keys(m))
    # the LiDAR half does not see the switch
    with torch.no_grad():
        bev_on = [f.clone() for f in g.extract_point_features([pts])]
        bev_def = default.extract_point_features([pts])
    r["bev_features_bitwise_default"] = len(bev_on) == len(bev_def) and all(torch.equal(a, b) for a, b in zip(bev_on, bev_def))
    r["bev_layers_stay_f32"] = not any(k.endswith("bf16") for part in (g.pts_backbone, g.pts_neck) for m in part.modules()
                                       for k in _cache_keys(m))
    # back to None: the original detections, bit for bit
    g.img_mfma_dtype = None
    r["unsetting_drops_state"] = not any(_cache_keys(m) for m in g.modules()) and not g._graphed_img.entries
    det(g)
    r["back_to_none_reproduces_detections_bitwise"] = _same_det(det(g), d0)
    return r


@pytest.fixture(scope="module")
def switch_results(dev):
    """`_switch_scenario` in ONE fresh child process.  It captures and destroys the whole-frame graph (head graph with fork / join
    pairs) and the camera graph three times; further head captures in the suite's own process are the pattern after which a LATER
    camera-graph replay of another test has died inside the runtime's graph launch (DESIGN.md section 3,
    profiles/fault_graph_replay_after_head_captures.log; seen again with this scenario in-process).  Same remedy as
    tests/test_gpu_decoder_free.py; what is asserted is the same as in-process."""
    import json
    import subprocess
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    res = None
    for line in run.stdout.splitlines():
        if line.startswith("SWITCH_RESULT "):
            res = json.loads(line[len("SWITCH_RESULT "):])
    print(run.stdout[-2000:])
    assert run.returncode == 0 and res is not None, run.stderr[-4000:]
    return res


CHECKS = ["default_replays_repeat", "default_captured_and_packed", "setting_drops_packed_weights", "setting_drops_graphs", "mode_captured",
          "mode_replays_repeat", "mode_changes_detections", "mode_packed_bf16", "replay_equals_eager_bitwise", "img_convs_stay_f32",
          "bev_features_bitwise_default", "bev_layers_stay_f32", "unsetting_drops_state", "back_to_none_reproduces_detections_bitwise"]


def test_switch_drops_derived_state_and_graphs_replay_the_mode(switch_results):
    assert switch_results["detections"] > 5, "the test needs detections"
    for name in CHECKS:
        assert switch_results[name] is True, name


def test_switch_error_cases(lc, dev):
    m = copy.deepcopy(lc["cpu"])
    with pytest.raises(ValueError, match="bfloat16"):
        m.img_mfma_dtype = torch.float16
    m.img_autocast_dtype = BF16
    with pytest.raises(ValueError, match="img_autocast_dtype"):
        m.img_mfma_dtype = BF16
    m.img_autocast_dtype = None
    m.img_mfma_dtype = BF16
    assert m.img_mfma_dtype is BF16
    m.img_autocast_dtype = BF16                       # set afterwards: refused where it would take effect
    with pytest.raises(ValueError, match="exclude"), torch.no_grad():
        m.extract_img_feat(lc["img"], copy.deepcopy(lc["metas"]))
    m.img_autocast_dtype = None
    m.img_mfma_dtype = None
    assert m.img_mfma_dtype is None
    r50 = workloads.build("srfdet_voxel_r50_nusc_LC", 48).eval()
    with pytest.raises(NotImplementedError, match="channels-last executor"):
        r50.img_mfma_dtype = BF16
    assert r50.img_mfma_dtype is None
    # a pass that leaves the executor (autograd on) is an error in the mode, not a quiet f32 pass
    md = copy.deepcopy(lc["cpu"]).to(dev)
    md.img_mfma_dtype = BF16
    with pytest.raises(RuntimeError, match="channels-last executor"), torch.enable_grad():
        md.extract_img_feat(lc["img"][:, :1].to(dev), copy.deepcopy(lc["metas"]))


if __name__ == "__main__":   # the child process of `switch_results`
    import json
    print("SWITCH_RESULT " + json.dumps(_switch_scenario(_lc(), torch.device("cuda:0"))), flush=True)
