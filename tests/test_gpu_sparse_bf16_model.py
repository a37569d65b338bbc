"""The bf16-product mode of the sparse encoder above the kernel: the accuracy of the nuScenes encoder in the mode against a route that
commits a strict superset of its roundings (built here from the f32 kernel: the yardstick is not the code under test), which layers
take which route, the error cases, and the public switch `SRFDet.sparse_mfma_dtype` on a graphed model (caches, graphs, replay ==
eager bit for bit)."""
import copy
import os
import sys

import pytest
import torch
from torch import nn

if __name__ == "__main__":   # run as the child process of `switch_results`: what tests/conftest.py does for pytest
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

from srfdet3d_amd import derived, ops, synthetic as S, workloads
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
from srfdet3d_amd.plugin.middle_encoders import SparseEncoderCustom

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FIVE = {(27, 32, 64), (27, 64, 64), (27, 64, 128), (27, 128, 128), (3, 128, 128)}


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _l():
    torch.manual_seed(2)
    cpu = workloads.build("srfdet_voxel_nusc_L", 48).eval()
    _randomize_bn(cpu, 2)
    cpu.bbox_head.test_cfg = dict(cpu.bbox_head.test_cfg, score_thr=0.02)      # random weights: let the NMS have work
    return dict(cpu=cpu, metas=[dict(box_type_3d=LiDARInstance3DBoxes)], pts=torch.from_numpy(S.nuscenes_sweep(2000, 12000)))


@pytest.fixture(scope="module")
def l():
    return _l()


def _bf16_names(part):
    return sorted(k for m in part.modules() for k in derived.names(m) if k.endswith("bf16"))


def _cout(route):
    return int(route["layer"].split("->")[1].split(" ")[0])


def test_encoder_in_the_mode_is_at_least_as_accurate_as_a_superset_of_its_roundings(l, dev, monkeypatch):
    """Error of the BEV map = RMS difference to the f32 map / RMS of the f32 map.  The superset route runs the five-shape layers on the
    f32 kernel with inputs, weights AND outputs rounded to bf16 (the mode rounds inputs and weights only), so
    err(mode) <= err(superset), without a margin."""
    m = copy.deepcopy(l["cpu"]).to(dev)
    pts = l["pts"].to(dev)

    def bev():
        with torch.no_grad():
            return m.extract_bev([pts]).float().clone()

    f32 = bev()
    real = ops.spconv_fwd
    rounded_layers = []

    def superset(feats, weight, nbr, alpha=None, beta=None, residual=None, relu=False, pair_counts=None, packed=None, rows_dev=None,
                 tiles=None, subm=False):
        if tuple(weight.shape) not in FIVE:
            return real(feats, weight, nbr, alpha, beta, residual, relu, pair_counts, packed, rows_dev, tiles, subm)
        rounded_layers.append(tuple(weight.shape))
        out = real(feats.bfloat16().float(), weight.detach().bfloat16().float(), nbr, alpha, beta, residual, relu, pair_counts, None, rows_dev,
                   None, subm)
        return out.bfloat16().float()

    monkeypatch.setattr(ops, "spconv_fwd", superset)
    sup = bev()
    monkeypatch.setattr(ops, "spconv_fwd", real)
    assert torch.equal(bev(), f32)                               # the stand-in is gone
    routes = m.pts_middle_encoder.mfma_routes = []
    m.sparse_mfma_dtype = BF16
    assert m.sparse_mfma_dtype is BF16 and m.pts_middle_encoder.mfma_dtype is BF16
    mode = bev()
    rms = f32.double().pow(2).mean().sqrt().item()
    e_mode = (mode.double() - f32.double()).pow(2).mean().sqrt().item() / rms
    e_sup = (sup.double() - f32.double()).pow(2).mean().sqrt().item() / rms
    print(f"\nBEV map: err(sparse_mfma_dtype=bf16) = {e_mode:.4e}, err(inputs, weights and outputs rounded) = {e_sup:.4e}, ratio {e_mode / e_sup:.3f}")
    assert rms > 1e-4 and not torch.equal(mode, f32) and e_mode > 0
    assert e_mode <= e_sup, (e_mode, e_sup)
    # every 64- / 128-channel layer on bf16, every other layer on f32; the superset route rounded the same layers
    assert len(routes) > 10 and len(rounded_layers) == sum(r["route"] == "bf16" for r in routes)
    for r in routes:
        assert (r["route"] == "bf16") == (_cout(r) in (64, 128)) and (r["why"] is None) == (r["route"] == "bf16"), r
    assert {_cout(r) for r in routes if r["route"] == "f32"} == {16, 32}
    assert _bf16_names(m.pts_middle_encoder) and set(_bf16_names(m.pts_middle_encoder)) == {"spconv_bf16"}
    # SECOND, the BEV FPN and the head are out of the switch's reach
    with torch.no_grad():
        m.simple_test(None, [pts], copy.deepcopy(l["metas"]))
    assert _bf16_names(m.pts_backbone) == [] and _bf16_names(m.pts_neck) == [] and _bf16_names(m.bbox_head) == []
    # back to None: the f32 map, and no bf16 pack left
    m.pts_middle_encoder.mfma_routes = None
    m.sparse_mfma_dtype = None
    assert _bf16_names(m) == []
    assert torch.equal(bev(), f32)


def test_switch_error_cases(l, dev):
    m = copy.deepcopy(l["cpu"]).to(dev)
    pts = l["pts"].to(dev)
    with pytest.raises(ValueError, match="bfloat16"):
        m.sparse_mfma_dtype = torch.float16
    assert m.sparse_mfma_dtype is None
    m.sparse_mfma_dtype = BF16
    with pytest.raises(RuntimeError, match="no_grad"), torch.enable_grad():        # gradients on: no quiet f32 pass
        m.extract_bev([pts])
    m.pts_middle_encoder.train()
    with pytest.raises(RuntimeError, match="eval mode"), torch.no_grad():          # training mode
        m.extract_bev([pts])
    m.pts_middle_encoder.eval()
    with torch.no_grad():
        m.extract_bev([pts])
    # an encoder without a 64- / 128-channel layer: no layer takes the bf16 route, which is an error in the mode
    enc = SparseEncoderCustom(5, [41, 1472, 1472], base_channels=16, output_channels=32, encoder_channels=((16,), (32, 32, 32)),
                              encoder_paddings=((1,), (1, 1, 1))).to(dev).eval()
    with torch.no_grad():
        voxels, num, coors = m.voxelize([pts])
        vf = m.pts_voxel_encoder(voxels, num, coors)
        enc(vf, coors, 1)
        enc.mfma_dtype = BF16
        with pytest.raises(RuntimeError, match="none of its layers"):
            enc(vf, coors, 1)
    # a model without a sparse encoder
    pillar = workloads.build("srfdet_pillar_nusc_L", 48).eval()
    with pytest.raises(NotImplementedError, match="sparse"):
        pillar.sparse_mfma_dtype = BF16
    pillar.sparse_mfma_dtype = None
    assert pillar.sparse_mfma_dtype is None


def _same_det(a, b):
    return (torch.equal(a["scores_3d"], b["scores_3d"]) and torch.equal(a["labels_3d"], b["labels_3d"])
            and torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor))


def _packed(model):
    return sorted({k for m in model.modules() for k in derived.names(m) if k.startswith("spconv")})


def _switch_scenario(l, dev):
    """The life of the switch on a graphed nusc_L model -> dict of named checks.  Three captures of the whole-frame graph (f32, the mode,
    f32 again): runs in the child process of `switch_results`."""
    pts, metas = l["pts"].to(dev), l["metas"]
    g = copy.deepcopy(l["cpu"]).to(dev).enable_hip_graphs()
    r = {}

    def det(model):
        with torch.no_grad():
            return model.simple_test(None, [pts], copy.deepcopy(metas))[0]["pts_bbox"]

    det(g)                           # eager + capture
    d0 = det(g)                      # replay
    r["detections"] = int(d0["scores_3d"].numel())
    r["default_replays_repeat"] = _same_det(d0, det(g))
    old = g._graphed_frame
    r["default_captured_and_packed"] = old is not None and old.entry is not None and _packed(g) == ["spconv"]
    g.sparse_mfma_dtype = BF16
    r["setting_drops_packed_weights"] = _packed(g) == []
    r["setting_drops_graphs"] = g._graphed_frame is not old and g._graphed_frame.entry is None
    det(g)
    d1 = det(g)
    r["mode_captured"] = g._graphed_frame.entry is not None and g._graphed_frame.stats["replays"] >= 1
    r["mode_replays_repeat"] = _same_det(d1, det(g))
    r["mode_changes_detections"] = not _same_det(d1, d0)
    r["mode_packed_bf16"] = _packed(g) == ["spconv", "spconv_bf16"]          # (the 16- / 32-channel layers keep their f32 pack)
    # graph replay at the padded capacities == the eager pass, bit for bit, in the mode: the BEV pyramid the graph left behind
    replayed = [t.clone() for t in g._graphed_frame.entry["bev"]]
    with torch.no_grad():
        eager = g.extract_point_features([pts])
        if g._graphed_frame._encodes():
            eager = g.bbox_head.encode_lidar(eager)
    r["replay_equals_eager_bitwise"] = len(eager) == len(replayed) and all(torch.equal(a, b) for a, b in zip(eager, replayed))
    g.sparse_mfma_dtype = None
    r["unsetting_drops_state"] = _packed(g) == [] and g._graphed_frame.entry is None
    det(g)
    r["back_to_none_reproduces_detections_bitwise"] = _same_det(det(g), d0)
    return r


@pytest.fixture(scope="module")
def switch_results(dev):
    """`_switch_scenario` in ONE fresh child process with a timeout, as tests/test_gpu_img_bf16.py and for the reason given there:
    repeated whole-frame captures inside the suite's own process are a known hazard."""
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
          "mode_replays_repeat", "mode_changes_detections", "mode_packed_bf16", "replay_equals_eager_bitwise", "unsetting_drops_state",
          "back_to_none_reproduces_detections_bitwise"]


def test_switch_drops_derived_state_and_graphs_replay_the_mode(switch_results):
    assert switch_results["detections"] > 5, "the test needs detections"
    for name in CHECKS:
        assert switch_results[name] is True, name


if __name__ == "__main__":   # the child process of `switch_results`
    import json
    print("SWITCH_RESULT " + json.dumps(_switch_scenario(_l(), torch.device("cuda:0"))), flush=True)
