"""`SRFDetHead(with_lidar_encoder=True)` on the GPU: `encode_lidar` on the HIP route and on the SRF_MSDA=0 torch route against the
reference's `_get_lidar_encoder_feats` (tests/golden/lidar_encoder.npz), the derived tensors going stale, and the encoder inside the
whole-frame graph of srfdet_voxel_nusc_L.

Bound of (a) and (b): 4 x the stored float32 figure `e_f32` (max |f32 - f64| / max |f64| of the reference's own float32 run on the host),
same normalisation.  The margin is for the MFMA GEMMs' summation order and the two LayerNorms per layer."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)      # the child process of `frame_results` runs this file as a script
from srfdet3d_amd import derived, ops, synthetic as S, workloads  # noqa: E402
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes  # noqa: E402
from test_lidar_encoder_host import CASES, GOLDEN, fixture_error, fixture_head, fixture_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


def _encode(case, dev):
    head = fixture_head(case).to(dev)
    feats = [f.to(dev) for f in fixture_inputs(case)]
    with torch.no_grad():
        return head, feats, head.encode_lidar(feats)


@pytest.mark.parametrize("case", sorted(CASES))
def test_hip_route_meets_the_reference(case, dev):
    gold = np.load(os.path.join(GOLDEN, "lidar_encoder.npz"))
    e_f32 = float(gold[f"{case}.e_f32"])
    head, feats, out = _encode(case, dev)
    with torch.no_grad():
        assert head._encode_rows_ok(feats, [tuple(f.shape[2:]) for f in feats])      # the kernel's route, not the torch one
    assert "lidar_pos" in derived.names(head) and "msda_qproj" in derived.names(head.encoder_lidar.layers[0].attentions[0])
    assert [tuple(o.shape) for o in out] == [tuple(f.shape) for f in feats]
    err = fixture_error(case, out, gold)
    print(case, "HIP route error", err, "stored e_f32", e_f32, "ratio", err / e_f32)
    assert err <= 4 * e_f32


_CHILD = """
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join({root!r}, "tests"))
from srfdet3d_amd import ops
from test_lidar_encoder_host import CASES, GOLDEN, fixture_error, fixture_head, fixture_inputs
assert not ops.msda_enabled()
gold = np.load(os.path.join(GOLDEN, "lidar_encoder.npz"))
dev = torch.device("cuda")
for case in sorted(CASES):
    head = fixture_head(case).to(dev)
    feats = [f.to(dev) for f in fixture_inputs(case)]
    with torch.no_grad():
        assert not head._encode_rows_ok(feats, [tuple(f.shape[2:]) for f in feats])
        out = head.encode_lidar(feats)
    print("RESULT", case, fixture_error(case, out, gold), float(gold[case + ".e_f32"]))
"""


def test_torch_route_meets_the_reference_in_a_fresh_process():
    env = dict(os.environ, SRF_MSDA="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert sorted(x[1] for x in rows) == sorted(CASES)
    for _, case, err, e_f32 in rows:
        print(case, "SRF_MSDA=0 error", err, "stored e_f32", e_f32, "ratio", float(err) / float(e_f32))
        assert float(err) <= 4 * float(e_f32)


def test_derived_tensors_go_stale(dev):
    """In-place updates through `.data` of `sampling_offsets.bias` and of a position-embedding weight, then the invalidation that
    `SRFDet.weights_changed()` performs: the output is that of a fresh copy of the updated module, bit for bit."""
    head, feats, before = _encode("c128", dev)
    att = head.encoder_lidar.layers[1].attentions[0]
    pe = head.bev_pos_encoder_mlvl_embed[0].position_embedding_head[3]
    with torch.no_grad():
        att.sampling_offsets.bias.data.mul_(1.5)
        pe.weight.data.mul_(0.5)
        stale = head.encode_lidar(feats)
        assert all(torch.equal(a, b) for a, b in zip(stale, before))      # updates through .data are invisible until told
        derived.invalidate(head)
        assert not any(derived.names(m) for m in head.modules())
        after = head.encode_lidar(feats)
        fresh = fixture_head("c128").to(dev)
        fresh.load_state_dict(head.state_dict())
        want = fresh.encode_lidar(feats)
    assert all(torch.equal(a, w) for a, w in zip(after, want))
    moved = max((a - b).abs().max().item() for a, b in zip(after, before))
    print("outputs moved by", moved)
    assert moved > 1e-3


def _randomize_bn(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _frame_scenario():
    """srfdet_voxel_nusc_L with the encoder, np = 200, one synthetic sweep: eager, through `GraphedFrame`, and with the encoder's output
    projections zeroed.  -> dict of the facts `test_graphed_frame_runs_the_encoder` asserts."""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cpu = workloads.build("srfdet_voxel_nusc_L", 200, **{"bbox_head.with_lidar_encoder": True}).eval()
    _randomize_bn(cpu)
    with torch.no_grad():     # the attention's initialisation zeroes the offset and attention weights: give the encoder something to do
        for m in cpu.bbox_head.encoder_lidar.modules():
            if hasattr(m, "sampling_offsets"):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
    cpu.bbox_head.test_cfg = dict(cpu.bbox_head.test_cfg, score_thr=0.02)
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 30000)).to(dev)
    r = {}
    eager = copy.deepcopy(cpu).to(dev)
    want = _detections(eager, pts)
    r["detections"] = int(want[1].numel())
    g = copy.deepcopy(cpu).to(dev).enable_hip_graphs(whole_frame=True)
    got = _detections(g, pts, 3)
    r["replays"] = int(g._graphed_frame.stats["replays"])
    r["replay_equals_eager_bitwise"] = all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, want))
    # with the output projections zeroed the encoder is `LayerNorm(x)` chains only: another pyramid, so the detections move
    z = copy.deepcopy(cpu)
    with torch.no_grad():
        for m in z.bbox_head.encoder_lidar.modules():
            if hasattr(m, "output_proj"):
                m.output_proj.weight.zero_()
                m.output_proj.bias.zero_()
    zg = z.to(dev).enable_hip_graphs(whole_frame=True)
    zgot = _detections(zg, pts, 3)
    r["zeroed_replays"] = int(zg._graphed_frame.stats["replays"])
    r["zeroed_projection_moves_the_detections"] = zgot[1].shape != got[1].shape or not torch.equal(zgot[1], got[1])
    with torch.no_grad():
        raw = eager.extract_point_features([pts])
        enc = eager.bbox_head.encode_lidar(raw)
        bev = g._graphed_frame.entry["bev"]
        r["graph_holds_the_encoded_pyramid"] = all(torch.equal(bev[l], enc[l]) and not torch.equal(bev[l], raw[l]) for l in range(4))
        r["proposal_logits_read_encoded_maps"] = not torch.equal(eager.bbox_head.dpg_lidar_logits(enc), eager.bbox_head.dpg_lidar_logits(raw))
    torch.cuda.synchronize()
    return r


@pytest.fixture(scope="module")
def frame_results(dev):
    """`_frame_scenario` in ONE fresh child process.  It captures the whole-frame graph twice; further captures in the suite's own
    process are the pattern after which a LATER camera-graph replay of another test has died inside the runtime's graph launch
    (profiles/fault_graph_replay_after_head_captures.log; seen again with this scenario in-process).  Same remedy as
    tests/test_gpu_decoder_free.py and tests/test_gpu_img_bf16.py; what is asserted is the same as in-process."""
    import json
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    res = None
    for line in run.stdout.splitlines():
        if line.startswith("FRAME_RESULT "):
            res = json.loads(line[len("FRAME_RESULT "):])
    print(run.stdout[-2000:])
    assert run.returncode == 0 and res is not None, run.stderr[-4000:]
    return res


def _detections(model, pts, n=1):
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    with torch.no_grad():
        for _ in range(n):
            r = model.simple_test(None, [pts], copy.deepcopy(metas))[0]["pts_bbox"]
    return r["boxes_3d"].tensor.clone(), r["scores_3d"].clone(), r["labels_3d"].clone()


def test_graphed_frame_runs_the_encoder(frame_results):
    """The `GraphedFrame` replay equals the eager pass to the bit; the encoder runs inside the graph (its BEV buffers hold the ENCODED
    pyramid, and zeroing the encoder's output projections moves the detections); the proposal generator reads encoded maps."""
    r = frame_results
    print(r)
    assert r["detections"] > 5, "the test needs detections to compare"
    assert r["replays"] >= 1 and r["zeroed_replays"] >= 1
    assert r["replay_equals_eager_bitwise"]
    assert r["zeroed_projection_moves_the_detections"]
    assert r["graph_holds_the_encoded_pyramid"]
    assert r["proposal_logits_read_encoded_maps"]


def test_flag_off_frame_does_not_depend_on_srf_msda(dev, monkeypatch):
    torch.manual_seed(0)
    cpu = workloads.build("srfdet_voxel_nusc_L", 200).eval()
    _randomize_bn(cpu)
    cpu.bbox_head.test_cfg = dict(cpu.bbox_head.test_cfg, score_thr=0.02)
    assert not cpu.bbox_head.with_lidar_encoder and not [k for k in cpu.state_dict() if "encoder_lidar" in k or "bev_" in k]
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 30000)).to(dev)
    on = _detections(copy.deepcopy(cpu).to(dev), pts)
    monkeypatch.setenv("SRF_MSDA", "0")
    assert not ops.msda_enabled()
    off = _detections(copy.deepcopy(cpu).to(dev), pts)
    assert on[1].numel() > 5
    for a, b in zip(on, off):
        assert torch.equal(a, b)


if __name__ == "__main__":
    import json
    print("FRAME_RESULT " + json.dumps(_frame_scenario()), flush=True)
