"""The OTA label assignment on the GPU (csrc/ota.hip: `ops.ota_assign` = `ops.ota_cost` + `ops.ota_match`) against its definition in
tests/ota_ref.py and against the torch route of `OTAssignerSRFDet`.

(a) cost kernel against the float64 `costs`: the inside-box / inside-centre flags are equal wherever the float64 comparison is further from
    equality than the float32 rounding of its operands; the error of cost and IoU against float64 is at most four times the error of the
    float32 torch route on the same inputs against the same float64 numbers, and no tighter than one float32 ulp of the cost -- the bar of
    tests/test_gpu_lidar_encoder_train.py, for its reason: the two float32 routes call different libm functions.  The cost error is taken
    per step class (cost, cost + 100, cost + 10100), since the rounding at 10100 would hide everything below it.
(b) match kernel against `match`, fed the device's own cost / IoU read back: equal, status word included, no case left out.
(c) end to end against the torch route (SRF_OTA=0) on scattered and crowded scenes: identical (fg, j) on every case where the torch route
    agrees with the float64 definition; at most 2 % of the cases may be left out.
(d) the reference run of tests/golden/extra_r2.npz through `assign_layers`, all stages and samples in one call, and the empty sample.
(e) `loss_ota` on both routes bit for bit, one device-to-host copy per step, no synchronisation inside `ops.ota_assign`, equal bytes twice."""
import warnings

import numpy as np
import pytest
import torch

import make_fixtures_r2 as mf2
import ota_ref as O
from srfdet3d_amd import ops
from srfdet3d_amd.plugin import training
from test_fixtures_r2 import GOLD, check_loss_ota, ota_inputs

pytestmark = pytest.mark.gpu
HEADS = [6, 1, 3]                       # S = 3 stages
# (name, P, boxes of the two samples, D, generator).  P: 1, 7 (below candidate_topk), 64, 65 (one row past a 64-row tile), 300, 900 (the config's);
# G: 0, 1, 5, 17, 64, 65, 128; an empty sample next to a full one twice; one prediction for five boxes can never serve them all: the cap.
CASES = [("p1", 1, (5, 1), 10, "scene"), ("p7", 7, (0, 17), 8, "scene"), ("p64", 64, (64, 65), 10, "crowded"),
         ("p65", 65, (128, 1), 8, "scene"), ("ties", 65, (5, 17), 10, "ties"), ("p300", 300, (17, 5), 10, "crowded"),
         ("p900", 900, (64, 0), 10, "scene"), ("p900w", 900, (128, 17), 8, "crowded")]
KERNEL_KW = dict(cost_weights=(O.CFG["w_cls"], O.CFG["w_reg"], O.CFG["w_iou"]), alpha=O.CFG["alpha"], gamma=O.CFG["gamma"], eps=O.CFG["eps"],
                 center_radius=O.CFG["center_radius"])
_CACHE = {}


def assigner():
    return training.OTAssignerSRFDet(**mf2.OTA_KW)


def case(name, dev):
    """Inputs of a case, the device's cost / IoU matrices and the float64 definition, computed once and left unchanged."""
    if name in _CACHE:
        return _CACHE[name]
    _, P, ns, D, gen = next(c for c in CASES if c[0] == name)
    seed = 100 + [c[0] for c in CASES].index(name)
    G = (max(max(ns), 1) + 7) // 8 * 8
    boxes, logits = np.zeros((3, 2, P, D), np.float32), np.zeros((3, 2, P, 10), np.float32)
    gt, labels = np.zeros((2, G, 7), np.float32), np.zeros((2, G), np.int32)
    gt[:], labels[:] = np.nan, 99                     # the padding is never read: NaN boxes and a class past C would show
    for b, n in enumerate(ns):
        for s in range(3):
            sc = O.scene(seed * 10 + b, P, n, D=D, crowded=gen != "scene", stage=s)
            if gen == "ties":
                for p in range(2, P, 3):
                    sc[0][p], sc[1][p] = sc[0][p - 1], sc[1][p - 1]
            boxes[s, b], logits[s, b] = sc[0], sc[1]
        gt[b, :n], labels[b, :n] = sc[2], sc[3]
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(boxes=boxes, logits=logits, gt=gt, labels=labels, n_gt=np.array(ns, np.int32),
                                                         heads=np.array(HEADS, np.int32)).items()}
    cost, iou = ops.ota_cost(t["boxes"], t["logits"], t["gt"], t["labels"], t["n_gt"], **KERNEL_KW)
    ref = {(s, b): O.costs(boxes[s, b], logits[s, b], gt[b, :n], labels[b, :n], **O.CFG) for s in range(3) for b, n in enumerate(ns) if n}
    _CACHE[name] = dict(P=P, ns=ns, G=G, np=dict(boxes=boxes, logits=logits, gt=gt, labels=labels), t=t, cost=cost, iou=iou,
                        cost_h=cost.cpu().numpy(), iou_h=iou.cpu().numpy(), ref=ref)
    return _CACHE[name]


def step_class(x, ref):
    """Which of the steps 0 / 100 / 10100 a float32 cost carries: the one that brings it closest to the float64 cost without steps.
    -> (class 0 / 1 / 2, |x - (base + step)|)"""
    cand = np.stack([np.abs(x - (ref["base"] + st)) for st in (0.0, 100.0, 10100.0)])
    return cand.argmin(0), cand.min(0)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_cost_kernel_meets_float64(dev, name):
    c = case(name, dev)
    a = assigner()
    e = {k: np.zeros(3) for k in ("dev", "torch", "top")}          # per step class: the largest error of either route, the largest |cost|
    e_iou = {"dev": 0.0, "torch": 0.0}
    decided = total = 0
    for (s, b), ref in c["ref"].items():
        n = c["ns"][b]
        got = c["cost_h"][s, b, :n].T.astype(np.float64)            # g-major on the device -> (P, n)
        got_iou = c["iou_h"][s, b, :n].T.astype(np.float64)
        assert np.isfinite(got).all() and np.isfinite(got_iou).all()
        tc, ti = a.cost_matrices(c["t"]["boxes"][s, b], c["t"]["logits"][s, b], c["t"]["gt"][b, :n], c["t"]["labels"][b, :n].long())
        want = np.where(ref["valid"][:, None], np.where(ref["in_both"], 0, 1), 2)
        sure = ref["decided"] & ref["row_decided"][:, None]
        for route, x in (("dev", got), ("torch", tc.cpu().numpy().astype(np.float64))):
            cls, err = step_class(x, ref)
            if route == "dev":                                   # the flags, wherever float32 rounding cannot flip them
                assert np.array_equal(cls[sure], want[sure]), (name, s, b, int((cls[sure] != want[sure]).sum()))
            for k in range(3):
                if (cls == k).any():
                    e[route][k] = max(e[route][k], err[cls == k].max())
                    e["top"][k] = max(e["top"][k], np.abs(x[cls == k]).max())
        e_iou["dev"] = max(e_iou["dev"], np.abs(got_iou - ref["iou"]).max())
        e_iou["torch"] = max(e_iou["torch"], np.abs(ti.cpu().numpy().astype(np.float64) - ref["iou"]).max())
        decided += int(sure.sum())
        total += sure.size
    ulp = np.spacing(e["top"].astype(np.float32)).astype(np.float64)
    print(f"ota cost {name}: flags decided on {decided} of {total} pairs; cost error per step class (0, 100, 10100): kernel {e['dev']}, "
          f"torch f32 {e['torch']}, one ulp {ulp}, ratio {e['dev'] / np.maximum(e['torch'], 1e-300)}; IoU error kernel {e_iou['dev']:.3e}, "
          f"torch f32 {e_iou['torch']:.3e}")
    assert decided > 0.9 * total
    for k in range(3):
        assert e["dev"][k] <= max(4 * e["torch"][k], ulp[k]), (name, k, e["dev"][k], e["torch"][k], ulp[k])
    assert e_iou["dev"] <= max(4 * e_iou["torch"], float(np.spacing(np.float32(1.0)))), (name, e_iou)
    # the columns behind n_gt were not written: the matrices came from torch.empty, so nothing can be said of them but that the
    # kernel got by without them (NaN boxes there), which the finite costs above show


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_match_kernel_is_the_definition(dev, name):
    c = case(name, dev)
    count, pred_idx, gt_idx, status = [x.cpu().numpy() for x in
                                       ops.ota_match(c["cost"], c["iou"], c["t"]["n_gt"], c["t"]["heads"], O.CFG["candidate_topk"], O.CFG["num_heads"])]
    assert np.array_equal(c["cost"].cpu().numpy(), c["cost_h"], equal_nan=True)          # the caller's matrix is left alone
    seen = dict(multi=0, repairs=0, cap=0)
    for s in range(3):
        for b, n in enumerate(c["ns"]):
            ref = O.match(c["cost_h"][s, b, :n].T, c["iou_h"][s, b, :n].T, HEADS[s], **O.CFG)
            k = int(ref["fg"].sum())
            assert count[s, b] == k and status[s, b] == ref["status"], (name, s, b, count[s, b], k, status[s, b], ref["status"])
            assert np.array_equal(pred_idx[s, b, :k], np.nonzero(ref["fg"])[0]) and np.array_equal(gt_idx[s, b, :k], ref["gt"]), (name, s, b)
            assert (pred_idx[s, b, k:] == -1).all() and (gt_idx[s, b, k:] == -1).all()
            seen["multi"] += ref["multi"]
            seen["repairs"] += ref["repairs"] > 0
            seen["cap"] += ref["status"]
    print(f"ota match {name}: multi-match branch in {seen['multi']}, repair loop in {seen['repairs']}, cap hit in {seen['cap']} of 6 pairs")
    if name == "p1":
        assert seen["cap"] == 3                     # one prediction, five boxes, in every stage
    if name in ("p64", "p300", "p900w", "ties"):
        assert seen["multi"] > 0 and seen["repairs"] > 0


def test_match_kernel_on_exact_ties(dev):
    """Integer costs and IoUs of 0 / 0.5: ties in every column, in every arg-min and in the top-k; P = 130 is two waves and two lanes, the
    9 columns leave 7 of the 16 waves idle."""
    rng = np.random.default_rng(7)
    S, B, P, G = 2, 2, 130, 16
    ns = [9, 16]
    cost = rng.integers(0, 4, (S, B, G, P)).astype(np.float32)
    iou = (rng.integers(0, 2, (S, B, G, P)) * 0.5).astype(np.float32)
    heads = [6, 5]
    out = ops.ota_match(torch.from_numpy(cost).to(dev), torch.from_numpy(iou).to(dev), torch.tensor(ns, dtype=torch.int32, device=dev),
                        torch.tensor(heads, dtype=torch.int32, device=dev), 8, 6)
    count, pred_idx, gt_idx, status = [x.cpu().numpy() for x in out]
    for s in range(S):
        for b, n in enumerate(ns):
            ref = O.match(cost[s, b, :n].T, iou[s, b, :n].T, heads[s], 8, 6)
            k = int(ref["fg"].sum())
            assert ref["gap"] == 0.0 and count[s, b] == k and status[s, b] == ref["status"]
            assert np.array_equal(pred_idx[s, b, :k], np.nonzero(ref["fg"])[0]) and np.array_equal(gt_idx[s, b, :k], ref["gt"])


def test_end_to_end_against_the_torch_route(dev, monkeypatch):
    a = assigner()
    cases = [(g, seed) for g in ("scattered", "crowded") for seed in range(48)]
    left_out, multi, repairs = [], 0, 0
    for gen, seed in cases:
        boxes, logits, gt, labels = getattr(O, gen)(seed)
        head_idx = 1 + seed % 6
        c = O.costs(boxes, logits, gt, labels, **O.CFG)
        ref = O.match(c["cost"].astype(np.float32), c["iou"].astype(np.float32), head_idx, **O.CFG)
        assert ref["status"] == 0                   # the torch loop has no cap
        multi += ref["multi"]
        repairs += ref["repairs"] > 0
        t = [torch.from_numpy(x).to(dev) for x in (boxes, logits, gt, labels)]
        monkeypatch.setenv("SRF_OTA", "0")
        res = a.single_assigner(*t, head_idx)
        fg_t, j_t = res
        assert res.rows is None
        monkeypatch.setenv("SRF_OTA", "1")
        res = a.single_assigner(*t, head_idx)
        fg_k, j_k = res
        assert res.rows is not None and fg_k.dtype == torch.bool and j_k.dtype == torch.long
        assert torch.equal(res.rows, fg_k.nonzero().squeeze(1))
        if not (np.array_equal(fg_t.cpu().numpy(), ref["fg"]) and np.array_equal(j_t.cpu().numpy(), ref["gt"])):
            left_out.append((gen, seed, ref["gap"]))
            continue
        assert torch.equal(fg_k, fg_t) and torch.equal(j_k, j_t), (gen, seed, ref["gap"])
    print(f"ota end to end: {len(cases)} cases, multi-match branch in {multi}, repair loop in {repairs}; the torch route differs from the float64 "
          f"definition in {len(left_out)}: {left_out}")
    assert multi > 10 and repairs > 5
    assert len(left_out) <= 0.02 * len(cases)


def test_the_reference_run_through_assign_layers(dev):
    outs, gts, labels = ota_inputs(dev)
    a = assigner()
    layers = [(outs[0], 6), (outs[1], 1), (outs[2], 2)]
    assert a.kernel_route(layers, gts, labels)
    res = a.assign_layers(layers, gts, labels)
    for (_, head_idx), stage in zip(layers, res):
        for b, r in enumerate(stage):
            np.testing.assert_array_equal(r[0].cpu().numpy(), GOLD[f"ota.h{head_idx}.fg{b}"])
            np.testing.assert_array_equal(r[1].cpu().numpy(), GOLD[f"ota.h{head_idx}.gt{b}"])
            assert torch.equal(r.rows, r[0].nonzero().squeeze(1))
    # an empty sample next to a full one
    res = a.assign_layers(layers, [gts[0][:0], gts[1]], [labels[0][:0], labels[1]])
    for (_, head_idx), stage in zip(layers, res):
        np.testing.assert_array_equal(stage[0][0].cpu().numpy(), np.zeros(64, bool))
        assert stage[0][1].numel() == 0 and stage[0][1].dtype == torch.long and stage[0].rows.numel() == 0
        np.testing.assert_array_equal(stage[1][0].cpu().numpy(), GOLD[f"ota.h{head_idx}.fg1"])
        np.testing.assert_array_equal(stage[1][1].cpu().numpy(), GOLD[f"ota.h{head_idx}.gt1"])
    fg, gi = a.single_assigner(outs[0]["pred_boxes"][0], outs[0]["pred_logits"][0], gts[0][:0], labels[0][:0], 6)
    np.testing.assert_array_equal(fg.cpu().numpy(), GOLD["ota.empty.fg"])
    assert gi.numel() == 0


def test_routes_the_kernel_does_not_take(dev, monkeypatch):
    outs, gts, labels = ota_inputs(dev)
    a = assigner()
    layers = [(outs[0], 6)]
    assert a.kernel_route(layers, gts, labels)
    assert not a.kernel_route([({k: v.cpu() for k, v in outs[0].items()}, 6)], [g.cpu() for g in gts], [l.cpu() for l in labels])
    assert not a.kernel_route([({k: v.double() for k, v in outs[0].items()}, 6)], [g.double() for g in gts], labels)
    wide = dict(pred_boxes=outs[0]["pred_boxes"].repeat(1, 65, 1), pred_logits=outs[0]["pred_logits"].repeat(1, 65, 1))   # P = 4160
    assert not a.kernel_route([(wide, 6)], gts, labels)
    other = training.OTAssignerSRFDet(**dict(mf2.OTA_KW, cls_cost=dict(type="ClassificationCost", weight=1.0)))
    assert not other.kernel_route(layers, gts, labels)
    monkeypatch.setenv("SRF_OTA", "0")
    assert not a.kernel_route(layers, gts, labels)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.ota_assign(*[torch.zeros(1)] * 6, **KERNEL_KW, candidate_topk=8, num_heads=6)


def test_loss_ota_on_both_routes(dev, monkeypatch):
    outs, gts, labels = ota_inputs(dev)
    a = assigner()
    check_loss_ota(a, outs, gts, labels, rtol=1e-4)          # the reference's numbers, with the route on

    def run():
        from srfdet3d_amd.plugin import heads
        import make_fixtures as mf
        leaves = [{k: v.clone().requires_grad_() for k, v in o.items()} for o in outs]
        hd = object.__new__(heads.SRFDetHead)
        torch.nn.Module.__init__(hd)
        hd.assigner, hd.num_heads, hd.deep_supervision, hd.num_classes, hd.sync_cls_avg_factor = a, 6, True, 10, True
        hd.pc_range = mf.NUSC_RANGE
        hd.code_weights = torch.nn.Parameter(torch.tensor([1.0] * 8 + [0.2, 0.2], device=dev), requires_grad=False)
        hd.loss_cls = training.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="sum", loss_weight=2.0)
        hd.loss_bbox = training.L1Loss(reduction="sum", loss_weight=0.25)
        boxes = [mf2._GtBoxes(g) for g in gts]
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                losses = hd.loss_ota(dict(leaves[0], aux_outputs=leaves[1:]), boxes, labels)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [str(w.message) for w in seen if "called a synchronizing" in str(w.message)]
        sum(losses.values()).backward()
        return losses, [l[k].grad for l in leaves for k in ("pred_boxes", "pred_logits")], syncs

    monkeypatch.setenv("SRF_OTA", "1")
    on, g_on, syncs_on = run()
    monkeypatch.setenv("SRF_OTA", "0")
    off, g_off, syncs_off = run()
    print(f"loss_ota: host synchronisations with the kernel route {len(syncs_on)}, with the torch route {len(syncs_off)}")
    assert len(syncs_on) == 1, syncs_on                      # the matched counts; everything else stays on the device
    assert len(syncs_off) > 10
    assert set(on) == set(off)
    for k in on:
        assert torch.equal(on[k], off[k]), (k, float(on[k]), float(off[k]))
    for x, y in zip(g_on, g_off):
        assert torch.equal(x, y)


def test_ota_assign_does_not_synchronise_and_repeats_its_bytes(dev):
    c = case("p300", dev)
    t = c["t"]
    args = (t["boxes"], t["logits"], t["gt"], t["labels"], t["n_gt"], t["heads"])
    kw = dict(KERNEL_KW, candidate_topk=O.CFG["candidate_topk"], num_heads=O.CFG["num_heads"])
    ops.ota_assign(*args, **kw)                              # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = ops.ota_assign(*args, **kw)
        second = ops.ota_assign(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert first[0]._base is first[3]._base and tuple(first[0]._base.shape) == (2, 3, 2)
    for x, y in zip(first, second):
        assert x.dtype == torch.int32 and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # and it is the two stages one after the other
    staged = ops.ota_match(c["cost"], c["iou"], t["n_gt"], t["heads"], O.CFG["candidate_topk"], O.CFG["num_heads"])
    for x, y in zip(first, staged):
        assert torch.equal(x, y)
