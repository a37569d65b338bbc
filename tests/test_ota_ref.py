"""tests/ota_ref.py against what it restates, on the CPU: `match` is `OTAssignerSRFDet._dynamic_k` (srfdet3d_amd/plugin/training.py) given
the same float32 matrices -- on scattered and crowded scenes, where the multi-match branch and the repair loop both run, and on exact ties
-- it is the reference's per-box top-k loop wherever that is defined (distinct costs), and it reproduces the assignments of the reference
run recorded in tests/golden/extra_r2.npz from that run's own IoU matrices.  This pins the tie rule of `_dynamic_k`: the lower index."""
import os

import numpy as np
import pytest
import torch

import make_fixtures_r2 as mf2
import ota_ref as O
from srfdet3d_amd.plugin import training
from test_fixtures_r2 import GOLD, ota_inputs

SEEDS = range(12)


def assigner():
    return training.OTAssignerSRFDet(**mf2.OTA_KW)


def matrices(case):
    """float32 cost / IoU matrices of a scene: the float64 definition rounded once (any float32 matrices would do here)"""
    boxes, logits, gt, labels = case
    c = O.costs(boxes, logits, gt, labels, **O.CFG)
    return c["cost"].astype(np.float32), c["iou"].astype(np.float32)


def torch_dynamic_k(cost, iou, head_idx):
    fg, j = assigner()._dynamic_k(torch.from_numpy(cost.copy()), torch.from_numpy(iou.copy()), cost.shape[1], head_idx)
    return fg.numpy(), j.numpy()


def test_the_configs_settings():
    kw = mf2.OTA_KW
    assert O.CFG == dict(w_cls=kw["cls_cost"]["weight"], w_reg=kw["reg_cost"]["weight"], w_iou=kw["iou_cost"]["weight"],
                         alpha=kw["cls_cost"]["alpha"], gamma=kw["cls_cost"]["gamma"], eps=kw["cls_cost"]["eps"],
                         center_radius=kw["center_radius"], candidate_topk=kw["candidate_topk"], num_heads=kw["num_heads"])


@pytest.mark.parametrize("gen", ["scattered", "crowded", "with_ties"])
def test_match_is_dynamic_k(gen):
    multi = repairs = 0
    for seed in SEEDS:
        cost, iou = matrices(getattr(O, gen)(seed))
        for head_idx in (1, 3, 6):
            ref = O.match(cost, iou, head_idx, **O.CFG)
            assert ref["status"] == 0, (gen, seed, head_idx)            # the torch loop has no cap: it would not come back
            fg, j = torch_dynamic_k(cost, iou, head_idx)
            assert np.array_equal(fg, ref["fg"]) and np.array_equal(j, ref["gt"]), (gen, seed, head_idx)
            multi += ref["multi"]
            repairs += ref["repairs"] > 0
    print(f"{gen}: multi-match branch in {multi}, repair loop in {repairs} of {3 * len(SEEDS)} calls")
    if gen == "crowded":
        assert multi > 0 and repairs > 0


@pytest.mark.parametrize("gen", ["scattered", "crowded"])
def test_match_is_the_per_box_topk_loop_on_distinct_costs(gen):
    seen = 0
    for seed in SEEDS:
        cost, iou = matrices(getattr(O, gen)(seed))
        ref = O.match(cost, iou, 4, **O.CFG)
        if any(np.unique(cost[:, g]).size != cost.shape[0] for g in range(cost.shape[1])):
            continue
        fg, j = O.match_by_column_loop(cost, iou, 4, O.CFG["candidate_topk"], O.CFG["num_heads"])
        assert np.array_equal(fg, ref["fg"]) and np.array_equal(j, ref["gt"]), (gen, seed)
        seen += 1
    assert seen >= len(SEEDS) // 2


def test_duplicated_predictions_the_lower_index_wins():
    """Four predictions, one box, k = 1: rows 0 and 1 are the same prediction.  The stable sort of `_dynamic_k` ranks row 0 first."""
    cost = np.array([[1.0], [1.0], [2.0], [3.0]], np.float32)
    iou = np.array([[0.9], [0.9], [0.1], [0.0]], np.float32)
    ref = O.match(cost, iou, 6, candidate_topk=8, num_heads=6)            # sum of IoUs 1.9 -> k = 1
    assert ref["fg"].tolist() == [True, False, False, False] and ref["gt"].tolist() == [0] and ref["gap"] == 0.0
    fg, j = torch_dynamic_k(cost, iou, 6)
    assert fg.tolist() == ref["fg"].tolist() and j.tolist() == [0]
    # two boxes that both rank the duplicated pair first: both rows are multi-matched, each keeps its arg-min column -- the lower one on a tie
    cost = np.array([[1.0, 1.0], [1.0, 1.0], [2.0, 5.0], [3.0, 4.0]], np.float32)
    iou = np.array([[0.9, 0.9], [0.9, 0.9], [0.8, 0.1], [0.0, 0.0]], np.float32)
    ref = O.match(cost, iou, 6, candidate_topk=8, num_heads=6)            # k = 2, 1: box 0 takes rows 0, 1; box 1 takes row 0
    fg, j = torch_dynamic_k(cost, iou, 6)
    assert fg.tolist() == ref["fg"].tolist() and j.tolist() == ref["gt"].tolist()
    assert ref["multi"] and ref["repairs"] >= 1


def test_the_cap():
    """One prediction, two boxes: the row is multi-matched, keeps box 0, and every repair hands it to box 1 and takes it back."""
    cost = np.array([[1.0, 2.0]], np.float32)
    iou = np.array([[0.5, 0.5]], np.float32)
    ref = O.match(cost, iou, 6, candidate_topk=8, num_heads=6)
    assert ref["status"] == 1 and ref["repairs"] == O.CAP and ref["fg"].tolist() == [True] and ref["gt"].tolist() == [0]


def test_empty():
    ref = O.match(np.zeros((5, 0), np.float32), np.zeros((5, 0), np.float32), 3)
    assert ref["fg"].tolist() == [False] * 5 and ref["gt"].size == 0 and ref["status"] == 0


def test_match_reproduces_the_reference_run(monkeypatch):
    """The fixture's own IoU matrices in, the fixture's assignments out: the cost is the torch route's on the CPU around those matrices."""
    outs, gts, labels = ota_inputs()
    a = assigner()
    for head_idx, o in ((6, outs[0]), (1, outs[1]), (2, outs[2])):
        for b in range(2):
            iou = GOLD[f"ota.h{head_idx}.iou{b}"]
            monkeypatch.setattr(training, "bbox_overlaps_3d", lambda p, g, iou=iou: torch.from_numpy(iou.copy()))
            cost, ious = a.cost_matrices(o["pred_boxes"][b], o["pred_logits"][b], gts[b], labels[b])
            ref = O.match(cost.numpy(), ious.numpy(), head_idx, **O.CFG)
            assert ref["status"] == 0
            np.testing.assert_array_equal(ref["fg"], GOLD[f"ota.h{head_idx}.fg{b}"])
            np.testing.assert_array_equal(ref["gt"], GOLD[f"ota.h{head_idx}.gt{b}"])
