"""The numpy float32 definition of srf_roi_extract_bwd_ordered (tests/roi_bwd_ordered_ref.py) held to the float64 gradient
`roi_ref.grad64` under the rule and constant tests/test_gpu_roi_domain.py::test_backward_against_float64 applies to the atomic route:
|gradient - float64 gradient| <= ROI_BWD_TOL x (the element's sum of |weight * output gradient|).  Runs without a GPU.

The case table: 64 identical RoIs (segments of 64 x several records), RoIs clamped at the last row / column, invalid batch ids, NaN
coordinates and inverted boxes, and a level that receives no RoI.  One planted wrong order (RoIs descending) gives other bits than the
definition on the 64 duplicates: the bit-level assertions of the GPU tests can see order."""
import numpy as np
import pytest
import torch

import roi_bwd_ordered_ref as OR
import roi_ref as RR

TABLE = OR.case_table()
POOL_SR = [(7, 2), (2, 3), (8, 4)]
C = 6


def _gout(R, pooled, seed):
    return np.random.default_rng(seed).standard_normal((R, pooled * pooled, C)).astype(np.float32)


@pytest.mark.parametrize("pooled,sr", POOL_SR)
@pytest.mark.parametrize("name", sorted(TABLE))
def test_definition_against_float64(name, pooled, sr):
    rois = TABLE[name]
    g = _gout(len(rois), pooled, pooled + sr)
    got = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois, g, pooled, sr)
    ref, mag = RR.grad64(OR.SHAPES, OR.STRIDES, torch.from_numpy(rois), torch.from_numpy(g), pooled, sr, OR.FINEST)
    hit = OR.touched(OR.SHAPES, OR.STRIDES, rois, pooled, sr)
    for l in range(4):
        err = ((torch.from_numpy(got[l]).double() - ref[l]).abs() / mag[l].clamp_min(1e-300)).max().item()
        assert err <= OR.ROI_BWD_TOL, f"{name} level {l}: {err:.3e}"
        # the float64 definition's taps are this definition's records: a pixel carries magnitude exactly where a record lands
        assert np.array_equal(hit[l], (mag[l].sum(-1) > 0).numpy()), (name, l)


def test_the_table_holds_what_it_promises():
    lv = {k: RR.levels(torch.from_numpy(v), 4, OR.FINEST).tolist() for k, v in TABLE.items()}
    assert len(TABLE["dup64"]) == 64 and len(np.unique(TABLE["dup64"], axis=0)) == 1
    assert sorted(set(lv["empty_level"])) == [0, 1, 3]                      # a level that receives no RoI
    pooled, sr = 7, 2
    # the duplicates: every touched pixel collects at least 64 records
    lvl, pix, w, live, _ = OR.records(TABLE["dup64"], OR.SHAPES, OR.STRIDES, pooled, sr)
    assert live.any() and np.bincount(pix[live]).max() >= 64 and np.bincount(pix[live])[np.bincount(pix[live]) > 0].min() >= 64
    # the clamped RoIs: samples whose two taps along an axis name the same pixel, the second one with weight 0 and so no record
    lvl, pix, w, live, _ = OR.records(TABLE["clamp"], OR.SHAPES, OR.STRIDES, pooled, sr)
    _, H, W = OR.SHAPES[0]
    q = pix.reshape(-1, 4)
    same = (lvl.reshape(-1, 4)[:, 0] == 0) & live.reshape(-1, 4)[:, 0]
    assert (same & (q[:, 0] % W == W - 1)).any() and (same & ((q[:, 0] // W) % H == H - 1)).any()
    assert not live.reshape(-1, 4)[same & (q[:, 0] % W == W - 1)][:, 1].any()
    # invalid batch ids and NaN coordinates: no record at all; the inverted boxes still sample inside the map
    lvl, pix, w, live, src = OR.records(TABLE["invalid"], OR.SHAPES, OR.STRIDES, pooled, sr)
    per = pooled * pooled * sr * sr * 4
    by_roi = live.reshape(len(TABLE["invalid"]), per).sum(1)
    assert (by_roi[:7] == 0).all() and (by_roi[7:9] > 0).all() and (by_roi[9:] == 0).all()


def test_a_planted_wrong_order_gives_other_bits():
    pooled, sr = 7, 2
    rois = TABLE["dup64"]
    g = _gout(64, pooled, 1)
    want = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois, g, pooled, sr)
    again = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois, g, pooled, sr, rank=np.arange(64 * pooled * pooled * sr * sr * 4))
    wrong = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois, g, pooled, sr, rank=OR.rank_r_descending(64, pooled, sr))
    assert np.array_equal(want[0].view(np.uint32), again[0].view(np.uint32))
    m = OR.touched(OR.SHAPES, OR.STRIDES, rois, pooled, sr)[0]
    differ = (want[0][m].view(np.uint32) != wrong[0][m].view(np.uint32)).mean()
    assert differ > 0.1, differ                                              # other bits ...
    ref, mag = RR.grad64(OR.SHAPES, OR.STRIDES, torch.from_numpy(rois), torch.from_numpy(g), pooled, sr, OR.FINEST)
    err = ((torch.from_numpy(wrong[0]).double() - ref[0]).abs() / mag[0].clamp_min(1e-300)).max().item()
    assert err <= OR.ROI_BWD_TOL                                             # ... of the same sum: only the order is wrong
    print(f"\nplanted order: {100 * differ:.1f} % of level 0's elements differ in bits")


def test_elements_without_a_record_keep_the_fill():
    rois = TABLE["empty_level"]
    g = _gout(len(rois), 2, 3)
    got = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois, g, 2, 3, fill=-7.5)
    hit = OR.touched(OR.SHAPES, OR.STRIDES, rois, 2, 3)
    assert not hit[2].any() and (got[2] == -7.5).all()
    for l in (0, 1, 3):
        assert hit[l].any() and not hit[l].all()
        assert (got[l][~hit[l]] == -7.5).all() and not (got[l][hit[l]] == -7.5).all(-1).any()
