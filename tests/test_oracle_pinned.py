"""Pin the decoder-side oracle (oracle/decoder_oracle.py) to arrays produced by the reference's own Python."""
import os

import numpy as np
import pytest

import detgen
from make_fixtures import NUSC_RANGE, NUSC_VOXEL, det_boxes
from oracle import decoder_oracle as DO
from srfdet3d_amd import synthetic as S

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "decoder_nusc.npz"))
P = 48


def test_corners_pinned():
    b = det_boxes("boxutil.boxes", P)
    b[..., :3] = b[..., :3] * 100.0 - 50.0
    np.testing.assert_allclose(DO.corners3d(b), GOLD["corners3d"], rtol=1e-6, atol=2e-5)


def test_lidar_rois_pinned():
    rois, bm = DO.lidar_rois(det_boxes("lstage.boxes", P), NUSC_RANGE, NUSC_VOXEL)
    np.testing.assert_allclose(rois, GOLD["lstage.rois"], rtol=0, atol=2e-3)
    np.testing.assert_allclose(bm, GOLD["lstage.boxes_after"], rtol=1e-6, atol=1e-5)
    rois, _ = DO.lidar_rois(det_boxes("fstage.boxes", P), NUSC_RANGE, NUSC_VOXEL)
    np.testing.assert_allclose(rois, GOLD["fstage.rois_lidar"], rtol=0, atol=2e-3)


def test_image_rois_pinned():
    got = DO.image_rois(det_boxes("fstage.boxes", P), NUSC_RANGE, S.camera_rig()[None])
    ref = GOLD["fstage.rois_img"]
    np.testing.assert_array_equal(got[:, 0], ref[:, 0])
    np.testing.assert_allclose(got[:, 1:], ref[:, 1:], rtol=2e-4, atol=5e-2)


def _head_and_feats():
    import torch
    import detgen
    from test_decoder_fixtures import _nusc_head
    hd = _nusc_head(32)
    detgen.load_det_params(hd, "head.")
    feats = [torch.from_numpy(detgen.det(f"head.feat{i}", (1, 128, s, s), scale=0.5)) for i, s in enumerate((184, 92, 46, 23))]
    return hd, feats


def test_cpu_head_stage_by_stage_matches_reference():
    """oracle/pipeline.py:head_forward (the CPU path the GPU is compared with) vs the reference's own 5-stage loop,
    each stage fed the inputs the reference's stage saw: box params within 1e-4 (the north-star tolerance)."""
    from oracle import pipeline
    hd, feats = _head_and_feats()
    forced = list(zip(GOLD["head.stage_in_boxes"], GOLD["head.stage_in_prop"]))
    cap = []
    logits, boxes = pipeline.head_forward(hd, None, feats, None, capture=cap, stage_inputs=forced)
    np.testing.assert_allclose(np.stack([c["rois"] for c in cap]), GOLD["head.rois"], rtol=1e-6, atol=2e-3)
    np.testing.assert_allclose(boxes.numpy(), GOLD["head.boxes"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(logits.numpy(), GOLD["head.logits"], rtol=1e-4, atol=1e-4)


def test_cpu_head_free_running_matches_reference():
    """The same loop free-running.  With seeded RANDOM weights (no checkpoint exists offline) every stage amplifies
    float rounding by about 10x (boxes move by metres per stage), so the 1e-4 contract holds for the first stages
    and the last stage is only checked loosely; this documents the sensitivity rather than hiding it."""
    from oracle import pipeline
    hd, feats = _head_and_feats()
    logits, boxes = pipeline.head_forward(hd, None, feats, None)
    np.testing.assert_allclose(boxes.numpy()[:2], GOLD["head.boxes"][:2], rtol=0, atol=1e-4)
    np.testing.assert_allclose(boxes.numpy()[4], GOLD["head.boxes"][4], rtol=0, atol=0.5)


# ---- the damped, trained-like fixture (tests/golden/make_free_fixture.py): the loop as a whole, at half the contract ----
FREE = np.load(os.path.join(os.path.dirname(__file__), "golden", "decoder_free.npz"))


@pytest.mark.parametrize("case", list(detgen.FREE_CASES))
def test_free_fixture_conditions_hold(case):
    """the conditions the generator checked on the reference's run before it wrote the file, re-asserted from `meta.*`"""
    P, bs, fusion = detgen.FREE_CASES[case]
    m = {k.split(".", 2)[2]: FREE[k] for k in FREE.files if k.startswith(f"meta.{case}.")}
    assert detgen.free_damping(FREE["meta.damping"]) in detgen.FREE_DAMPINGS
    assert FREE[f"{case}.boxes"].shape == (5, bs, P, 10) and FREE[f"{case}.boxes"].dtype == np.float32
    assert float(m["margin"]) >= 2e-4                 # no RoI near a pyramid-level boundary: a flip cannot happen
    assert m["bev_levels"].shape == (5, 4) and (m["bev_levels"].sum(1) == bs * P).all()
    assert (m["bev_levels"].min(1) >= 0.01 * bs * P).all()   # every stage uses all four levels
    assert float(m["move"].min()) >= 0.1              # >= 1000 x the tolerance of movement at every hand-over
    assert int(m["clamped"]) >= 3
    if bs > 1:
        assert float(m["samples_apart"]) >= 0.1
    if fusion:
        assert (m["img_levels"].sum(1) == 6 * bs * P).all()
        # the seed that passed still exercises the hard camera geometry: at every stage more than 5 % of the (box, camera) pairs
        # straddle the camera's image plane (134 of 1200 at stage 1) and more than a quarter of the image RoIs are wider than
        # 1e4 px (676 of 1200)
        assert (m["img_rois_crossing"] > 0.05 * 6 * bs * P).all() and (m["img_rois_wide"] > 0.25 * 6 * bs * P).all()
        wide = [int(((r[:, 3] - r[:, 1]) > 1e4).sum()) for r in FREE[f"{case}.rois_img"]]
        assert wide == m["img_rois_wide"].tolist()
    assert float(m["cpu_box_diff"].max()) <= 5e-5 and float(m["cpu_decode_diff"].max()) <= 5e-5
    # the fixture's own sensitivity: the reference against itself on inputs perturbed at rounding level (1e-6 relative on the
    # feature maps, one float32 epsilon on the camera matrices) stays within half the contract, so the other half is the kernels'
    assert float(m["perturbed_box_diff"].max()) <= 5e-5 and float(m["perturbed_decode_diff"].max()) <= 5e-5
    # the stored RoIs are the ones the margin was computed from
    margins = [detgen.level_stats(FREE[f"{case}.rois_bev"][s])[1] for s in range(5)]
    if fusion:
        margins += [detgen.level_stats(FREE[f"{case}.rois_img"][s])[1] for s in range(5)]
    assert min(margins) == pytest.approx(float(m["margin"]), rel=1e-5)


@pytest.mark.parametrize("case", list(detgen.FREE_CASES))
def test_cpu_head_free_running_matches_reference_on_damped_fixture(case):
    """oracle/pipeline.head_forward FREE-RUNNING over five stages against the reference's own run: boxes within 5e-5 (half
    the 1e-4 contract, so that the GPU tests' 1e-4 is not used up by the fixture's own sensitivity), logits within half of
    the GPU tests' logit tolerance.  This pins the oracle pipeline and the host-side stage arithmetic chained over five
    stages, for the LiDAR head at P = 200 / 900 / bs = 2 and the fusion head.  Measured: see `meta.<case>.cpu_box_diff`."""
    from detgen import free_metas, repo_head
    from oracle import pipeline
    import torch
    P, bs, fusion = detgen.FREE_CASES[case]
    k = int(FREE[f"meta.{case}.seed"])
    bev, img = detgen.free_inputs(case, k)
    hd = repo_head(case, k, detgen.free_damping(FREE["meta.damping"]))
    logits, boxes = pipeline.head_forward(hd, [torch.from_numpy(f) for f in img] if fusion else None,
                                          [torch.from_numpy(f) for f in bev], free_metas(bs))
    d = np.abs(boxes.numpy() - FREE[f"{case}.boxes"]).max(axis=(1, 2, 3))
    print(f"\n[free] cpu {case}: boxes per stage {d.tolist()}")
    np.testing.assert_allclose(boxes.numpy(), FREE[f"{case}.boxes"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(logits.numpy(), FREE[f"{case}.logits"], rtol=5e-5, atol=1.5e-4 if fusion else 1e-4)
    with torch.no_grad():
        scores, dec = hd.decode(logits, boxes.clone())     # the pre-NMS pair of the reference's get_bboxes
    np.testing.assert_allclose(dec.numpy(), FREE[f"{case}.dec_boxes"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(scores.numpy(), FREE[f"{case}.dec_scores"], rtol=0, atol=5e-5)
