"""Train-time augmentation, host side (no GPU): every transform of the reference's train / test pipelines that this project
covers builds from its unchanged config dict, the numpy draws happen in the documented order, and the new C entry points
refuse bad arguments before any HIP call.  The device half is tests/test_gpu_augment.py."""
import json
import os

import numpy as np
import pytest
import torch

from srfdet3d_amd import _lib, ops
from srfdet3d_amd.compat.registry import PIPELINES
from srfdet3d_amd.plugin import pipelines as P
from srfdet3d_amd.plugin.grid_mask import GridMask

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_pipelines.json")

# not built here: file loaders (host I/O) and the transforms this project leaves out (a GT database on disk, KITTI-only
# object noise, 2-D image resize / normalise / pad of waymo_LC and kitti_LC)
OUT_OF_SCOPE = {"ObjectSample", "ObjectNoise", "ResizeImageMultiViewImage", "Normalize", "Pad"}


def _decode(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_decode(v) for v in o["__tuple__"])
        return {k: _decode(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_decode(v) for v in o]
    return o


def _pipelines():
    with open(FIXTURE) as f:
        return {k: _decode(v) for k, v in json.load(f).items()}


def _covered(t):
    return not t["type"].startswith("Load") and t["type"] not in OUT_OF_SCOPE


def _build_all(transforms, seen):
    for t in transforms:
        if not _covered(t):
            continue
        seen.add(t["type"])
        obj = PIPELINES.build(t)
        assert obj is not None
        if t["type"] == "MultiScaleFlipAug3D":
            inner = [u for u in t["transforms"] if _covered(u)]
            _build_all(inner, seen)
            PIPELINES.build(dict(t, transforms=inner))


def test_fixture_covers_the_eleven_configs():
    pl = _pipelines()
    assert len(pl) == 11
    for name, v in pl.items():
        assert v["train_pipeline"] and v["test_pipeline"], name


@pytest.mark.parametrize("name", sorted(_pipelines()))
def test_every_covered_transform_builds_from_its_config_dict(name):
    v = _pipelines()[name]
    seen = set()
    _build_all(v["train_pipeline"], seen)
    _build_all(v["test_pipeline"], seen)
    assert seen


def test_the_new_transforms_are_registered():
    for t in ("GlobalRotScaleTrans", "RandomFlip3D", "ObjectRangeFilter", "ObjectNameFilter", "PointShuffle"):
        assert PIPELINES.get(t) is not None, t
    seen = set()
    for v in _pipelines().values():
        _build_all(v["train_pipeline"] + v["test_pipeline"], seen)
    assert {"GlobalRotScaleTrans", "RandomFlip3D", "ObjectRangeFilter", "ObjectNameFilter", "PointShuffle",
            "PointsRangeFilter", "MultiScaleFlipAug3D"} <= seen


def test_compose_fuses_the_adjacent_3d_transforms():
    pl = _pipelines()
    nusc = P.Compose([t for t in pl["srfdet_voxel_nusc_L"]["train_pipeline"] if _covered(t)])
    names = [type(t).__name__ for t in nusc.transforms]
    assert names[:5] == ["GlobalRotScaleTrans", "RandomFlip3D", "PointsRangeFilter", "ObjectRangeFilter", "ObjectNameFilter"]
    assert nusc._fusable_run(0) == 5
    # kitti flips before it rotates: the flip runs on its own, the rest fuses
    kitti = P.Compose([t for t in pl["srfdet_voxel_kitti_L"]["train_pipeline"] if _covered(t)])
    names = [type(t).__name__ for t in kitti.transforms]
    assert names[:2] == ["RandomFlip3D", "GlobalRotScaleTrans"]
    assert kitti._fusable_run(0) == 1 and kitti._fusable_run(1) == 5
    # the LC test pipeline's lone PointsRangeFilter stays a run of one
    lc = P.Compose([t for t in pl["srfdet_voxel_nusc_LC"]["test_pipeline"][-1]["transforms"] if _covered(t)])
    assert lc._fusable_run(0) == 1


# ------------------------------------------------------------------------------------------------------ draw order
def _grst_expected(seed, rot, scale_range, std, preset_scale=None):
    rs = np.random.RandomState(seed)
    angle = rs.uniform(rot[0], rot[1])
    scale = preset_scale if preset_scale is not None else rs.uniform(scale_range[0], scale_range[1])
    trans = rs.normal(scale=np.array(std, dtype=np.float32), size=3)
    return angle, scale, trans, rs.rand()


@pytest.mark.parametrize("seed", [0, 1, 7, 12345])
@pytest.mark.parametrize("preset", [None, 1.0])
def test_global_rot_scale_trans_draws(seed, preset):
    t = PIPELINES.build(dict(type="GlobalRotScaleTrans", rot_range=[-0.785, 0.785], scale_ratio_range=[0.9, 1.1],
                             translation_std=[0.5, 0.5, 0.5]))
    results = {} if preset is None else dict(pcd_scale_factor=preset)
    np.random.seed(seed)
    sin, cos, yaw_add, rotate_points = t.draw(results)
    after = np.random.rand()
    angle, scale, trans, next_draw = _grst_expected(seed, [-0.785, 0.785], [0.9, 1.1], [0.5, 0.5, 0.5], preset)
    assert after == next_draw  # nothing else was drawn
    assert results["pcd_rotation_angle"] == angle
    assert results["pcd_scale_factor"] == scale
    assert np.array_equal(results["pcd_trans"], trans)
    assert results["transformation_3d_flow"] == ["R", "S", "T"]
    a32 = torch.tensor(angle, dtype=torch.float32)
    assert sin == np.float32(torch.sin(a32).item()) and cos == np.float32(torch.cos(a32).item())
    assert yaw_add == np.arctan2(sin, cos) and yaw_add.dtype == np.float32
    rot = results["pcd_rotation"]
    assert rot.dtype == torch.float32 and rot.shape == (3, 3)
    assert rot[0, 0].item() == cos and rot[0, 1].item() == sin and rot[1, 0].item() == -sin and rot[2, 2].item() == 1
    assert rotate_points


def test_global_rot_scale_trans_keeps_points_unrotated_with_an_empty_box_field():
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    t = PIPELINES.build(dict(type="GlobalRotScaleTrans"))
    results = dict(gt_bboxes_3d=LiDARInstance3DBoxes(torch.zeros((0, 9)), box_dim=9))
    np.random.seed(3)
    *_, rotate_points = t.draw(results)
    assert not rotate_points and "pcd_rotation" not in results and "pcd_rotation_angle" in results


def test_identity_parameters_plan_nothing():
    t = PIPELINES.build(dict(type="GlobalRotScaleTrans", rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]))
    f = PIPELINES.build(dict(type="RandomFlip3D"))
    results = dict(flip=False, pcd_scale_factor=1, pcd_horizontal_flip=False, pcd_vertical_flip=False)
    plan = P._AugPlan()
    np.random.seed(0)
    t._plan(results, plan)
    f._plan(results, plan)
    assert plan.pts_steps == 0 and plan.box_steps == 0
    # with nothing to do the plan never touches the points: a CPU tensor goes through untouched
    pts = torch.zeros((4, 5))
    assert plan.run(dict(points=pts))["points"] is pts


@pytest.mark.parametrize("seed", [0, 3, 99])
def test_random_flip_3d_draws_sync_2d_false(seed):
    f = PIPELINES.build(dict(type="RandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5))
    results = {}
    np.random.seed(seed)
    f.draw(results)
    rs = np.random.RandomState(seed)
    cur = rs.choice(["horizontal", None], p=[0.5, 0.5])
    h = rs.rand() < 0.5
    v = rs.rand() < 0.5
    assert results["flip"] == (cur is not None) and results["flip_direction"] == cur
    assert results["pcd_horizontal_flip"] == h and results["pcd_vertical_flip"] == v
    assert results["transformation_3d_flow"] == (["HF"] if h else []) + (["VF"] if v else [])
    assert np.random.rand() == rs.rand()


@pytest.mark.parametrize("seed", [0, 3, 99])
def test_random_flip_3d_draws_sync_2d(seed):
    f = PIPELINES.build(dict(type="RandomFlip3D", flip_ratio_bev_horizontal=0.5))  # kitti_L
    results = {}
    np.random.seed(seed)
    f.draw(results)
    rs = np.random.RandomState(seed)
    cur = rs.choice(["horizontal", None], p=[0.5, 0.5])
    assert results["pcd_horizontal_flip"] == (cur is not None) and results["pcd_vertical_flip"] is False
    assert np.random.rand() == rs.rand()


def test_random_flip_3d_preset_flags_draw_nothing():
    f = PIPELINES.build(dict(type="RandomFlip3D", sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5))
    results = dict(flip=False, pcd_horizontal_flip=True, pcd_vertical_flip=False)
    np.random.seed(5)
    f.draw(results)
    assert np.random.rand() == np.random.RandomState(5).rand()
    assert results["pcd_horizontal_flip"] and results["transformation_3d_flow"] == ["HF"]


def test_random_flip_3d_refuses_to_flip_images():
    f = PIPELINES.build(dict(type="RandomFlip3D", flip_ratio_bev_horizontal=1.0))
    with pytest.raises(NotImplementedError):
        f.draw(dict(img=torch.zeros(1)))
    f.draw(dict(img=torch.zeros(1), img_fields=[]))  # no image field to flip


@pytest.mark.parametrize("seed", [0, 1, 2024])
def test_grid_mask_draws(seed):
    g = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
    np.random.seed(seed)
    params = g.draw(928)
    rs = np.random.RandomState(seed)
    if rs.rand() > 0.7:
        assert params is None
    else:
        d = rs.randint(2, 928)
        st_h, st_w = rs.randint(d), rs.randint(d)
        rs.randint(1)
        assert params == dict(d=d, l=min(max(int(d * 0.5 + 0.5), 1), d - 1), st_h=st_h, st_w=st_w, use_h=True, use_w=True,
                              mode=1)
    assert np.random.rand() == rs.rand()


def test_grid_mask_is_identity_in_eval_and_draws_nothing():
    g = GridMask(True, True, mode=1, prob=1.0).eval()
    x = torch.ones(1, 3, 8, 8)
    state = np.random.get_state()[1].copy()
    assert g(x) is x
    assert np.array_equal(np.random.get_state()[1], state)


def test_grid_mask_set_prob_and_refusals():
    g = GridMask(True, True, prob=0.7)
    g.set_prob(3, 6)
    assert g.prob == 0.7 * 3 / 6
    with pytest.raises(NotImplementedError):
        GridMask(True, True, rotate=2)
    with pytest.raises(NotImplementedError):
        GridMask(True, True, offset=True)


# ------------------------------------------------------------------------------------------------------ C ABI
def test_augment_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    hf = _lib.hf
    aug = hf([0, 1, 0, 1, 0, 0, 0])
    assert L.srf_points_augment_workspace_bytes(300000) >= 8 and L.srf_points_augment_workspace_bytes(-1) == 0
    assert L.srf_boxes_augment_workspace_bytes(5000) >= 8 and L.srf_boxes_augment_workspace_bytes(-1) == 0
    assert L.srf_points_augment(None, 10, 2, 1, aug, None, None, None, None, None, None) == -1     # nf < 3
    assert L.srf_points_augment(None, -1, 4, 1, aug, None, None, None, None, None, None) == -1     # n < 0
    assert L.srf_points_augment(None, 10, 4, 32, aug, None, None, None, None, None, None) == -1    # unknown step bit
    assert L.srf_points_augment(None, 10, 4, 1, None, None, None, None, None, None, None) == -1    # steps without aug
    assert L.srf_points_augment(None, 10, 4, 1, aug, None, None, None, None, None, None) == -1     # no counter
    assert L.srf_boxes_augment(None, None, 10, 8, 1, aug, None, 0, None, None, None, None, None, None) == -1  # box_dim
    assert L.srf_boxes_augment(None, None, 10, 7, 64, aug, None, 0, None, None, None, None, None, None) == -1
    assert L.srf_boxes_augment(None, None, 10, 9, 3, None, None, 0, None, None, None, None, None, None) == -1
    assert L.srf_boxes_augment(None, None, -2, 9, 0, None, None, 0, None, None, None, None, None, None) == -1
    assert L.srf_grid_mask(None, 6, 928, 1600, 1, 1, 0, 0, 1, 1, 1, None, None) == -1    # d < 2
    assert L.srf_grid_mask(None, 6, 928, 1600, 10, 10, 0, 0, 1, 1, 1, None, None) == -1  # l >= d
    assert L.srf_grid_mask(None, 6, 928, 1600, 10, 0, 0, 0, 1, 1, 1, None, None) == -1   # l < 1
    assert L.srf_grid_mask(None, 6, 928, 1600, 10, 5, 10, 0, 1, 1, 1, None, None) == -1  # st_h >= d
    assert L.srf_grid_mask(None, 6, 928, 1600, 10, 5, 0, -1, 1, 1, 1, None, None) == -1  # st_w < 0
    assert L.srf_grid_mask(None, 6, 928, 1600, 10, 5, 0, 0, 1, 1, 2, None, None) == -1   # mode
    assert L.srf_grid_mask(None, 6, 0, 1600, 10, 5, 0, 0, 1, 1, 1, None, None) == -1     # H
    assert L.srf_grid_mask(None, 6, 928, 1600, 10, 5, 0, 0, 1, 1, 1, None, None) == -1   # no buffers
    assert L.srf_grid_mask(None, 0, 928, 1600, 10, 5, 0, 0, 1, 1, 1, None, None) == 0    # no planes: nothing to do


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU"):
        ops.points_augment(torch.zeros((4, 5)), ops.AUG_ROTATE, [0, 1, 0, 1, 0, 0, 0])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.boxes_augment(torch.zeros((4, 9)), torch.zeros(4, dtype=torch.int64), 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.grid_mask(torch.zeros((1, 3, 8, 8)), 4, 2, 0, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        PIPELINES.build(dict(type="PointShuffle"))(dict(points=torch.zeros((4, 5))))
