"""Train-time augmentation on the device: srf_points_augment / srf_boxes_augment / srf_grid_mask bit for bit against numpy
float32 restatements written here, Compose's fused 3-D run against the transforms one by one, the LiDAR-only test pipelines,
PointShuffle, and GridMask inside the LC detector."""
import json
import os

import numpy as np
import pytest
import torch

from srfdet3d_amd import ops, synthetic as S, workloads
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
from srfdet3d_amd.compat.registry import PIPELINES
from srfdet3d_amd.plugin import pipelines as P
from srfdet3d_amd.plugin.grid_mask import GridMask

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NUSC_RANGE = [-55.2, -55.2, -5.0, 55.2, 55.2, 3.0]
F32 = np.float32
PI32 = F32(np.pi)
TWO_PI32 = F32(2 * np.pi)


# ------------------------------------------------------------------------------------------------- numpy restatements
def _aug(angle=0.3, scale=1.05, t=(0.4, -0.7, 0.2)):
    a = torch.tensor(angle, dtype=torch.float32)
    s, c = F32(torch.sin(a).item()), F32(torch.cos(a).item())
    return [s, c, np.arctan2(s, c), F32(scale), F32(t[0]), F32(t[1]), F32(t[2])]


def _np_rotate(x, y, z, s, c):
    z0, one = F32(0), F32(1)
    return (x * c + y * (-s)) + z * z0, (x * s + y * c) + z * z0, (x * z0 + y * z0) + z * one


def _np_xyz(x, y, z, steps, aug):
    s, c, _, sc, tx, ty, tz = [F32(v) for v in aug]
    if steps & ops.AUG_ROTATE:
        x, y, z = _np_rotate(x, y, z, s, c)
    if steps & ops.AUG_SCALE:
        x, y, z = x * sc, y * sc, z * sc
    if steps & ops.AUG_TRANSLATE:
        x, y, z = x + tx, y + ty, z + tz
    if steps & ops.AUG_FLIP_H:
        y = -y
    if steps & ops.AUG_FLIP_V:
        x = -x
    return x, y, z


def np_points_augment(p, steps, aug, pc_range):
    with np.errstate(all="ignore"):
        x, y, z = _np_xyz(p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), steps, aug)
        out = p.copy()
        out[:, 0], out[:, 1], out[:, 2] = x, y, z
        keep = np.ones(len(p), bool)
        if pc_range is not None:
            r = np.asarray(pc_range, F32)
            keep = (x > r[0]) & (y > r[1]) & (z > r[2]) & (x < r[3]) & (y < r[4]) & (z < r[5])
    idx = np.nonzero(keep)[0]
    return out[idx], idx


def np_boxes_augment(b, labels, steps, aug, bev_range, num_classes):
    s, c, yaw_add, sc, tx, ty, tz = [F32(v) for v in aug]
    b = b.copy()
    dim = b.shape[1]
    with np.errstate(all="ignore"):
        if steps & ops.AUG_ROTATE:
            b[:, 0], b[:, 1], b[:, 2] = _np_rotate(b[:, 0].copy(), b[:, 1].copy(), b[:, 2].copy(), s, c)
            b[:, 6] = b[:, 6] + yaw_add
            if dim == 9:
                vx, vy = b[:, 7].copy(), b[:, 8].copy()
                b[:, 7], b[:, 8] = vx * c + vy * (-s), vx * s + vy * c
        if steps & ops.AUG_SCALE:
            b[:, :6] *= sc
            b[:, 7:] *= sc
        if steps & ops.AUG_TRANSLATE:
            b[:, :3] += np.array([tx, ty, tz], F32)
        if steps & ops.AUG_FLIP_H:
            b[:, 1::7] = -b[:, 1::7]
            b[:, 6] = -b[:, 6]
        if steps & ops.AUG_FLIP_V:
            b[:, 0::7] = -b[:, 0::7]
            b[:, 6] = -b[:, 6] + PI32
        keep = np.ones(len(b), bool)
        if bev_range is not None:
            r = np.asarray(bev_range, F32)
            keep = (b[:, 0] > r[0]) & (b[:, 1] > r[1]) & (b[:, 0] < r[2]) & (b[:, 1] < r[3])
            b[:, 6] = b[:, 6] - np.floor(b[:, 6] / TWO_PI32 + F32(0.5)) * TWO_PI32
        if num_classes > 0:
            keep &= (labels >= 0) & (labels < num_classes)
    idx = np.nonzero(keep)[0]
    return b[idx], labels[idx], idx


def np_grid_mask(x, d, l, st_h, st_w, use_h, use_w, mode):
    """grid_mask.py:89-128 literally (rotate = 1: PIL's rotate(0) is a copy), mask crop and all."""
    h, w = x.shape[-2:]
    hh, ww = int(1.5 * h), int(1.5 * w)
    mask = np.ones((hh, ww), np.float32)
    if use_h:
        for i in range(hh // d):
            s = d * i + st_h
            t = min(s + l, hh)
            mask[s:t, :] *= 0
    if use_w:
        for i in range(ww // d):
            s = d * i + st_w
            t = min(s + l, ww)
            mask[:, s:t] *= 0
    mask = np.asarray(np.uint8(mask))
    mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]
    mask = mask.astype(np.float32)
    if mode == 1:
        mask = 1 - mask
    with np.errstate(all="ignore"):
        return x * mask


def _same(a, b):
    """bit for bit, signed zeros included; a NaN must meet a NaN (its payload is the hardware's business)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


# ------------------------------------------------------------------------------------------------- points
def _points(n, nf, seed):
    rng = np.random.default_rng(seed)
    p = np.empty((n, nf), F32)
    p[:, 0:2] = rng.uniform(-62, 62, (n, 2))
    p[:, 2] = rng.uniform(-6, 4, n)
    p[:, 3:] = rng.uniform(0, 255, (n, nf - 3))
    if n >= 16:  # exactly on the range faces, and NaN / inf coordinates
        r = np.asarray(NUSC_RANGE, F32)
        p[0, 0], p[1, 0], p[2, 1], p[3, 1], p[4, 2], p[5, 2] = r[0], r[3], r[1], r[4], r[2], r[5]
        p[6, :3] = [r[0], r[1], r[2]]
        p[7, :3] = [r[3], r[4], r[5]]
        p[8, 0], p[9, 1], p[10, 2] = np.nan, np.nan, np.nan
        p[11, 2] = np.inf
        p[12, 0] = -0.0
    return p


@pytest.mark.parametrize("n", [0, 1, 777, 30000, 300000])
@pytest.mark.parametrize("nf", [4, 5])
def test_points_augment_bit_exact(dev, n, nf):
    p = _points(n, nf, seed=n + nf)
    tp = torch.from_numpy(p).to(dev)
    aug = _aug()
    for steps in range(32):
        for rng in ((NUSC_RANGE, None) if steps in (0, 31) else ((NUSC_RANGE,) if steps % 2 else (None,))):
            want, want_idx = np_points_augment(p, steps, aug, rng)
            got, idx = ops.points_augment(tp, steps, aug, rng, with_index=True)
            assert _same(got.cpu().numpy(), want), (steps, rng)
            assert np.array_equal(idx.cpu().numpy(), want_idx), (steps, rng)


def test_points_augment_on_face_points_under_flips(dev):
    """flips are exact negations and the nuScenes range is symmetric in x / y: points on the faces stay on them"""
    p = _points(64, 5, seed=3)
    tp = torch.from_numpy(p).to(dev)
    for steps in (0, ops.AUG_FLIP_H, ops.AUG_FLIP_V, ops.AUG_FLIP_H | ops.AUG_FLIP_V):
        want, want_idx = np_points_augment(p, steps, _aug(), NUSC_RANGE)
        assert not np.isin(np.arange(8), want_idx).any()
        got, idx = ops.points_augment(tp, steps, _aug(), NUSC_RANGE, with_index=True)
        assert _same(got.cpu().numpy(), want) and np.array_equal(idx.cpu().numpy(), want_idx)


# ------------------------------------------------------------------------------------------------- boxes
def _boxes(n, dim, seed):
    rng = np.random.default_rng(seed)
    b = np.empty((n, dim), F32)
    b[:, 0:2] = rng.uniform(-60, 60, (n, 2))
    b[:, 2] = rng.uniform(-3, 1, n)
    b[:, 3:6] = rng.uniform(0.3, 12, (n, 3))
    b[:, 6] = rng.uniform(-3.3, 3.3, n)
    if dim == 9:
        b[:, 7:9] = rng.normal(0, 5, (n, 2))
    labels = rng.integers(-1, 12, n).astype(np.int64)
    if n >= 16:
        r = np.asarray(NUSC_RANGE, F32)
        b[0, 0], b[1, 0], b[2, 1], b[3, 1] = r[0], r[3], r[1], r[4]   # centres on the BEV faces
        b[4, 6], b[5, 6], b[6, 6], b[7, 6] = PI32, -PI32, np.nextafter(PI32, F32(0)), np.nextafter(-PI32, F32(0))
        b[8, 6], b[9, 6], b[10, 6], b[11, 6] = 0.0, TWO_PI32, F32(3 * np.pi), F32(-2 * np.pi)
        b[12, 6] = np.nextafter(PI32, F32(4))
        labels[13], labels[14], labels[15] = -1, 10, 0
    return b, labels


@pytest.mark.parametrize("n", [0, 1, 37, 5000])
@pytest.mark.parametrize("dim", [7, 9])
def test_boxes_augment_bit_exact(dev, n, dim):
    b, labels = _boxes(n, dim, seed=n + dim)
    tb, tl = torch.from_numpy(b).to(dev), torch.from_numpy(labels).to(dev)
    bev = [NUSC_RANGE[i] for i in (0, 1, 3, 4)]
    aug = _aug(angle=-0.61, scale=0.93, t=(-0.3, 0.25, 0.6))
    for steps in range(32):
        for bev_range, ncls in ((bev, 10), (None, 0), (bev, 0), (None, 10)) if steps in (0, 31) else ((bev, 10) if steps % 2 else (None, 0),):
            wb, wl, wi = np_boxes_augment(b, labels, steps, aug, bev_range, ncls)
            gb, gl, gi = ops.boxes_augment(tb, tl, steps, aug, bev_range, ncls, with_index=True)
            assert _same(gb.cpu().numpy(), wb), (steps, bev_range, ncls)
            assert np.array_equal(gl.cpu().numpy(), wl) and np.array_equal(gi.cpu().numpy(), wi), (steps, bev_range, ncls)


def test_limit_yaw_at_the_period_edges(dev):
    b, labels = _boxes(16, 7, seed=5)
    b[:, :2] = 0.0
    labels[:] = 0
    got, _ = ops.boxes_augment(torch.from_numpy(b).to(dev), torch.from_numpy(labels).to(dev), 0, None, [-1, -1, 1, 1], 1)
    want, _, _ = np_boxes_augment(b, labels, 0, _aug(), [-1, -1, 1, 1], 1)
    assert _same(got.cpu().numpy(), want)
    assert (np.abs(want[:, 6]) <= np.nextafter(PI32, F32(4))).all()  # float32 limit_period may land one ulp beyond pi


# ------------------------------------------------------------------------------------------------- pipelines
def _frame(dev, seed, n_boxes=40, dim=9):
    pts = S.nuscenes_sweep(2000 + seed, 6000)
    b, labels = _boxes(n_boxes, dim, seed)
    return dict(points=torch.from_numpy(pts).to(dev),
                gt_bboxes_3d=LiDARInstance3DBoxes(torch.from_numpy(b).to(dev), box_dim=dim),
                gt_labels_3d=torch.from_numpy(labels).to(dev))


def _decode(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_decode(v) for v in o["__tuple__"])
        return {k: _decode(v) for k, v in o.items()}
    return [_decode(v) for v in o] if isinstance(o, list) else o


def _pipeline(name, which="train_pipeline"):
    """the config's pipeline without the file loaders and the transforms out of scope"""
    with open(os.path.join(HERE, "golden", "reference_pipelines.json")) as f:
        pl = _decode(json.load(f)[name][which])
    return [t for t in pl if not t["type"].startswith("Load") and t["type"] not in ("ObjectSample", "ObjectNoise")]


FUSABLE = ("GlobalRotScaleTrans", "RandomFlip3D", "PointsRangeFilter", "ObjectRangeFilter", "ObjectNameFilter")


@pytest.mark.parametrize("name", ["srfdet_voxel_nusc_L", "srfdet_voxel_kitti_L", "srfdet_dvoxel_waymo_L"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_fused_compose_matches_one_by_one(dev, name, seed):
    cfg = [t for t in _pipeline(name) if t["type"] in FUSABLE]
    fused = P.Compose(cfg)
    assert any(fused._fusable_run(i) - i >= 2 for i in range(len(fused.transforms)))
    single = [PIPELINES.build(t) for t in cfg]
    np.random.seed(seed)
    a = fused(_frame(dev, seed))
    state_a = np.random.get_state()[1].copy()
    np.random.seed(seed)
    b = _frame(dev, seed)
    for t in single:
        b = t(b)
    assert np.array_equal(state_a, np.random.get_state()[1])
    assert _same(a["points"].cpu().numpy(), b["points"].cpu().numpy())
    assert _same(a["gt_bboxes_3d"].tensor.cpu().numpy(), b["gt_bboxes_3d"].tensor.cpu().numpy())
    assert np.array_equal(a["gt_labels_3d"].cpu().numpy(), b["gt_labels_3d"].cpu().numpy())
    for k in ("pcd_rotation_angle", "pcd_scale_factor", "pcd_horizontal_flip", "pcd_vertical_flip", "transformation_3d_flow"):
        assert a.get(k) == b.get(k), k
    assert np.array_equal(a["pcd_trans"], b["pcd_trans"])
    # and the whole chain against numpy from the recorded parameters
    src = _frame(dev, seed)
    p = src["points"].cpu().numpy()
    bx, lab = src["gt_bboxes_3d"].tensor.cpu().numpy(), src["gt_labels_3d"].cpu().numpy()
    aug = _aug(a["pcd_rotation_angle"], a["pcd_scale_factor"], np.asarray(a["pcd_trans"], F32))
    for t in cfg:
        if t["type"] == "GlobalRotScaleTrans":
            steps = 0
            steps |= ops.AUG_ROTATE if a["pcd_rotation_angle"] != 0 else 0
            steps |= ops.AUG_SCALE if F32(a["pcd_scale_factor"]) != 1 else 0
            steps |= ops.AUG_TRANSLATE if np.any(np.asarray(a["pcd_trans"], F32) != 0) else 0
            p, _ = np_points_augment(p, steps, aug, None)
            bx, lab, _ = np_boxes_augment(bx, lab, steps, aug, None, 0)
        elif t["type"] == "RandomFlip3D":
            steps = (ops.AUG_FLIP_H if a["pcd_horizontal_flip"] else 0) | (ops.AUG_FLIP_V if a["pcd_vertical_flip"] else 0)
            p, _ = np_points_augment(p, steps, aug, None)
            bx, lab, _ = np_boxes_augment(bx, lab, steps, aug, None, 0)
        elif t["type"] == "PointsRangeFilter":
            p, _ = np_points_augment(p, 0, aug, t["point_cloud_range"])
        elif t["type"] == "ObjectRangeFilter":
            r = t["point_cloud_range"]
            bx, lab, _ = np_boxes_augment(bx, lab, 0, aug, [r[0], r[1], r[3], r[4]], 0)
        elif t["type"] == "ObjectNameFilter":
            bx, lab, _ = np_boxes_augment(bx, lab, 0, aug, None, len(t["classes"]))
    assert _same(a["points"].cpu().numpy(), p)
    assert _same(a["gt_bboxes_3d"].tensor.cpu().numpy(), bx) and np.array_equal(a["gt_labels_3d"].cpu().numpy(), lab)


@pytest.mark.parametrize("name", ["srfdet_voxel_nusc_L", "srfdet_voxel_kitti_L"])
def test_lidar_only_test_pipeline_runs_unchanged(dev, name):
    pipe = P.Compose(_pipeline(name, "test_pipeline"))
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 30000)).to(dev)
    data = pipe(dict(points=pts))
    got = data["points"][0]
    inner = [t["type"] for t in _pipeline(name, "test_pipeline")[-1]["transforms"]]
    if "PointsRangeFilter" in inner:
        rng = [t for t in _pipeline(name, "test_pipeline")[-1]["transforms"] if t["type"] == "PointsRangeFilter"][0]
        want = ops.points_filter(pts, rng["point_cloud_range"])
        assert _same(got.cpu().numpy(), want.cpu().numpy()) and got.shape[0] < pts.shape[0]
    else:
        assert got is pts
    assert data["img_metas"][0]["pcd_scale_factor"] == 1


def test_point_shuffle(dev):
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 5000)).to(dev)
    t = PIPELINES.build(dict(type="PointShuffle"))
    torch.manual_seed(11)
    a = t(dict(points=pts))["points"]
    torch.manual_seed(11)
    b = t(dict(points=pts))["points"]
    assert torch.equal(a, b) and not torch.equal(a, pts)
    key = lambda x: x[np.lexsort(x.T[::-1])]
    assert _same(key(a.cpu().numpy()), key(pts.cpu().numpy()))


# ------------------------------------------------------------------------------------------------- GridMask
@pytest.mark.parametrize("shape", [(2, 3, 928, 1600), (1, 3, 370, 1224), (1, 3, 37, 53), (2, 2, 5, 3), (1, 1, 31, 4)])
def test_grid_mask_kernel_bit_exact(dev, shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape, dtype=np.float32)
    flat = x.reshape(-1)
    flat[::7] = -0.0
    flat[3::11] = np.nan
    flat[5::13] = -np.inf
    tx = torch.from_numpy(x).to(dev)
    before = tx.clone()
    h = shape[-2]
    for d in sorted({2, 3, max(2, h // 3), h - 1}):
        if d >= h or d < 2:
            continue
        l = min(max(int(d * 0.5 + 0.5), 1), d - 1)
        st = (d - 1, d // 2)
        for mode in (0, 1):
            for use_h, use_w in ((True, True), (True, False), (False, True), (False, False)):
                want = np_grid_mask(x, d, l, st[0], st[1], use_h, use_w, mode)
                got = ops.grid_mask(tx, d, l, st[0], st[1], use_h, use_w, mode)
                assert _same(got.cpu().numpy(), want), (d, mode, use_h, use_w)
    assert _same(tx.cpu().numpy(), before.cpu().numpy())


def test_grid_mask_kernel_unaligned_rows(dev):
    """a view that starts 4 bytes into its storage takes the scalar path"""
    x = torch.randn(1 + 3 * 64 * 96, device=dev)[1:].view(1, 3, 64, 96)
    assert x.data_ptr() % 16 != 0
    got = ops.grid_mask(x, 9, 5, 2, 7, True, True, 1)
    assert _same(got.cpu().numpy(), np_grid_mask(x.cpu().numpy(), 9, 5, 2, 7, True, True, 1))


def test_grid_mask_module_gradient(dev):
    g = GridMask(True, True, mode=1, prob=1.0).train()
    x = torch.randn(2, 3, 40, 56, device=dev, requires_grad=True)
    np.random.seed(4)
    y = g(x)
    np.random.seed(4)
    p = g.draw(40)
    y.backward(torch.ones_like(y))
    mask = np_grid_mask(np.ones((1, 40, 56), np.float32), **{k: p[k] for k in ("d", "l", "st_h", "st_w", "use_h", "use_w", "mode")})
    assert _same(x.grad.cpu().numpy(), np.broadcast_to(mask, (2, 3, 40, 56)).astype(np.float32))


def _lc_model(dev, use_grid_mask):
    torch.manual_seed(0)
    m = workloads.build("srfdet_voxel_nusc_LC", 32)
    m.use_grid_mask = use_grid_mask
    return m.to(dev)


def test_grid_mask_in_the_model(dev):
    img = torch.from_numpy(S.camera_images(3000, h=128, w=224)).to(dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    on, off = _lc_model(dev, True).eval(), _lc_model(dev, False).eval()
    assert on.grid_mask.prob == 0.7 and on.grid_mask.mode == 1
    # eval: GridMask is not called, numpy's RNG is not touched, the features are the same
    np.random.seed(9)
    with torch.no_grad():
        fa = on.extract_img_feat(img, [dict(m) for m in metas])
    assert np.array_equal(np.random.get_state()[1], np.random.RandomState(9).get_state()[1])
    with torch.no_grad():
        fb = off.extract_img_feat(img, [dict(m) for m in metas])
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    # train with prob = 1: the backbone sees exactly img * mask, the caller's img is unchanged
    on.train()
    on.grid_mask.prob = 1.0
    seen = []
    h = on.img_backbone.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().clone()))
    before = img.clone()
    np.random.seed(21)
    with torch.no_grad():
        on.extract_img_feat(img, [dict(m) for m in metas])
    h.remove()
    np.random.seed(21)
    p = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=1.0).draw(128)
    want = np_grid_mask(img.cpu().numpy().reshape(-1, 3, 128, 224), **{k: p[k] for k in ("d", "l", "st_h", "st_w", "use_h",
                                                                                             "use_w", "mode")})
    assert len(seen) == 1 and _same(seen[0].cpu().numpy(), want)
    assert torch.equal(img, before)
