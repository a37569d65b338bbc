"""numpy restatements of mmdet3d's GT-database sampling and object noise (box_collision_test, sample_class_v2, noise_per_box,
points_in_rbbox, points_transform_), float64 geometry for the invariant tests, and a writer for a synthetic GT database
(pickle + .bin files) in a temporary directory.  The float32 arithmetic follows the order the kernels document
(csrc/objsample.hip), so the device results must match bit for bit."""
import os
import pickle

import numpy as np

F32 = np.float32
NUSC_CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                "traffic_cone"]
# srfdet_voxel_nusc_L's sample_groups in config order (the pipeline fixture stores dict keys sorted)
NUSC_GROUPS = dict(car=2, truck=3, construction_vehicle=7, bus=4, trailer=6, barrier=2, motorcycle=6, bicycle=6, pedestrian=2,
                   traffic_cone=2)
KITTI_CLASSES = ["Pedestrian", "Cyclist", "Car"]


# ------------------------------------------------------------------------------------------------- points in boxes
def np_points_in_boxes(points, planes, mask=None):
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    idx = np.full(len(points), -1, np.int32)
    for b in reversed(range(len(planes))):
        if mask is not None and not mask[b]:
            continue
        inside = np.ones(len(points), bool)
        for f in range(6):
            a, bb, c, d = (F32(v) for v in planes[b, f])
            with np.errstate(all="ignore"):
                inside &= (((x * a + y * bb) + z * c) + d) < 0
        idx[inside] = b
    return idx


# ------------------------------------------------------------------------------------------------- collisions
def _ccw(A, C, D):
    return (D[:, 1] - A[:, 1]) * (C[:, 0] - A[:, 0]) > (C[:, 1] - A[:, 1]) * (D[:, 0] - A[:, 0])


def _contains(a, q):
    ok = np.ones(len(a), bool)
    for l in range(4):
        for k in range(4):
            k1 = (k + 1) % 4
            v = -(a[:, k] - a[:, k1])
            cross = v[:, 1] * (a[:, k, 0] - q[:, l, 0])
            cross = cross - v[:, 0] * (a[:, k, 1] - q[:, l, 1])
            ok &= ~(cross >= 0)
    return ok


def np_collide(a, q):
    """box_collision_test for the pairs (a[p], q[p]), both (P, 4, 2) float32 -> bool (P,)"""
    a, q = np.asarray(a, F32), np.asarray(q, F32)
    amin, amax, qmin, qmax = a.min(1), a.max(1), q.min(1), q.max(1)
    iw = np.minimum(amax[:, 0], qmax[:, 0]) - np.maximum(amin[:, 0], qmin[:, 0])
    ih = np.minimum(amax[:, 1], qmax[:, 1]) - np.maximum(amin[:, 1], qmin[:, 1])
    edge = np.zeros(len(a), bool)
    for k in range(4):
        A, B = a[:, k], a[:, (k + 1) % 4]
        for l in range(4):
            C, D = q[:, l], q[:, (l + 1) % 4]
            edge |= (_ccw(A, C, D) != _ccw(B, C, D)) & (_ccw(A, B, C) != _ccw(A, B, D))
    return (iw > 0) & (ih > 0) & (edge | _contains(a, q) | _contains(q, a))


def np_collision_matrix(boxes, qboxes):
    N, K = len(boxes), len(qboxes)
    a = np.repeat(np.asarray(boxes, F32), K, 0)
    q = np.tile(np.asarray(qboxes, F32), (N, 1, 1))
    return np_collide(a, q).reshape(N, K)


def np_accept(fixed, cand, offsets):
    """sample_all's loop over classes with sample_class_v2's coll_mat walk, literally"""
    avoid = np.asarray(fixed, F32).reshape(-1, 4, 2)
    accept = np.zeros(len(cand), np.int32)
    for c in range(len(offsets) - 1):
        cb, ce = offsets[c], offsets[c + 1]
        if ce <= cb:
            continue
        num_gt = len(avoid)
        total = np.concatenate([avoid, cand[cb:ce]])
        coll = np_collision_matrix(total, total)
        coll[np.arange(len(total)), np.arange(len(total))] = False
        valid = []
        for i in range(num_gt, len(total)):
            if coll[i].any():
                coll[i] = False
                coll[:, i] = False
            else:
                valid.append(i - num_gt)
        for v in valid:
            accept[cb + v] = 1
        if valid:
            avoid = np.concatenate([avoid, cand[cb:ce][valid]])
    return accept


# ------------------------------------------------------------------------------------------------- object noise
def np_try_corners(base, bx, by, s, c, loc):
    """(T, 4, 2) corners of the tries of one box: base (4, 2), centre bx, by (float32), s, c (T,) float32, loc (T, 3) float64"""
    x, y = base[None, :, 0] - bx, base[None, :, 1] - by
    s, c = s[:, None], c[:, None]
    rx, ry = x * c + y * (-s), x * s + y * c
    tx, ty = np.float64(bx) + loc[:, 0:1], np.float64(by) + loc[:, 1:2]
    return np.stack([(rx.astype(np.float64) + tx).astype(F32), (ry.astype(np.float64) + ty).astype(F32)], -1)


def np_object_noise(points, boxes, corners, planes, rot, loc):
    """noise_per_box + points_transform_ + box3d_transform_ -> (points, boxes, chosen)"""
    m, T = rot.shape
    s_all, c_all = np.sin(rot).astype(F32), np.cos(rot).astype(F32)
    cur = corners.copy()
    chosen = np.full(m, -1, np.int32)
    for i in range(m):
        tries = np_try_corners(cur[i], boxes[i, 0], boxes[i, 1], s_all[i], c_all[i], loc[i])
        others = np.array([k for k in range(m) if k != i], int)
        if len(others):
            coll = np_collide(np.repeat(tries, len(others), 0), np.tile(cur[others], (T, 1, 1))).reshape(T, len(others)).any(1)
        else:
            coll = np.zeros(T, bool)
        free = np.nonzero(~coll)[0]
        if len(free):
            chosen[i] = free[0]
            cur[i] = tries[free[0]]
    out = points.copy()
    idx = np_points_in_boxes(points, planes)
    sel = idx >= 0
    b = idx[sel]
    j = chosen[b]
    ok = j >= 0
    jj = np.where(ok, j, 0)
    s = np.where(ok, s_all[b, jj], F32(0)).astype(F32)
    c = np.where(ok, c_all[b, jj], F32(1)).astype(F32)
    lo = np.where(ok[:, None], loc[b, jj], 0.0)
    ctr = boxes[b, :3]
    x, y, z = points[sel, 0] - ctr[:, 0], points[sel, 1] - ctr[:, 1], points[sel, 2] - ctr[:, 2]
    z0, one = F32(0), F32(1)
    nx = (x * c + y * (-s)) + z * z0
    ny = (x * s + y * c) + z * z0
    nz = (x * z0 + y * z0) + z * one
    for d, v in enumerate((nx, ny, nz)):
        out[sel, d] = ((v + ctr[:, d]).astype(np.float64) + lo[:, d]).astype(F32)
    ob = boxes.copy()
    okb = chosen >= 0
    jb = np.where(okb, chosen, 0)
    lb = np.where(okb[:, None], loc[np.arange(m), jb], 0.0)
    rb = np.where(okb, rot[np.arange(m), jb], 0.0)
    ob[:, :3] = (boxes[:, :3].astype(np.float64) + lb).astype(F32)
    ob[:, 6] = (boxes[:, 6].astype(np.float64) + rb).astype(F32)
    return out, ob, chosen


# ------------------------------------------------------------------------------------------------- float64 geometry
def corners64(boxes):
    """(n, >= 7) -> (n, 4, 2) float64 BEV corners, counter-clockwise by the yaw"""
    b = np.asarray(boxes, np.float64)
    u = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]])
    x, y = b[:, None, 3] * u[None, :, 0], b[:, None, 4] * u[None, :, 1]
    s, c = np.sin(b[:, 6])[:, None], np.cos(b[:, 6])[:, None]
    return np.stack([x * c - y * s + b[:, None, 0], x * s + y * c + b[:, None, 1]], -1)


def sat_overlap(a, b, tol=1e-6):
    """two convex quads (4, 2) float64 overlap with positive area (separating-axis test; touching is not overlap)"""
    for poly in (a, b):
        for k in range(4):
            e = poly[(k + 1) % 4] - poly[k]
            n = np.array([-e[1], e[0]]) / np.hypot(*e)
            pa, pb = a @ n, b @ n
            if pa.max() <= pb.min() + tol or pb.max() <= pa.min() + tol:
                return False
    return True


def local_coords(points, box):
    """points (n, 3) in the frame of box (float64): centre at the bottom face's middle, x along the box's dx"""
    b = np.asarray(box, np.float64)
    d = np.asarray(points, np.float64)[:, :3] - b[:3]
    s, c = np.sin(b[6]), np.cos(b[6])
    return np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], -1)


def face_distance(points, box):
    """signed distance to the nearest face (> 0 inside), float64"""
    q = local_coords(points, box)
    b = np.asarray(box, np.float64)
    return np.min(np.stack([b[3] / 2 - np.abs(q[:, 0]), b[4] / 2 - np.abs(q[:, 1]), q[:, 2], b[5] - q[:, 2]], -1), -1)


# ------------------------------------------------------------------------------------------------- synthetic database
def random_box(rng, dim, centre_range=40.0):
    b = np.zeros(dim, F32)
    b[0:2] = rng.uniform(-centre_range, centre_range, 2)
    b[2] = rng.uniform(-2.5, 0.0)
    b[3:6] = [rng.uniform(1.0, 6.0), rng.uniform(0.6, 2.5), rng.uniform(0.8, 3.0)]
    b[6] = rng.uniform(-np.pi, np.pi)
    if dim == 9:
        b[7:9] = rng.normal(0, 2, 2)
    return b


def object_points(rng, box, k, load_dim):
    """k points inside box, in the database's layout: relative to the box's bottom centre (mmdet3d subtracts the centre)"""
    q = rng.uniform(-0.45, 0.45, (k, 3)) * np.asarray(box[3:6], np.float64)
    q[:, 2] = (q[:, 2] / box[5] + 0.5) * box[5]
    s, c = np.sin(np.float64(box[6])), np.cos(np.float64(box[6]))
    p = np.zeros((k, load_dim), F32)
    p[:, 0] = q[:, 0] * c - q[:, 1] * s
    p[:, 1] = q[:, 0] * s + q[:, 1] * c
    p[:, 2] = q[:, 2]
    p[:, 3:] = rng.uniform(0, 100, (k, load_dim - 3))
    return p


def write_db(root, classes, per_class, dim, load_dim, seed=0, difficulties=(0, 0, 1, -1), pts=(3, 60)):
    """a GT database as create_data.py lays it out: root/gt_database/*.bin + root/dbinfos.pkl -> (info_path, data_root)"""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    infos = {}
    for name in classes:
        lst = []
        for j in range(per_class):
            box = random_box(rng, dim)
            k = int(rng.integers(pts[0], pts[1]))
            rel = os.path.join("gt_database", f"{j}_{name}.bin")
            object_points(rng, box, k, load_dim).tofile(os.path.join(root, rel))
            lst.append(dict(name=name, path=rel, image_idx=j, gt_idx=j, box3d_lidar=box, num_points_in_gt=k,
                            difficulty=int(difficulties[j % len(difficulties)]), group_id=j))
        infos[name] = lst
    info_path = os.path.join(root, "dbinfos.pkl")
    with open(info_path, "wb") as f:
        pickle.dump(infos, f)
    return info_path, root


class RefSampler:
    """DataBaseSampler's draws restated (independently of plugin/object_sample.py): construction shuffles, then sample_all"""

    def __init__(self, info_path, data_root, rate, prepare, sample_groups, classes, load_dim=4, use_dim=(0, 1, 2, 3)):
        with open(info_path, "rb") as f:
            db = pickle.load(f)
        for k, v in prepare.items():
            if k == "filter_by_difficulty":
                db = {n: [i for i in lst if i["difficulty"] not in v] for n, lst in db.items()}
            elif k == "filter_by_min_points":
                for n, mn in v.items():
                    if int(mn) > 0:
                        db[n] = [i for i in db[n] if i["num_points_in_gt"] >= int(mn)]
        self.db, self.rate, self.groups, self.classes = db, rate, list(sample_groups.items()), list(classes)
        self.data_root, self.load_dim = data_root, load_dim
        self.use_dim = list(range(use_dim)) if isinstance(use_dim, int) else list(use_dim)
        self.state = {}
        for n, lst in db.items():
            idx = np.arange(len(lst))
            np.random.shuffle(idx)
            self.state[n] = [idx, 0]

    def _take(self, name, num):
        idx, pos = self.state[name]
        if pos + num >= len(idx):
            out = idx[pos:].copy()
            np.random.shuffle(idx)
            self.state[name][1] = 0
        else:
            out = idx[pos:pos + num]
            self.state[name][1] = pos + num
        return [self.db[name][i] for i in out]

    def candidates(self, gt_labels):
        nums = [int(np.round(self.rate * int(mx - np.sum(gt_labels == self.classes.index(n))))) for n, mx in self.groups]
        return [(n, self._take(n, num) if num > 0 else []) for (n, _), num in zip(self.groups, nums)]

    def load(self, info):
        return np.fromfile(os.path.join(self.data_root, info["path"]), np.float32).reshape(-1, self.load_dim)[:, self.use_dim]


def np_object_sample(points, gt_boxes, gt_labels, sampler, bev_corners, box_planes):
    """ObjectSample end to end on the host: the draws (sampler), the greedy acceptance, the removal and the concatenation.
    bev_corners / box_planes are the host geometry helpers (the same float32 host code the transform uses)."""
    groups = sampler.candidates(gt_labels)
    cands = [(n, i) for n, lst in groups for i in lst]
    if not cands:
        return points, gt_boxes, gt_labels, None
    cand = np.stack([np.asarray(i["box3d_lidar"], F32) for _, i in cands])
    offsets = np.cumsum([0] + [len(lst) for _, lst in groups])
    acc = np.nonzero(np_accept(bev_corners(gt_boxes), bev_corners(cand), offsets))[0]
    if len(acc) == 0:
        return points, gt_boxes, gt_labels, acc
    keep = np_points_in_boxes(points, box_planes(cand[acc])) < 0
    sampled = []
    for a in acc:
        p = sampler.load(cands[a][1]).copy()
        p[:, :3] = p[:, :3] + cand[a, :3]
        sampled.append(p)
    pts = np.concatenate(sampled + [points[keep]])
    labels = np.array([sampler.classes.index(cands[a][1].get("name", cands[a][0])) for a in acc], np.int64)
    return pts, np.concatenate([gt_boxes, cand[acc]]), np.concatenate([gt_labels, labels]), acc
