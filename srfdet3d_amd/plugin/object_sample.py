"""GT-database sampling (`ObjectSample` over `DataBaseSampler`) and per-object noise (`ObjectNoise`) of the LiDAR-only train
pipelines (configs/nus/srfdet_voxel_nusc_L.py, configs/kitti/srfdet_voxel_kitti_L.py), on the device.

Reference: mmdet3d 1.0.0rc6 `ObjectSample`, `ObjectNoise` (datasets/pipelines/transforms_3d.py), `DataBaseSampler`,
`BatchSampler` (datasets/pipelines/dbsampler.py), `box_np_ops.points_in_rbbox` / `center_to_corner_box2d` /
`center_to_corner_box3d` / `corner_to_surfaces_3d` / `surface_equ_3d`, `data_augment_utils.box_collision_test` /
`noise_per_object_v3_` / `noise_per_box` / `points_transform_` / `box3d_transform_`.  Third party, restated here from the
published source: parity unpinned (neither mmdet3d nor numba is available to compare against).

Split of the work: every random draw stays on the host in numpy, in the reference's order; so does the O(boxes) geometry
(numpy float32, box_np_ops's order: sin / cos of each yaw, BEV corners, the six surface planes of each box), after one small
read-back of the boxes.  The point- and pair-level work runs in `csrc/objsample.hip`: points in boxes, BEV collisions, the
greedy acceptance, the removal and concatenation, the point and box transforms.  Read-backs: ObjectSample two (GT boxes with
their labels; the accept flags with the count of kept points), ObjectNoise one (the boxes).  The pipeline is never captured.

Yaw convention: the one `GlobalRotScaleTrans` implies (csrc/augment.hip `aug_rotate` turns points counter-clockwise by the
angle and adds the angle to the yaw), i.e. a box's corners are its local corners turned counter-clockwise by its yaw, as
mmdet3d 1.0's `LiDARInstance3DBoxes.corners`: x' = x cos - y sin, y' = x sin + y cos.  LiDAR boxes are bottom-centred
(origin (0.5, 0.5, 0)): a box spans [z, z + dz].

numpy draw order (restated, unpinned):
  ObjectSample: for each class of `sample_groups` in config order with n = round(rate * (max - #GT of that label)) > 0, that
    class's BatchSampler.sample(n): np.random.shuffle of its index array when it runs out (indices[idx:idx + n]; when
    idx + n >= len it returns the remainder only and reshuffles).  Each BatchSampler shuffles once at construction, in the
    pickle's class order.  The draws do not depend on acceptance, so all candidates are drawn before the one device pass.
  ObjectNoise: np.random.normal(scale=float32(translation_std), size=[n, num_try, 3]);
    np.random.uniform(*rot_range, size=[n, num_try]); the global-rotation uniform, size [n, num_try], drawn (and unused) even
    when global rotation is off -- also when there are no boxes (then all three have size 0).

dtype flow (mmdet3d keeps the boxes and points float32 and draws float64 noise; promotions assumed from the published
source): corners / planes float32; the try corners are float32(float64(corner) + (float64(centre) + loc)) with the float32
sin / cos of the float64 angle; points float32(float64(rotate(p - centre) + centre) + loc); boxes xyz float32(float64(xyz) +
loc), yaw float32(float64(yaw) + angle).  The database's `box3d_lidar` rows are read as float32 (what mmdet3d's
create_data.py writes; a float64 database would have promoted the sampler's collision test to float64 in mmdet3d).

Differences from the reference, each deliberate:
  - a point whose plane test gives NaN counts as outside (numba's `sign >= 0` loop counts it inside);
  - the labels of sampled objects come from `info['name']` when present (mmdet3d), else from the class key they were
    sampled under; a class whose filtered database is empty yields no candidates (mmdet3d raises in np.stack);
  - `results['points']`, `gt_bboxes_3d` and `gt_labels_3d` are new device tensors (mmdet3d's ObjectNoise writes its numpy
    views of the tensors in place);
  - `box_collision_test`'s containment branch is taken whenever no edges cross (the published loop guards it with
    `ret[i, j] is False`, whose meaning under numba depends on its version).
"""
import os
import pickle

import numpy as np
import torch

from .. import ops
from ..compat.boxes import LiDARInstance3DBoxes
from ..compat.registry import OBJECTSAMPLERS, PIPELINES

F32 = np.float32

# corners_nd's unit corners: 2-D clockwise from the minimum; 3-D in box_np_ops' order, then minus the origin
_NORM2 = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], F32) - F32(0.5)
_NORM3 = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], F32) - \
    np.array([0.5, 0.5, 0.0], F32)
# corner_to_surfaces_3d
_SURFACES = np.array([[0, 1, 2, 3], [7, 6, 5, 4], [0, 3, 7, 4], [1, 5, 6, 2], [0, 4, 5, 1], [3, 2, 6, 7]])


def _device_tensor(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"srfdet3d_amd: `{name}` must be a GPU tensor (no CPU fallback exists)")
    return t


def bev_corners(boxes):
    """(n, >= 7) float32 boxes -> (n, 4, 2) float32 BEV corners (center_to_corner_box2d of x, y, dx, dy, yaw; also
    box2d_to_corner_jit): dims * unit corner, turned counter-clockwise by the yaw (products rounded one by one), + centre."""
    b = np.asarray(boxes, F32)
    s, c = np.sin(b[:, 6])[:, None], np.cos(b[:, 6])[:, None]
    x = b[:, 3:4] * _NORM2[None, :, 0]
    y = b[:, 4:5] * _NORM2[None, :, 1]
    out = np.empty((len(b), 4, 2), F32)
    out[:, :, 0] = (x * c + y * (-s)) + b[:, 0:1]
    out[:, :, 1] = (x * s + y * c) + b[:, 1:2]
    return out


def box_corners3d(boxes):
    """(n, >= 7) float32 boxes -> (n, 8, 3) corners (center_to_corner_box3d, origin (0.5, 0.5, 0), axis 2)."""
    b = np.asarray(boxes, F32)
    s, c = np.sin(b[:, 6])[:, None], np.cos(b[:, 6])[:, None]
    z0, one = F32(0), F32(1)
    x = b[:, 3:4] * _NORM3[None, :, 0]
    y = b[:, 4:5] * _NORM3[None, :, 1]
    z = b[:, 5:6] * _NORM3[None, :, 2]
    out = np.empty((len(b), 8, 3), F32)
    out[:, :, 0] = ((x * c + y * (-s)) + z * z0) + b[:, 0:1]
    out[:, :, 1] = ((x * s + y * c) + z * z0) + b[:, 1:2]
    out[:, :, 2] = ((x * z0 + y * z0) + z * one) + b[:, 2:3]
    return out


def box_planes(boxes):
    """(n, >= 7) float32 boxes -> (n, 6, 4) float32 [a, b, c, d] of the six faces, outward (surface_equ_3d of
    corner_to_surfaces_3d): v0 = p0 - p1, v1 = p1 - p2, normal = v0 x v1, d = -((a x0 + b y0) + c z0)."""
    surf = box_corners3d(boxes)[:, _SURFACES]  # (n, 6, 4, 3)
    p0, p1, p2 = surf[:, :, 0], surf[:, :, 1], surf[:, :, 2]
    v0, v1 = p0 - p1, p1 - p2
    out = np.empty(surf.shape[:2] + (4,), F32)
    out[..., 0] = v0[..., 1] * v1[..., 2] - v0[..., 2] * v1[..., 1]
    out[..., 1] = v0[..., 2] * v1[..., 0] - v0[..., 0] * v1[..., 2]
    out[..., 2] = v0[..., 0] * v1[..., 1] - v0[..., 1] * v1[..., 0]
    out[..., 3] = -((out[..., 0] * p0[..., 0] + out[..., 1] * p0[..., 1]) + out[..., 2] * p0[..., 2])
    return out


class BatchSampler:
    """mmdet3d `BatchSampler`: a shuffled index array handed out in slices; when a request reaches the end it gets only the
    remainder and the array is reshuffled (the reference's quirk, kept)."""

    def __init__(self, sampled_list, name=None, epoch=None, shuffle=True, drop_reminder=False):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0
        self._example_num = len(sampled_list)
        self._name = name
        self._shuffle = shuffle

    def _sample(self, num):
        if self._idx + num >= self._example_num:
            ret = self._indices[self._idx:].copy()
            self._reset()
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def _reset(self):
        if self._shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0

    def sample(self, num):
        return [self._sampled_list[i] for i in self._sample(num)]


def _check_disk(file_client_args, who):
    backend = (file_client_args or {}).get("backend", "disk")
    if backend != "disk":
        raise NotImplementedError(f"srfdet3d_amd: {who}: file backend {backend!r} (only 'disk' is implemented)")


class _ObjectPointsLoader:
    """The sampler's `points_loader` (mmdet3d LoadPointsFromFile): np.fromfile(float32).reshape(-1, load_dim)[:, use_dim]."""

    def __init__(self, type="LoadPointsFromFile", coord_type="LIDAR", load_dim=6, use_dim=(0, 1, 2), shift_height=False,
                 use_color=False, file_client_args=None):
        if type != "LoadPointsFromFile":
            raise NotImplementedError(f"srfdet3d_amd: DataBaseSampler points_loader {type!r}")
        if shift_height or use_color:
            raise NotImplementedError("srfdet3d_amd: DataBaseSampler points_loader with shift_height / use_color")
        _check_disk(file_client_args, "DataBaseSampler points_loader")
        self.load_dim = int(load_dim)
        self.use_dim = list(range(use_dim)) if isinstance(use_dim, int) else list(use_dim)
        assert max(self.use_dim) < self.load_dim, f"Expect all used dimensions < {self.load_dim}, got {self.use_dim}"

    def __call__(self, path):
        return np.fromfile(path, dtype=np.float32).reshape(-1, self.load_dim)[:, self.use_dim]


@OBJECTSAMPLERS.register_module()
class DataBaseSampler:
    """mmdet3d `DataBaseSampler` over a GT database written by mmdet3d's create_data.py: `info_path` is a pickle of
    {class name: [info dict with 'path', 'box3d_lidar', 'num_points_in_gt', 'difficulty', ('name')]}, `data_root` the
    directory the infos' paths are relative to.  `prepare` filters run in dict order; one BatchSampler per class of the
    filtered database, in the pickle's order; `sample_groups` keeps the config's order."""

    def __init__(self, info_path, data_root, rate, prepare, sample_groups, classes=None,
                 points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=4, use_dim=[0, 1, 2, 3]),
                 file_client_args=dict(backend="disk")):
        _check_disk(file_client_args, "DataBaseSampler")
        self.data_root = data_root
        self.info_path = info_path
        self.rate = rate
        self.prepare = prepare
        self.classes = classes
        self.cat2label = {name: i for i, name in enumerate(classes)}
        self.label2cat = {i: name for i, name in enumerate(classes)}
        self.points_loader = _ObjectPointsLoader(**dict(points_loader))
        with open(info_path, "rb") as f:
            db_infos = pickle.load(f)
        for prep_func, val in prepare.items():
            db_infos = getattr(self, prep_func)(db_infos, val)
        self.db_infos = db_infos
        self.sample_groups = [{name: int(num)} for name, num in sample_groups.items()]
        self.sample_classes = [name for g in self.sample_groups for name in g]
        self.sample_max_nums = [num for g in self.sample_groups for num in g.values()]
        self.sampler_dict = {k: BatchSampler(v, k, shuffle=True) for k, v in self.db_infos.items()}

    @staticmethod
    def filter_by_difficulty(db_infos, removed_difficulty):
        return {key: [info for info in dinfos if info["difficulty"] not in removed_difficulty] for key, dinfos in db_infos.items()}

    @staticmethod
    def filter_by_min_points(db_infos, min_gt_points_dict):
        for name, min_num in min_gt_points_dict.items():
            min_num = int(min_num)
            if min_num > 0:
                db_infos[name] = [info for info in db_infos[name] if info["num_points_in_gt"] >= min_num]
        return db_infos

    def sample_candidates(self, gt_labels):
        """The draws of sample_all: -> [(class name, [info, ...])] in sample_groups order, every candidate before any
        collision test (the draws never depend on which candidates are accepted)."""
        gt_labels = np.asarray(gt_labels)
        nums = []
        for class_name, max_sample_num in zip(self.sample_classes, self.sample_max_nums):
            label = self.cat2label[class_name]
            sampled_num = int(max_sample_num - np.sum([n == label for n in gt_labels]))
            nums.append(np.round(self.rate * sampled_num).astype(np.int64))
        return [(name, self.sampler_dict[name].sample(int(num)) if num > 0 else []) for name, num in zip(self.sample_classes, nums)]

    def load_points(self, info):
        path = os.path.join(self.data_root, info["path"]) if self.data_root else info["path"]
        return self.points_loader(path)


@PIPELINES.register_module()
class ObjectSample:
    """mmdet3d `ObjectSample`: pastes objects from the GT database into the frame.  Candidates are drawn per class, then
    accepted greedily on the device when their BEV box collides with no GT box, no accepted box and no not-rejected
    candidate of their own class; the original points inside accepted boxes are removed and the accepted objects' points
    (translated to their box) go first: points = cat([sampled, kept]).  Boxes and labels are appended.  When nothing is
    accepted `results` is returned unchanged."""

    def __init__(self, db_sampler, sample_2d=False, use_ground_plane=False):
        if sample_2d:
            raise NotImplementedError("srfdet3d_amd: ObjectSample(sample_2d=True) (no reference config uses it)")
        if use_ground_plane:
            raise NotImplementedError("srfdet3d_amd: ObjectSample(use_ground_plane=True) (no reference config uses it)")
        self.sample_2d = sample_2d
        self.use_ground_plane = use_ground_plane
        cfg = dict(db_sampler)
        cfg.setdefault("type", "DataBaseSampler")
        self.db_sampler = OBJECTSAMPLERS.build(cfg)

    def __call__(self, results):
        boxes = results["gt_bboxes_3d"]
        labels = _device_tensor(results["gt_labels_3d"], "gt_labels_3d")
        points = _device_tensor(results["points"], "points")
        t = _device_tensor(boxes.tensor, "gt_bboxes_3d").contiguous()
        n_gt, dim = t.shape
        nf = points.shape[1]
        if len(self.db_sampler.points_loader.use_dim) != nf:
            raise ValueError(f"srfdet3d_amd: ObjectSample: the database loader's use_dim has "
                             f"{len(self.db_sampler.points_loader.use_dim)} features, the points {nf}")
        dev = points.device
        # read-back 1: the GT boxes and their labels in one transfer
        if n_gt:
            host = torch.cat([t.reshape(-1).view(torch.int32), labels.contiguous().view(torch.int32)]).cpu().numpy()
            gt = host[:n_gt * dim].view(F32).reshape(n_gt, dim)
            gt_labels = host[n_gt * dim:].view(np.int64)
        else:
            gt, gt_labels = np.zeros((0, dim), F32), np.zeros((0,), np.int64)
        groups = self.db_sampler.sample_candidates(gt_labels)
        cands = [(name, info) for name, infos in groups for info in infos]
        if not cands:
            return results
        cand = np.stack([np.asarray(info["box3d_lidar"], F32) for _, info in cands])
        if cand.shape[1] != dim:
            raise ValueError(f"srfdet3d_amd: ObjectSample: database boxes have {cand.shape[1]} columns, gt_bboxes_3d {dim}")
        cand_labels = np.array([self.db_sampler.cat2label[info.get("name", name)] for name, info in cands], np.int64)
        offsets = np.cumsum([0] + [len(infos) for _, infos in groups]).astype(np.int32)
        nc = len(cands)
        # one upload: GT corners, candidate corners, candidate planes, class offsets
        host = np.concatenate([bev_corners(gt).ravel(), bev_corners(cand).ravel(), box_planes(cand).ravel(), offsets.view(F32)])
        buf = torch.from_numpy(host).to(dev)
        a, b, c = 8 * n_gt, 8 * (n_gt + nc), 8 * (n_gt + nc) + 24 * nc
        flags = torch.empty((nc + 1,), dtype=torch.int32, device=dev)
        ops.box_collision_accept(buf[:a].view(n_gt, 4, 2), buf[a:b].view(nc, 4, 2), buf[c:].view(torch.int32), out=flags[:nc])
        point_box = ops.points_in_boxes(points, buf[b:c].view(nc, 6, 4), box_mask=flags[:nc], num_outside=flags[nc:])
        # read-back 2: the accept flags and the number of original points that stay
        back = flags.cpu().numpy()
        accepted = np.nonzero(back[:nc])[0]
        if len(accepted) == 0:
            return results
        objs = [self.db_sampler.load_points(cands[i][1]) for i in accepted]
        s_off = np.cumsum([0] + [len(o) for o in objs]).astype(np.int32)
        sampled = np.ascontiguousarray(np.concatenate(objs), dtype=F32)
        s = len(sampled)
        host = np.concatenate([sampled.ravel(), cand[accepted, :3].ravel(), s_off.view(F32)])
        buf = torch.from_numpy(host).to(dev)
        a, b = s * nf, s * nf + 3 * len(accepted)
        results["points"] = ops.object_sample_merge(points, point_box, buf[:a].view(s, nf), buf[b:].view(torch.int32),
                                                    buf[a:b].view(-1, 3), s + int(back[nc]))
        new_boxes = torch.cat([t, torch.from_numpy(cand[accepted]).to(dev)])
        results["gt_bboxes_3d"] = LiDARInstance3DBoxes(new_boxes, box_dim=dim, with_yaw=boxes.with_yaw)
        results["gt_labels_3d"] = torch.cat([labels, torch.from_numpy(cand_labels[accepted]).to(dev)])
        return results

    def __repr__(self):
        return f"{self.__class__.__name__}(sample_2d={self.sample_2d}, db_sampler={type(self.db_sampler).__name__})"


@PIPELINES.register_module()
class ObjectNoise:
    """mmdet3d `ObjectNoise` (noise_per_object_v3_ with global rotation off): every GT box tries num_try random (rotation
    about its centre, translation) moves in index order and takes the first whose BEV box collides with no other box as it
    stands by then; the points inside each original box (the first box by index) move with it.  A box with no successful
    try stays where it is (its points go through the identity move, as in the reference)."""

    def __init__(self, translation_std=(0.25, 0.25, 0.25), global_rot_range=(0.0, 0.0), rot_range=(-0.15707963267, 0.15707963267),
                 num_try=100):
        if not isinstance(global_rot_range, (list, tuple, np.ndarray)):
            global_rot_range = [-global_rot_range, global_rot_range]
        if np.abs(global_rot_range[0] - global_rot_range[1]) >= 1e-3:
            raise NotImplementedError("srfdet3d_amd: ObjectNoise with a global rotation range (noise_per_box_v2_)")
        if not isinstance(rot_range, (list, tuple, np.ndarray)):
            rot_range = [-rot_range, rot_range]
        if not isinstance(translation_std, (list, tuple, np.ndarray)):
            translation_std = [translation_std] * 3
        self.translation_std = list(translation_std)
        self.global_rot_range = list(global_rot_range)
        self.rot_range = list(rot_range)
        self.num_try = int(num_try)

    def draw(self, n):
        """The numpy draws of noise_per_object_v3_ for n boxes -> (loc (n, num_try, 3) float64, rot (n, num_try) float64)."""
        loc = np.random.normal(scale=np.array(self.translation_std, dtype=F32), size=[n, self.num_try, 3])
        rot = np.random.uniform(self.rot_range[0], self.rot_range[1], size=[n, self.num_try])
        # global_rot_noises: uniform(global_rot_range - arctan2(x, y)) per box; its count does not depend on the boxes
        np.random.uniform(self.global_rot_range[0], self.global_rot_range[1], size=[n, self.num_try])
        return loc, rot

    def __call__(self, results):
        boxes = results["gt_bboxes_3d"]
        points = _device_tensor(results["points"], "points")
        t = _device_tensor(boxes.tensor, "gt_bboxes_3d").contiguous()
        n, dim = t.shape
        loc, rot = self.draw(n)
        if n == 0:
            return results
        b = t.cpu().numpy()  # the one read-back
        rot_sc = np.stack([np.sin(rot).astype(F32), np.cos(rot).astype(F32)], -1)
        dev = points.device
        geo = torch.from_numpy(np.concatenate([bev_corners(b).ravel(), box_planes(b).ravel(), rot_sc.ravel()])).to(dev)
        dbl = torch.from_numpy(np.concatenate([rot.ravel(), loc.ravel()])).to(dev)
        a, c = 8 * n, 32 * n
        T = self.num_try
        out_p, out_b, _ = ops.object_noise(points, t, geo[:a].view(n, 4, 2), geo[a:c].view(n, 6, 4), geo[c:].view(n, T, 2),
                                           dbl[:n * T].view(n, T), dbl[n * T:].view(n, T, 3))
        results["points"] = out_p
        results["gt_bboxes_3d"] = LiDARInstance3DBoxes(out_b, box_dim=dim, with_yaw=boxes.with_yaw)
        return results

    def __repr__(self):
        return (f"{self.__class__.__name__}(num_try={self.num_try}, translation_std={self.translation_std}, "
                f"global_rot_range={self.global_rot_range}, rot_range={self.rot_range})")
