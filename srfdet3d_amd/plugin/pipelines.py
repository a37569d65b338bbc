"""The step before the path: the reference's `test_pipeline` between decoded sensor data and
`SRFDet.forward`, on the device.

Reference: configs/nus/srfdet_voxel_nusc_LC.py:253-283 (the pipeline), mmdet3d_plugin/datasets/pipelines/transform_3d.py:7-93
(`PadMultiViewImage`, `NormalizeMultiviewImage`), mmdet3d 1.0.0rc6 for `PointsRangeFilter`, `LoadPointsFromMultiSweeps`,
`MultiScaleFlipAug3D`, `DefaultFormatBundle3D`, `Collect3D` (third party: their semantics are restated here, parity unpinned).

What is different from the reference and why: the transforms keep their registry names, constructor arguments and the
`results` keys they read / write, but `results['points']` is a GPU (N, nf) float32 tensor and `results['img']` a GPU
(V, H, W, 3) uint8 tensor (the decoded views, as `LoadMultiViewImageFromFiles` stacks them) instead of numpy on the host:
the sweep of a frame is 0.6 MB and its six views 26 MB as bytes (107 MB once they are float32), so they are uploaded raw
and everything after the decode runs as two HBM-bound kernels (`ops.points_filter`, `ops.image_prepare`).  File reading
and image decoding (`LoadPointsFromFile`, `LoadMultiViewImageFromFiles`) stay outside: they are host I/O.
`Compose` fuses an adjacent Normalize + Pad pair into the one `image_prepare` launch.

Train-time 3-D augmentation (mmdet3d 1.0.0rc6 `GlobalRotScaleTrans`, `RandomFlip3D`, `ObjectRangeFilter`,
`ObjectNameFilter`, `PointShuffle`): the random draws, sin / cos and arctan2 happen here on the host in float32, the point and
box arithmetic in `ops.points_augment` / `ops.boxes_augment`.  `results['gt_bboxes_3d']` is a `LiDARInstance3DBoxes` on the
device and `results['gt_labels_3d']` a device int64 tensor.  A run of adjacent GlobalRotScaleTrans -> RandomFlip3D ->
PointsRangeFilter -> ObjectRangeFilter -> ObjectNameFilter (any of them, in that order) becomes one points launch plus one
boxes launch in `Compose`; the draws still happen per transform in order, and the result is bit-identical to running them
one by one.

The numpy draw order is restated from memory of mmdet 2.28.2 / mmdet3d 1.0.0rc6 (third party, not pinned here):
  GlobalRotScaleTrans: np.random.uniform(*rot_range); np.random.uniform(*scale_ratio_range) unless 'pcd_scale_factor' is
    already set; np.random.normal(scale=translation_std (float32), size=3).
  RandomFlip3D: np.random.choice([direction, None], p=[flip_ratio, 1 - flip_ratio]) of mmdet's RandomFlip.__call__ unless
    'flip' is already set; then, with sync_2d=False, np.random.rand() < flip_ratio_bev_horizontal unless
    'pcd_horizontal_flip' is set, and np.random.rand() < flip_ratio_bev_vertical unless 'pcd_vertical_flip' is set.
A step with identity parameters (angle 0, scale 1, translation 0, no flip) is skipped, so the test pipelines of the
LiDAR-only configs launch nothing and hand `results['points']` on unchanged (the reference's product by the identity
matrix would turn -0.0 into +0.0 and an infinite coordinate into NaN; nothing else differs).
"""
import numpy as np
import torch

from .. import ops
from ..compat.boxes import LiDARInstance3DBoxes
from ..compat.registry import PIPELINES


def _points_tensor(p):
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise RuntimeError("srfdet3d_amd: pipeline transforms take GPU tensors (no CPU fallback exists)")
    return p


@PIPELINES.register_module()
class PointsRangeFilter:
    """results['points'] <- the points strictly inside point_cloud_range, order kept (mmdet3d `points.in_range_3d`)."""

    def __init__(self, point_cloud_range):
        self.pcd_range = [float(v) for v in point_cloud_range]

    def __call__(self, results):
        results["points"] = ops.points_filter(_points_tensor(results["points"]), self.pcd_range)
        return results

    def _plan(self, results, plan):
        plan.pc_range = self.pcd_range

    def __repr__(self):
        return f"{self.__class__.__name__}(point_cloud_range={self.pcd_range})"


class _AugPlan:
    """The device work of one or more of the fusable 3-D transforms: their steps in kernel order (`_FUSE_ORDER`), the
    parameters the host drew for them, and the filters.  `run` launches at most one points and one boxes kernel."""

    def __init__(self):
        self.pts_steps = 0
        self.box_steps = 0
        self.aug = [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0]  # sin, cos, yaw_add, scale, tx, ty, tz (float32 values)
        self.pc_range = None
        self.bev_range = None
        self.num_classes = 0
        self.no_class = False

    def run(self, results):
        pts = results.get("points")
        if pts is not None and (self.pts_steps or self.pc_range is not None):
            pts = _points_tensor(pts)
            if self.pts_steps:
                results["points"] = ops.points_augment(pts, self.pts_steps, self.aug, self.pc_range)
            else:  # a lone PointsRangeFilter: the kernel it always used
                results["points"] = ops.points_filter(pts, self.pc_range)
        boxes = results.get("gt_bboxes_3d")
        if boxes is not None and (self.box_steps or self.bev_range is not None or self.num_classes > 0 or self.no_class):
            t = _points_tensor(boxes.tensor)
            labels = results.get("gt_labels_3d")
            if labels is None:
                if self.bev_range is not None or self.num_classes > 0 or self.no_class:
                    raise KeyError("gt_labels_3d")
                labels = torch.zeros((t.shape[0],), dtype=torch.int64, device=t.device)
            b, lab = ops.boxes_augment(t, _points_tensor(labels), self.box_steps, self.aug, self.bev_range, self.num_classes)
            if self.no_class:
                b, lab = b[:0], lab[:0]
            results["gt_bboxes_3d"] = LiDARInstance3DBoxes(b, box_dim=boxes.box_dim, with_yaw=boxes.with_yaw)
            if "gt_labels_3d" in results:
                results["gt_labels_3d"] = lab
        return results


def _run_planned(transforms, results):
    plan = _AugPlan()
    for t in transforms:
        t._plan(results, plan)
    return plan.run(results)


@PIPELINES.register_module()
class GlobalRotScaleTrans:
    """Random rotation about z, uniform scaling and a Gaussian translation of the points and the GT boxes (mmdet3d
    `GlobalRotScaleTrans`).  Writes 'pcd_rotation' (3 x 3 float32 rot_mat_T), 'pcd_rotation_angle', 'pcd_scale_factor',
    'pcd_trans' and extends 'transformation_3d_flow' with R, S, T, as the reference does.  As in the reference, a frame whose
    GT box field is present but empty keeps its points unrotated (mmdet3d rotates the points through the boxes)."""

    def __init__(self, rot_range=(-0.78539816, 0.78539816), scale_ratio_range=(0.95, 1.05), translation_std=(0, 0, 0),
                 shift_height=False):
        if not isinstance(rot_range, (list, tuple, np.ndarray)):
            rot_range = [-rot_range, rot_range]
        if not isinstance(translation_std, (list, tuple, np.ndarray)):
            translation_std = [translation_std] * 3
        assert all(std >= 0 for std in translation_std), "translation_std should be positive"
        if shift_height:
            raise NotImplementedError("srfdet3d_amd: GlobalRotScaleTrans(shift_height=True) (no reference config uses it)")
        self.rot_range = list(rot_range)
        self.scale_ratio_range = list(scale_ratio_range)
        self.translation_std = list(translation_std)
        self.shift_height = shift_height

    def draw(self, results):
        """The host half: the numpy draws in the reference's order and the `results` keys they produce.  -> (angle,
        sin, cos, yaw_add) as float32 values and whether the points are rotated."""
        results.setdefault("transformation_3d_flow", [])
        angle = np.random.uniform(self.rot_range[0], self.rot_range[1])
        if "pcd_scale_factor" not in results:
            results["pcd_scale_factor"] = np.random.uniform(self.scale_ratio_range[0], self.scale_ratio_range[1])
        trans = np.random.normal(scale=np.array(self.translation_std, dtype=np.float32), size=3).T
        a32 = torch.tensor(angle, dtype=torch.float32)
        sin, cos = torch.sin(a32), torch.cos(a32)
        yaw_add = np.arctan2(np.float32(sin.item()), np.float32(cos.item()))  # LiDARInstance3DBoxes.rotate
        boxes = results.get("gt_bboxes_3d")
        rotate_points = boxes is None or len(boxes) != 0
        if rotate_points:
            results["pcd_rotation"] = torch.stack([torch.stack([cos, sin, torch.zeros(())]),
                                                   torch.stack([-sin, cos, torch.zeros(())]),
                                                   torch.tensor([0.0, 0.0, 1.0])])
        results["pcd_rotation_angle"] = angle
        results["pcd_trans"] = trans
        results["transformation_3d_flow"].extend(["R", "S", "T"])
        return np.float32(sin.item()), np.float32(cos.item()), np.float32(yaw_add), rotate_points

    def _plan(self, results, plan):
        sin, cos, yaw_add, rotate_points = self.draw(results)
        angle = results["pcd_rotation_angle"]
        scale = np.float32(results["pcd_scale_factor"])
        trans = np.asarray(results["pcd_trans"], dtype=np.float32)
        if angle != 0:
            plan.aug[0:3] = [float(sin), float(cos), float(yaw_add)]
            plan.box_steps |= ops.AUG_ROTATE
            if rotate_points:
                plan.pts_steps |= ops.AUG_ROTATE
        if scale != 1:
            plan.aug[3] = float(scale)
            plan.pts_steps |= ops.AUG_SCALE
            plan.box_steps |= ops.AUG_SCALE
        if np.any(trans != 0):
            plan.aug[4:7] = [float(v) for v in trans]
            plan.pts_steps |= ops.AUG_TRANSLATE
            plan.box_steps |= ops.AUG_TRANSLATE

    def __call__(self, results):
        return _run_planned([self], results)

    def __repr__(self):
        return (f"{self.__class__.__name__}(rot_range={self.rot_range}, scale_ratio_range={self.scale_ratio_range}, "
                f"translation_std={self.translation_std}, shift_height={self.shift_height})")


@PIPELINES.register_module()
class RandomFlip3D:
    """Random BEV flips of the points and the GT boxes (mmdet3d `RandomFlip3D` over mmdet's `RandomFlip`).  Writes 'flip',
    'flip_direction', 'pcd_horizontal_flip', 'pcd_vertical_flip' and extends 'transformation_3d_flow' with HF / VF.  Flipping
    2-D images is not implemented: a drawn 2-D flip with an image in `results` raises NotImplementedError (only kitti_LC's
    train pipeline could draw one)."""

    def __init__(self, sync_2d=True, flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0, direction="horizontal"):
        for r in (flip_ratio_bev_horizontal, flip_ratio_bev_vertical):
            assert r is None or (isinstance(r, (int, float)) and 0 <= r <= 1)
        assert direction in ("horizontal", "vertical", "diagonal")
        self.sync_2d = sync_2d
        self.flip_ratio = flip_ratio_bev_horizontal
        self.flip_ratio_bev_vertical = flip_ratio_bev_vertical
        self.direction = direction

    def draw(self, results):
        """The host half: the numpy draws in the reference's order and the `results` keys they produce."""
        if "flip" not in results:  # mmdet RandomFlip.__call__
            direction_list = [self.direction, None]
            single_ratio = self.flip_ratio / (len(direction_list) - 1)
            cur_dir = np.random.choice(direction_list, p=[single_ratio] * (len(direction_list) - 1) + [1 - self.flip_ratio])
            results["flip"] = cur_dir is not None
            results.setdefault("flip_direction", cur_dir)
        if results["flip"] and any(k in results for k in results.get("img_fields", ["img"])):
            raise NotImplementedError("srfdet3d_amd: RandomFlip3D does not flip 2-D images")
        if self.sync_2d:
            results["pcd_horizontal_flip"] = results["flip"]
            results["pcd_vertical_flip"] = False
        else:
            if "pcd_horizontal_flip" not in results:
                results["pcd_horizontal_flip"] = bool(np.random.rand() < self.flip_ratio)
            if "pcd_vertical_flip" not in results:
                results["pcd_vertical_flip"] = bool(np.random.rand() < self.flip_ratio_bev_vertical)
        results.setdefault("transformation_3d_flow", [])
        if results["pcd_horizontal_flip"]:
            results["transformation_3d_flow"].extend(["HF"])
        if results["pcd_vertical_flip"]:
            results["transformation_3d_flow"].extend(["VF"])

    def _plan(self, results, plan):
        self.draw(results)
        for key, bit in (("pcd_horizontal_flip", ops.AUG_FLIP_H), ("pcd_vertical_flip", ops.AUG_FLIP_V)):
            if results[key]:
                plan.pts_steps |= bit
                plan.box_steps |= bit

    def __call__(self, results):
        return _run_planned([self], results)

    def __repr__(self):
        return (f"{self.__class__.__name__}(sync_2d={self.sync_2d}, flip_ratio_bev_horizontal={self.flip_ratio}, "
                f"flip_ratio_bev_vertical={self.flip_ratio_bev_vertical})")


@PIPELINES.register_module()
class ObjectRangeFilter:
    """Keeps the GT boxes whose BEV centre lies strictly inside point_cloud_range, then limit_yaw(offset=0.5, period=2 pi)
    (mmdet3d `ObjectRangeFilter` on LiDAR boxes)."""

    def __init__(self, point_cloud_range):
        self.pcd_range = np.array(point_cloud_range, dtype=np.float32)

    def _plan(self, results, plan):
        plan.bev_range = [float(v) for v in self.pcd_range[[0, 1, 3, 4]]]

    def __call__(self, results):
        return _run_planned([self], results)

    def __repr__(self):
        return f"{self.__class__.__name__}(point_cloud_range={self.pcd_range.tolist()})"


@PIPELINES.register_module()
class ObjectNameFilter:
    """Keeps the GT boxes whose label is one of the classes, i.e. 0 <= label < len(classes) (mmdet3d `ObjectNameFilter`)."""

    def __init__(self, classes):
        self.classes = classes
        self.labels = list(range(len(self.classes)))

    def _plan(self, results, plan):
        plan.num_classes = len(self.labels)
        plan.no_class = not self.labels  # the kernel reads num_classes <= 0 as "no name filter"

    def __call__(self, results):
        return _run_planned([self], results)

    def __repr__(self):
        return f"{self.__class__.__name__}(classes={self.classes})"


@PIPELINES.register_module()
class PointShuffle:
    """results['points'] <- its rows in a random order: torch.randperm on the points' device and a gather, exactly the
    reference's `BasePoints.shuffle`."""

    def __call__(self, results):
        pts = _points_tensor(results["points"])
        idx = torch.randperm(pts.shape[0], device=pts.device)
        results["points"] = pts[idx]
        return results

    def __repr__(self):
        return self.__class__.__name__


# the transforms Compose may run as one plan, in the order of the kernels' steps
_FUSE_ORDER = (GlobalRotScaleTrans, RandomFlip3D, PointsRangeFilter, ObjectRangeFilter, ObjectNameFilter)


def _fuse_rank(t):
    for r, cls in enumerate(_FUSE_ORDER):
        if type(t) is cls:
            return r
    return None


@PIPELINES.register_module()
class LoadPointsFromMultiSweeps:
    """The in-memory half of mmdet3d's transform of the same name: results['sweeps'] is a list of dicts with the already
    loaded 'points' (GPU (n, >= 5) tensor: x, y, z, intensity, ring/time slot), 'sensor2lidar_rotation' (3x3),
    'sensor2lidar_translation' (3), 'timestamp' (us); results['timestamp'] the key frame's in SECONDS (the dataset divides
    it, nuscenes_dataset.py:44).  Every sweep is cleaned of the
    returns from the ego vehicle (`remove_close`, radius 1 m), moved into the key frame's LiDAR frame, stamped with its age
    in seconds in channel 4, and appended to the key frame's points (whose channel 4 is set to 0)."""

    def __init__(self, sweeps_num=10, load_dim=5, use_dim=(0, 1, 2, 4), pad_empty_sweeps=False, remove_close=False,
                 test_mode=False, file_client_args=None):
        self.sweeps_num = sweeps_num
        self.load_dim = load_dim
        self.use_dim = list(use_dim)
        self.pad_empty_sweeps = pad_empty_sweeps
        self.remove_close = remove_close
        self.test_mode = test_mode

    def __call__(self, results):
        points = _points_tensor(results["points"]).clone()
        points[:, 4] = 0
        out = [points]
        ts = results["timestamp"]
        sweeps = results.get("sweeps", [])
        if self.pad_empty_sweeps and len(sweeps) == 0:
            for _ in range(self.sweeps_num):
                out.append(ops.points_filter(points, None, 1.0) if self.remove_close else points)
        else:
            if len(sweeps) <= self.sweeps_num or self.test_mode:
                choices = range(min(len(sweeps), self.sweeps_num))
            else:
                choices = np.random.choice(len(sweeps), self.sweeps_num, replace=False)
            for i in choices:
                sw = sweeps[int(i)]
                p = _points_tensor(sw["points"])[:, :self.load_dim]
                p = ops.points_filter(p, None, 1.0) if self.remove_close else p.clone()
                rot = torch.as_tensor(np.asarray(sw["sensor2lidar_rotation"], np.float32), device=p.device)
                p[:, :3] = p[:, :3] @ rot.T
                p[:, :3] += torch.as_tensor(np.asarray(sw["sensor2lidar_translation"], np.float32), device=p.device)
                p[:, 4] = ts - sw["timestamp"] / 1e6
                out.append(p)
        results["points"] = torch.cat(out, 0)[:, self.use_dim].contiguous()
        return results


@PIPELINES.register_module()
class NormalizeMultiviewImage:
    """(x - mean) / std per channel in float32, after a BGR -> RGB swap when to_rgb (transform_3d.py:59-93).  On its own it
    turns the (V, H, W, 3) uint8 views into (V, 3, H, W) float32; followed by PadMultiViewImage, `Compose` runs both as one
    launch."""

    def __init__(self, mean, std, to_rgb=True):
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        self.to_rgb = to_rgb

    def _cfg(self, results):
        results["img_norm_cfg"] = dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)

    def __call__(self, results, pad=None):
        img = results["img"]
        V, H, W, _ = img.shape
        if pad is None:
            size = (H, W)
        elif pad.size is not None:
            size = tuple(pad.size)
        else:
            d = pad.size_divisor
            size = (-(-H // d) * d, -(-W // d) * d)
        results["img"] = ops.image_prepare(img, self.mean, self.std, self.to_rgb, size=size)
        self._cfg(results)
        if pad is not None:
            pad._keys(results, (H, W), size)
        return results

    def __repr__(self):
        return f"{self.__class__.__name__}(mean={self.mean}, std={self.std}, to_rgb={self.to_rgb})"


@PIPELINES.register_module()
class PadMultiViewImage:
    """Zero padding below / right of every view to a fixed size or to a multiple of size_divisor (transform_3d.py:7-56).
    Adds 'img_shape', 'pad_shape', 'pad_fixed_size', 'pad_size_divisor' like the reference (shapes as (H, W, 3) per view)."""

    def __init__(self, size=None, size_divisor=None, pad_val=0):
        assert size is not None or size_divisor is not None
        assert size is None or size_divisor is None
        if pad_val != 0:
            raise NotImplementedError("srfdet3d_amd: PadMultiViewImage pads with zeros (every reference config does)")
        self.size = size
        self.size_divisor = size_divisor
        self.pad_val = pad_val

    def _keys(self, results, hw, size):
        V = results["img"].shape[0]
        results.setdefault("ori_shape", [(hw[0], hw[1], 3)] * V)
        results["img_shape"] = [(size[0], size[1], 3)] * V
        results["pad_shape"] = [(size[0], size[1], 3)] * V
        results["pad_fixed_size"] = self.size
        results["pad_size_divisor"] = self.size_divisor

    def __call__(self, results):
        img = results["img"]  # (V, 3, H, W) float32, already normalised
        if img.dtype == torch.uint8:
            raise RuntimeError("srfdet3d_amd: PadMultiViewImage follows NormalizeMultiviewImage in every reference pipeline")
        H, W = img.shape[-2:]
        if self.size is not None:
            size = tuple(self.size)
        else:
            d = self.size_divisor
            size = (-(-H // d) * d, -(-W // d) * d)
        results["img"] = torch.nn.functional.pad(img, (0, size[1] - W, 0, size[0] - H))
        self._keys(results, (H, W), size)
        return results

    def __repr__(self):
        return f"{self.__class__.__name__}(size={self.size}, size_divisor={self.size_divisor}, pad_val={self.pad_val})"


@PIPELINES.register_module()
class DefaultFormatBundle3D:
    """The reference's bundle transposes every view HWC -> CHW, stacks them and wraps points / images as tensors.  Here the
    views already are one (V, 3, H, W) device tensor and the points a device tensor: nothing is left to do."""

    def __init__(self, class_names=None, with_gt=True, with_label=True):
        self.class_names = class_names

    def __call__(self, results):
        return results


@PIPELINES.register_module()
class Collect3D:
    """-> {'img_metas': dict of the meta keys present, key: results[key] for the requested keys}."""

    META_KEYS = ("filename", "ori_shape", "img_shape", "lidar2img", "depth2img", "cam2img", "pad_shape", "scale_factor", "flip",
                 "pcd_horizontal_flip", "pcd_vertical_flip", "box_mode_3d", "box_type_3d", "img_norm_cfg", "pcd_trans",
                 "sample_idx", "pcd_scale_factor", "pcd_rotation", "pcd_rotation_angle", "pts_filename", "transformation_3d_flow",
                 "trans_mat", "affine_aug")

    def __init__(self, keys, meta_keys=None):
        self.keys = list(keys)
        self.meta_keys = tuple(meta_keys) if meta_keys is not None else self.META_KEYS

    def __call__(self, results):
        data = {"img_metas": {k: results[k] for k in self.meta_keys if k in results}}
        for k in self.keys:
            data[k] = results[k]
        return data


@PIPELINES.register_module()
class MultiScaleFlipAug3D:
    """Test-time wrapper.  Every reference config uses one scale, pts_scale_ratio = 1 and flip = False, i.e. exactly one
    pass of the inner transforms whose outputs are wrapped in one-element lists; anything else is refused."""

    def __init__(self, transforms, img_scale=None, pts_scale_ratio=1, flip=False, flip_direction="horizontal",
                 pcd_horizontal_flip=False, pcd_vertical_flip=False):
        ratios = pts_scale_ratio if isinstance(pts_scale_ratio, (list, tuple)) else [pts_scale_ratio]
        if flip or pcd_horizontal_flip or pcd_vertical_flip or list(ratios) != [1]:
            raise NotImplementedError("srfdet3d_amd: test-time augmentation beyond the reference configs' single pass")
        self.transforms = Compose(transforms)
        self.img_scale = img_scale

    def __call__(self, results):
        results = dict(results)
        results.update(scale=self.img_scale, flip=False, pcd_scale_factor=1, pcd_horizontal_flip=False, pcd_vertical_flip=False)
        data = self.transforms(results)
        return {k: [v] for k, v in data.items()}


class Compose:
    """Builds the transforms of a config list through the PIPELINES registry and runs them in order; a
    NormalizeMultiviewImage directly followed by a PadMultiViewImage becomes one `image_prepare` launch, and a run of two or
    more adjacent 3-D transforms in `_FUSE_ORDER` (e.g. GlobalRotScaleTrans, RandomFlip3D, PointsRangeFilter,
    ObjectRangeFilter, ObjectNameFilter) one points launch plus one boxes launch, bit-identical to running them one by one."""

    def __init__(self, transforms):
        self.transforms = [PIPELINES.build(dict(t)) if isinstance(t, dict) else t for t in transforms]

    def _fusable_run(self, i):
        j = i
        while j < len(self.transforms):
            r = _fuse_rank(self.transforms[j])
            if r is None or (j > i and r <= _fuse_rank(self.transforms[j - 1])):
                break
            j += 1
        return j

    def __call__(self, results):
        i = 0
        while i < len(self.transforms):
            t = self.transforms[i]
            nxt = self.transforms[i + 1] if i + 1 < len(self.transforms) else None
            j = self._fusable_run(i)
            if j - i >= 2:
                results = _run_planned(self.transforms[i:j], results)
                i = j
            elif isinstance(t, NormalizeMultiviewImage) and isinstance(nxt, PadMultiViewImage):
                results = t(results, pad=nxt)
                i += 2
            else:
                results = t(results)
                i += 1
            if results is None:
                return None
        return results


class FrameFeeder:
    """Host -> device staging of one frame's raw inputs (points float32, views uint8), double buffered: `put` of frame
    i+1 is issued before the compute of frame i is waited for; `get` makes the current stream wait for the copy (an
    event, no host sync) and hands out the device tensors.

    pinned=False (default): plain copies from pageable memory (the runtime stages them through its own bounce buffers).
    pinned=True: pinned staging buffers + non-blocking copies on a separate copy stream -- the textbook overlap, but on the
    MI355X boxes of this project every third copy out of a `pin_memory()` buffer stalled the device for 70-90 ms (blocking
    or not, with or without the copy stream, SDMA on or off; pageable copies never did), so it is opt-in."""

    def __init__(self, max_points, nf, views, height, width, device="cuda:0", depth=2, pinned=False):
        self.dev = torch.device(device)
        self.pinned = pinned
        self.stream = torch.cuda.Stream(self.dev) if pinned else None
        self.slots = []
        for _ in range(depth):
            s = dict(d_pts=torch.empty((max_points, nf), dtype=torch.float32, device=self.dev),
                     d_img=torch.empty((views, height, width, 3), dtype=torch.uint8, device=self.dev),
                     n=0, ready=torch.cuda.Event(), free=torch.cuda.Event())
            if pinned:
                s["h_pts"] = torch.empty((max_points, nf), dtype=torch.float32).pin_memory()
                s["h_img"] = torch.empty((views, height, width, 3), dtype=torch.uint8).pin_memory()
            self.slots.append(s)
        self._put = 0
        self._get = 0

    def put(self, points, images=None):
        s = self.slots[self._put % len(self.slots)]
        self._put += 1
        n = int(points.shape[0])
        s["n"] = n
        if not self.pinned:
            cur = torch.cuda.current_stream(self.dev)
            cur.wait_event(s["free"])  # the kernels that read this slot last are ahead of the copy on the device
            s["d_pts"][:n].copy_(torch.as_tensor(points))
            if images is not None:
                s["d_img"].copy_(torch.as_tensor(images))
            s["ready"].record(cur)
            return
        s["free"].synchronize()  # the compute that read this slot last has finished (no-op the first time round)
        s["h_pts"][:n].copy_(torch.as_tensor(points))
        if images is not None:
            s["h_img"].copy_(torch.as_tensor(images))
        with torch.cuda.stream(self.stream):
            s["d_pts"][:n].copy_(s["h_pts"][:n], non_blocking=True)
            if images is not None:
                s["d_img"].copy_(s["h_img"], non_blocking=True)
            s["ready"].record(self.stream)

    def get(self):
        s = self.slots[self._get % len(self.slots)]
        self._get += 1
        torch.cuda.current_stream(self.dev).wait_event(s["ready"])
        return s["d_pts"][:s["n"]], s["d_img"], s

    @staticmethod
    def release(slot):
        """call once the frame's kernels that read the slot are enqueued"""
        slot["free"].record(torch.cuda.current_stream())
