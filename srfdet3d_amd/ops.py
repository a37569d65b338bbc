"""Functional layer over the C ABI: torch device tensors in, torch device tensors out.

torch is used here only to own device memory and to name the current HIP stream; every computation is a
kernel of libsrfdet3d_hip.so.  All functions raise on CPU tensors (there is no CPU fallback).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import FeatMap, check, hf, hi


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream.  torch.cuda.current_stream() costs ~9 us of Python per call (35 calls per
    frame); the raw accessor the graph-capture machinery itself uses is ~30x cheaper."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"srfdet3d_amd: `{name}` must be a GPU tensor (no CPU fallback exists)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"srfdet3d_amd: `{name}` must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _opt(t, name):
    return None if t is None else _ptr(_dev(t, name, torch.float32))


def _empty(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def grid_size(voxel_size, pc_range):
    """mmcv Voxelization.__init__: round((range[3:] - range[:3]) / voxel_size) in float32 -> (gx, gy, gz)."""
    r = np.asarray(pc_range, np.float32)
    v = np.asarray(voxel_size, np.float32)
    return [int(x) for x in np.round((r[3:] - r[:3]) / v)]


# ---------------------------------------------------------------------------------------------- voxelization
def dynamic_voxelize(points, voxel_size, pc_range):
    points = _dev(points, "points", torch.float32)
    n, nf = points.shape
    coors = _empty((n, 3), torch.int32, points.device)
    check(_lib.lib().srf_dynamic_voxelize(_ptr(points), n, nf, hf(voxel_size), hf(pc_range),
                                          hi(grid_size(voxel_size, pc_range)), _ptr(coors), _stream()),
          "dynamic_voxelize")
    return coors


def points_filter(points, pc_range=None, close_radius=0.0, static=False, with_index=False):
    """PointsRangeFilter (strict inequalities on x, y, z against pc_range) and / or the multi-sweep `remove_close`
    (|x| < r and |y| < r dropped) as one order-preserving compaction -> kept points (M, nf) [, their source rows].
    One D2H sync for M; static=True returns all n rows (rows >= M undefined) and the device scalar M instead."""
    points = _dev(points, "points", torch.float32)
    n, nf = points.shape
    L = _lib.lib()
    dev = points.device
    out = _empty((max(n, 1), nf), torch.float32, dev)
    index = _empty((max(n, 1),), torch.int32, dev) if with_index else None
    num = _empty((1,), torch.int32, dev)
    ws = _empty((max(L.srf_points_filter_workspace_bytes(n), 4),), torch.uint8, dev)
    check(L.srf_points_filter(_ptr(points), n, nf, hf(pc_range) if pc_range is not None else None, float(close_radius),
                              _ptr(out), _ptr(index), _ptr(num), _ptr(ws), _stream()), "points_filter")
    if static:
        return (out[:n], index[:n], num) if with_index else (out[:n], num)
    M = int(num.item())
    return (out[:M], index[:M]) if with_index else out[:M]


# srf_points_augment / srf_boxes_augment step bits (include/srfdet3d.h f-5), applied in this order
AUG_ROTATE, AUG_SCALE, AUG_TRANSLATE, AUG_FLIP_H, AUG_FLIP_V = 1, 2, 4, 8, 16


def points_augment(points, steps, aug=None, pc_range=None, with_index=False):
    """GlobalRotScaleTrans / RandomFlip3D steps on channels 0-2 (`steps`: AUG_* bits; a clear bit skips the step) and, with
    pc_range, the PointsRangeFilter test, as one order-preserving compaction -> kept points (M, nf) [, their source rows].
    aug = (sin, cos, yaw_add, scale, tx, ty, tz), float32 values computed on the host.  One D2H sync for M."""
    points = _dev(points, "points", torch.float32)
    n, nf = points.shape
    L = _lib.lib()
    dev = points.device
    out = _empty((max(n, 1), nf), torch.float32, dev)
    index = _empty((max(n, 1),), torch.int32, dev) if with_index else None
    num = _empty((1,), torch.int32, dev)
    ws = _empty((max(L.srf_points_augment_workspace_bytes(n), 4),), torch.uint8, dev)
    check(L.srf_points_augment(_ptr(points), n, nf, int(steps), hf(aug) if aug is not None else None,
                               hf(pc_range) if pc_range is not None else None, _ptr(out), _ptr(index), _ptr(num), _ptr(ws),
                               _stream()), "points_augment")
    M = int(num.item())
    return (out[:M], index[:M]) if with_index else out[:M]


def boxes_augment(boxes, labels, steps, aug=None, bev_range=None, num_classes=0, with_index=False):
    """The box half of `points_augment` on (n, 7 | 9) LiDAR boxes and their int64 labels, then ObjectRangeFilter (bev_range =
    (xmin, ymin, xmax, ymax), followed by limit_yaw) and ObjectNameFilter (num_classes > 0: 0 <= label < num_classes), one
    order-preserving compaction of boxes and labels -> (boxes (M, box_dim), labels (M,) [, source rows]).  One D2H sync."""
    boxes = _dev(boxes, "boxes", torch.float32)
    labels = _dev(labels, "labels", torch.int64)
    n, box_dim = boxes.shape
    if labels.shape != (n,):
        raise RuntimeError(f"srfdet3d_amd: `labels` must have shape ({n},), got {tuple(labels.shape)}")
    L = _lib.lib()
    dev = boxes.device
    out = _empty((max(n, 1), box_dim), torch.float32, dev)
    out_labels = _empty((max(n, 1),), torch.int64, dev)
    index = _empty((max(n, 1),), torch.int32, dev) if with_index else None
    num = _empty((1,), torch.int32, dev)
    ws = _empty((max(L.srf_boxes_augment_workspace_bytes(n), 4),), torch.uint8, dev)
    check(L.srf_boxes_augment(_ptr(boxes), _ptr(labels), n, box_dim, int(steps), hf(aug) if aug is not None else None,
                              hf(bev_range) if bev_range is not None else None, int(num_classes), _ptr(out), _ptr(out_labels),
                              _ptr(index), _ptr(num), _ptr(ws), _stream()), "boxes_augment")
    M = int(num.item())
    res = (out[:M], out_labels[:M])
    return res + (index[:M],) if with_index else res


def grid_mask(x, d, l, st_h, st_w, use_h=True, use_w=True, mode=1):
    """GridMask's `x * mask` out of place on a (..., H, W) float32 tensor: the stripe mask of grid_mask.py:72-128 (rotate 0,
    no offset) evaluated per pixel, never materialised.  x itself is not changed."""
    x = _dev(x, "x", torch.float32)
    if x.dim() < 2:
        raise RuntimeError("srfdet3d_amd: grid_mask expects (..., H, W)")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    planes = x.numel() // (H * W) if H * W else 0
    out = torch.empty_like(x)
    check(_lib.lib().srf_grid_mask(_ptr(x), planes, H, W, int(d), int(l), int(st_h), int(st_w), int(bool(use_h)),
                                   int(bool(use_w)), int(mode), _ptr(out), _stream()), "grid_mask")
    return out


# ---------------------------------------------------------------------------------------------- GT sampling / object noise
def points_in_boxes(points, planes, box_mask=None, num_outside=None):
    """First box per point whose six surface planes (m, 6, 4) [a, b, c, d] all give ((x a + y b) + z c) + d < 0, else -1
    -> int32 (n,).  box_mask (m,) int32: boxes with 0 are skipped.  num_outside: a device int32 (1,) that receives the count
    of -1s.  No host sync."""
    points = _dev(points, "points", torch.float32)
    planes = _dev(planes, "planes", torch.float32)
    n, nf = points.shape
    m = planes.shape[0]
    if planes.shape[1:] != (6, 4):
        raise RuntimeError(f"srfdet3d_amd: `planes` must be (m, 6, 4), got {tuple(planes.shape)}")
    mask = _dev(box_mask, "box_mask", torch.int32) if box_mask is not None else None
    if num_outside is not None and (num_outside.dtype != torch.int32 or not num_outside.is_cuda or num_outside.numel() < 1):
        raise RuntimeError("srfdet3d_amd: `num_outside` must be a device int32 tensor")
    out = _empty((max(n, 1),), torch.int32, points.device)
    check(_lib.lib().srf_points_in_boxes(_ptr(points), n, nf, _ptr(planes), m, _ptr(mask), _ptr(out), _ptr(num_outside), _stream()),
          "points_in_boxes")
    return out[:n]


def box_collision_matrix(boxes, qboxes):
    """box_collision_test of every (boxes[i], qboxes[j]) pair of BEV corners (N, 4, 2) x (K, 4, 2) -> bool (N, K)."""
    boxes = _dev(boxes, "boxes", torch.float32)
    qboxes = _dev(qboxes, "qboxes", torch.float32)
    N, K = boxes.shape[0], qboxes.shape[0]
    out = _empty((N, K), torch.uint8, boxes.device)
    check(_lib.lib().srf_box_collision_matrix(_ptr(boxes), N, _ptr(qboxes), K, _ptr(out), _stream()), "box_collision_matrix")
    return out.bool()


def box_collision_accept(fixed, cand, class_offsets, out=None):
    """The greedy rejection of DataBaseSampler.sample_all: fixed (n_fixed, 4, 2) and candidate (n_cand, 4, 2) BEV corners, the
    candidates grouped by class at class_offsets (device int32, num_classes + 1) -> int32 accept flags (n_cand,), written to
    `out` when given.  No host sync."""
    fixed = _dev(fixed, "fixed", torch.float32)
    cand = _dev(cand, "cand", torch.float32)
    off = _dev(class_offsets, "class_offsets", torch.int32)
    nc = cand.shape[0]
    if out is None:
        out = _empty((nc,), torch.int32, cand.device)
    check(_lib.lib().srf_box_collision_accept(_ptr(fixed), fixed.shape[0], _ptr(cand), nc, _ptr(off), off.numel() - 1, _ptr(out),
                                              _stream()), "box_collision_accept")
    return out


def object_sample_merge(points, point_box, sampled, obj_offsets, obj_centres, total):
    """cat([sampled rows + the centre of their object, points with point_box < 0]) -> (total, nf).  `total` (= s + the count
    of points in no box) is the caller's: it read it back together with the accept flags, so there is no sync here."""
    points = _dev(points, "points", torch.float32)
    point_box = _dev(point_box, "point_box", torch.int32)
    sampled = _dev(sampled, "sampled", torch.float32)
    off = _dev(obj_offsets, "obj_offsets", torch.int32)
    ctr = _dev(obj_centres, "obj_centres", torch.float32)
    n, nf = points.shape
    s = sampled.shape[0]
    if sampled.shape[1] != nf:
        raise RuntimeError(f"srfdet3d_amd: sampled points have {sampled.shape[1]} features, the sweep {nf}")
    L = _lib.lib()
    dev = points.device
    out = _empty((max(n + s, 1), nf), torch.float32, dev)
    num = _empty((1,), torch.int32, dev)
    ws = _empty((max(L.srf_object_sample_merge_workspace_bytes(n, s), 4),), torch.uint8, dev)
    check(L.srf_object_sample_merge(_ptr(points), n, nf, _ptr(point_box), _ptr(sampled), s, _ptr(off), _ptr(ctr), ctr.shape[0],
                                    _ptr(out), _ptr(num), _ptr(ws), _stream()), "object_sample_merge")
    return out[:total]


def object_noise(points, boxes, corners, planes, rot_sc, rot, loc):
    """noise_per_box + points_transform_ + box3d_transform_ (srf_object_noise) -> (points (n, nf), boxes (m, box_dim),
    chosen try per box int32 (m,), -1 where none fits).  Out of place, no host sync."""
    points = _dev(points, "points", torch.float32)
    boxes = _dev(boxes, "boxes", torch.float32)
    corners = _dev(corners, "corners", torch.float32)
    planes = _dev(planes, "planes", torch.float32)
    rot_sc = _dev(rot_sc, "rot_sc", torch.float32)
    rot = _dev(rot, "rot", torch.float64)
    loc = _dev(loc, "loc", torch.float64)
    n, nf = points.shape
    m, box_dim = boxes.shape
    num_try = rot.shape[1] if rot.dim() == 2 else 0
    if corners.shape != (m, 4, 2) or planes.shape != (m, 6, 4) or rot.shape != (m, num_try) or \
            rot_sc.shape != (m, num_try, 2) or loc.shape != (m, num_try, 3):
        raise RuntimeError("srfdet3d_amd: object_noise: corners / planes / rot_sc / rot / loc do not match the boxes")
    out_p = torch.empty_like(points)
    out_b = torch.empty_like(boxes)
    chosen = _empty((max(m, 1),), torch.int32, points.device)
    check(_lib.lib().srf_object_noise(_ptr(points), n, nf, _ptr(boxes), m, box_dim, _ptr(corners), _ptr(planes), _ptr(rot_sc),
                                      _ptr(rot), _ptr(loc), max(num_try, 1), _ptr(out_p), _ptr(out_b), _ptr(chosen), _stream()),
          "object_noise")
    return out_p, out_b, chosen[:m]


def image_prepare(images_u8, mean, std, to_rgb=False, size_divisor=32, size=None):
    """(V, H, W, 3) uint8 decoded views -> (V, 3, Hp, Wp) float32: NormalizeMultiviewImage + PadMultiViewImage + the
    HWC -> CHW transpose of the format bundle in one pass.  Padding to `size` (Hp, Wp) or up to a multiple of
    `size_divisor`."""
    if not isinstance(images_u8, torch.Tensor) or not images_u8.is_cuda or images_u8.dtype != torch.uint8:
        raise RuntimeError("srfdet3d_amd: `images_u8` must be a GPU uint8 tensor (no CPU fallback exists)")
    images_u8 = images_u8.contiguous()
    V, H, W, C = images_u8.shape
    if C != 3:
        raise RuntimeError("srfdet3d_amd: image_prepare expects 3-channel views")
    if size is not None:
        Hp, Wp = int(size[0]), int(size[1])
    else:
        d = int(size_divisor)
        Hp, Wp = -(-H // d) * d, -(-W // d) * d
    out = _empty((V, 3, Hp, Wp), torch.float32, images_u8.device)
    check(_lib.lib().srf_image_prepare(_ptr(images_u8), V, H, W, hf(mean), hf(std), int(bool(to_rgb)), Hp, Wp, _ptr(out),
                                       _stream()), "image_prepare")
    return out


def hard_voxelize(points, voxel_size, pc_range, max_points, max_voxels, mean_features=0, static=False, batch_index=0):
    """-> voxels (M,max_points,nf), coors (M,3) zyx, num (M,), mean (M,mean_features) or None.  One D2H sync for M.
    static=True: no sync; all min(n, max_voxels) rows are returned, rows >= M being padding (coors -1, num 0, zeros), the coordinates
    as (rows, 4) (batch_index, z, y, x), followed by the device scalar M -- the fixed-shape form a hipGraph can replay
    (srf_hard_voxelize_static: the padding is written by the gather kernel itself, no fills and no batch-column ops around it)."""
    points = _dev(points, "points", torch.float32)
    n, nf = points.shape
    L = _lib.lib()
    dev = points.device
    rows = max(min(n, max_voxels), 1)
    voxels = _empty((rows, max_points, nf), torch.float32, dev)
    coors = _empty((rows, 4 if static else 3), torch.int32, dev)
    num = _empty((rows,), torch.int32, dev)
    mean = _empty((rows, mean_features), torch.float32, dev) if mean_features else None
    vnum = _empty((1,), torch.int32, dev)
    ws_bytes = L.srf_hard_voxelize_workspace_bytes(n, max_points)
    ws = _empty((max(ws_bytes, 1),), torch.uint8, dev)
    if static:
        if n < 1:
            raise ValueError("hard_voxelize(static=True) needs at least one point row")
        check(L.srf_hard_voxelize_static(_ptr(points), n, nf, hf(voxel_size), hf(pc_range), hi(grid_size(voxel_size, pc_range)),
                                         max_points, max_voxels, _ptr(voxels), _ptr(coors), _ptr(num), _ptr(vnum), _ptr(mean),
                                         mean_features, int(batch_index), _ptr(ws), ws_bytes, _stream()), "hard_voxelize_static")
        return voxels, coors, num, mean, vnum
    check(L.srf_hard_voxelize(_ptr(points), n, nf, hf(voxel_size), hf(pc_range), hi(grid_size(voxel_size, pc_range)),
                              max_points, max_voxels, _ptr(voxels), _ptr(coors), _ptr(num), _ptr(vnum), _ptr(mean),
                              mean_features, _ptr(ws), ws_bytes, _stream()), "hard_voxelize")
    M = int(vnum.item())
    return voxels[:M], coors[:M], num[:M], (mean[:M] if mean is not None else None)


# ---------------------------------------------------------------------------------------------- dynamic scatter
class VoxelMap:
    """Sorted unique voxels of a (n,4) coordinate list and the point lists of each voxel."""

    def __init__(self, coors, grid_zyx, batch, known_num_voxels=None, static_rows=None):
        """static_rows: fixed-shape mode for hipGraph replay -- nothing is read back; `coors` / `reduce` have static_rows
        rows, those past the real count (device scalar `num_dev`) being padding (coordinates -1, zero features)."""
        coors = _dev(coors, "coors", torch.int32)
        n = coors.shape[0]
        L = _lib.lib()
        dev = coors.device
        self.n = n
        rows = max(n, 1)
        self.static = static_rows is not None
        out_coors = torch.full((rows, 4), -1, dtype=torch.int32, device=dev) if self.static else _empty((rows, 4), torch.int32, dev)
        self.point2voxel = _empty((rows,), torch.int32, dev)
        self.counts = _empty((rows,), torch.int32, dev)
        self.offsets = _empty((rows,), torch.int32, dev)
        self.order = _empty((rows,), torch.int32, dev)
        self.num_dev = _empty((1,), torch.int32, dev)
        ws_bytes = L.srf_voxel_unique_workspace_bytes(n, hi(grid_zyx), batch)
        if ws_bytes == 0 and n > 0:
            raise RuntimeError("srfdet3d voxel_unique: grid too large for 32-bit keys")
        ws = _empty((max(ws_bytes, 1),), torch.uint8, dev)
        check(L.srf_voxel_unique(_ptr(coors), n, hi(grid_zyx), batch, _ptr(out_coors), _ptr(self.point2voxel),
                                 _ptr(self.counts), _ptr(self.offsets), _ptr(self.order), _ptr(self.num_dev), _ptr(ws),
                                 ws_bytes, _stream()), "voxel_unique")
        # the one device->host read of this op; a caller that knows the count (all rows distinct) skips it
        if self.static:
            self.M = min(int(static_rows), rows)
        else:
            self.M = int(self.num_dev.item()) if known_num_voxels is None else int(known_num_voxels)
        self.coors = out_coors[:self.M]
        self.point2voxel = self.point2voxel[:n]

    def reduce(self, feats, mode):
        if torch.is_grad_enabled() and feats.requires_grad:
            return _ScatterReduceFn.apply(feats, self, mode)
        return self._reduce(feats, mode)

    def _reduce(self, feats, mode):
        feats = _dev(feats, "feats", torch.float32)
        C = feats.shape[1]
        if self.static:
            out = torch.zeros((max(self.M, 1), C), dtype=torch.float32, device=feats.device)
        else:
            out = _empty((max(self.M, 1), C), torch.float32, feats.device)
        check(_lib.lib().srf_scatter_reduce(_ptr(feats), _ptr(self.order), _ptr(self.offsets), _ptr(self.counts),
                                            _ptr(self.num_dev), self.M, C, 0 if mode == "mean" else 1, _ptr(out),
                                            _stream()), "scatter_reduce")
        return out[:self.M]


def spatial_order(indices, spatial_shape, batch):
    """Permutation that sorts DISTINCT active sites (A,4) (b,z,y,x) by (b, y, x, z): rows that are close in space
    become close in index, so a tile of consecutive output rows gathers from a compact set of input rows (L2 reuse,
    see csrc/spconv.hip).  Uses the occupancy-bitmap rank of K3 -- no sort, no host sync."""
    indices = _dev(indices, "indices", torch.int32)
    D, H, W = spatial_shape
    byxz = indices[:, [0, 2, 3, 1]].contiguous()
    vm = VoxelMap(byxz, [H, W, D], batch, known_num_voxels=indices.shape[0])
    return vm.order[:indices.shape[0]].long()


# ---------------------------------------------------------------------------------------------- rulebooks
class CoordTable:
    def __init__(self, capacity, device):
        self.capacity = capacity
        self.buf = _empty((capacity * 2,), torch.int32, device)


def coord_table_build(indices, spatial_shape, batch):
    indices = _dev(indices, "indices", torch.int32)
    L = _lib.lib()
    A = indices.shape[0]
    t = CoordTable(L.srf_coord_table_capacity(A), indices.device)
    check(L.srf_coord_table_build(_ptr(indices), A, hi(spatial_shape), batch, _ptr(t.buf), t.capacity, _stream()),
          "coord_table_build")
    return t


def rulebook_subm(indices, spatial_shape, ksize, table):
    indices = _dev(indices, "indices", torch.int32)
    A = indices.shape[0]
    K = int(np.prod(ksize))
    nbr = _empty((K, max(A, 1)), torch.int32, indices.device)
    counts = _empty((K,), torch.int32, indices.device)
    check(_lib.lib().srf_rulebook_subm(_ptr(indices), A, hi(spatial_shape), hi(ksize), _ptr(table.buf), table.capacity,
                                       _ptr(nbr), _ptr(counts), _stream()), "rulebook_subm")
    return nbr[:, :A], counts


def out_spatial_shape(shape, ksize, stride, pad):
    return [int((shape[d] + 2 * pad[d] - ksize[d]) // stride[d] + 1) for d in range(3)]


def rulebook_strided(indices, spatial_shape, batch, ksize, stride, pad):
    """-> out_indices (A_out,4), nbr (K,A_out), pair_counts (K,), out_table, out_shape.  One D2H sync for A_out."""
    indices = _dev(indices, "indices", torch.int32)
    L = _lib.lib()
    dev = indices.device
    A = indices.shape[0]
    K = int(np.prod(ksize))
    bound = L.srf_strided_max_outputs(A, batch, hi(spatial_shape), hi(ksize), hi(stride), hi(pad))
    if bound < 0:
        check(bound, "strided_max_outputs")
    table = CoordTable(L.srf_coord_table_capacity(bound), dev)
    out_idx = _empty((max(bound, 1), 4), torch.int32, dev)
    num_out = _empty((1,), torch.int32, dev)
    ws_bytes = L.srf_rulebook_strided_workspace_bytes(A, hi(ksize), table.capacity)
    ws = _empty((max(ws_bytes, 1),), torch.uint8, dev)
    check(L.srf_rulebook_strided_outputs(_ptr(indices), A, hi(spatial_shape), batch, hi(ksize), hi(stride), hi(pad),
                                         _ptr(out_idx), _ptr(num_out), _ptr(table.buf), table.capacity, _ptr(ws),
                                         ws_bytes, _stream()), "rulebook_strided_outputs")
    A_out = int(num_out.item())
    nbr = _empty((K, max(A_out, 1)), torch.int32, dev)
    counts = _empty((K,), torch.int32, dev)
    check(L.srf_rulebook_strided_pairs(A, hi(ksize), _ptr(table.buf), table.capacity, _ptr(ws), A_out, _ptr(nbr),
                                       _ptr(counts), _stream()), "rulebook_strided_pairs")
    return out_idx[:A_out], nbr[:, :A_out], counts, table, out_spatial_shape(spatial_shape, ksize, stride, pad)


# ---------------------------------------------------------------------------------------------- bitmap-rank rulebooks
class BitmapLevel:
    """Occupancy bitmap + popcount prefix of one level's grid; valid for rows sorted by (b, y, x, z)."""

    def __init__(self, spatial_shape, batch, device):
        self.shape = [int(v) for v in spatial_shape]
        self.batch = int(batch)
        self.words = _lib.lib().srf_bitmap_words(hi(self.shape), self.batch)
        if self.words == 0:
            raise ValueError("bitmap level: grid too large or empty")
        self.bitmap = _empty((self.words,), torch.int32, device)
        self.prefix = _empty((self.words,), torch.int32, device)

    def workspace(self):
        nbytes = _lib.lib().srf_bitmap_workspace_bytes(self.words)
        return _empty((nbytes,), torch.uint8, self.bitmap.device), nbytes


def bitmap_build(indices, spatial_shape, batch, want_order=True, padded=False):
    """Distinct active sites (A,4) (b,z,y,x) -> (BitmapLevel, order, sorted_indices): row r of the sorted set is
    original row order[r].  One clear + mark + rank scan (three launches; one workgroup for <= 8192 bitmap words) + place; no host sync.  padded=True: rows with b < 0 are
    padding of a capacity-sized set; the valid rows come first in the sorted result, padding stays (-1,...)."""
    indices = _dev(indices, "indices", torch.int32)
    lvl = BitmapLevel(spatial_shape, batch, indices.device)
    A = indices.shape[0]
    order = sorted_idx = None
    if want_order:
        # padded: rows with b < 0 are padding: their sorted slots become (-1,-1,-1,-1) and point at row 0 (written by the call)
        order = _empty((max(A, 1),), torch.int32, indices.device)
        sorted_idx = _empty((max(A, 1), 4), torch.int32, indices.device)
    ws, nbytes = lvl.workspace()
    build = _lib.lib().srf_bitmap_build_padded if padded and want_order else _lib.lib().srf_bitmap_build
    check(build(_ptr(indices), A, hi(lvl.shape), lvl.batch, _ptr(lvl.bitmap), _ptr(lvl.prefix), _ptr(order), _ptr(sorted_idx), _ptr(ws),
                nbytes, _stream()), "bitmap_build")
    if not want_order:
        return lvl, None, None
    return lvl, order[:A], sorted_idx[:A]


def rulebook_subm_bitmap(sorted_indices, level, ksize, want_counts=True):
    sorted_indices = _dev(sorted_indices, "indices", torch.int32)
    A = sorted_indices.shape[0]
    K = int(np.prod(ksize))
    nbr = _empty((K, max(A, 1)), torch.int32, sorted_indices.device)
    counts = _empty((_lib.lib().srf_bitmap_pair_count_ints(),), torch.int32, sorted_indices.device) if want_counts else None
    check(_lib.lib().srf_bitmap_rulebook_subm(_ptr(sorted_indices), A, hi(level.shape), level.batch, hi(ksize), _ptr(level.bitmap),
                                              _ptr(level.prefix), _ptr(nbr), _ptr(counts), _stream()), "bitmap_rulebook_subm")
    return nbr[:, :A], (counts[:K] if want_counts else None)


def rulebook_strided_bitmap(indices, level, ksize, stride, pad, out_capacity=None):
    """-> out_indices (A_out,4) sorted by (b,y,x,z), nbr (K,A_out), pair_counts (K,), the output BitmapLevel, out_shape.
    One D2H sync for A_out.  With out_capacity the shapes are static: out_indices has out_capacity rows (padding rows are
    -1), nbr is (K, out_capacity) with -1 in the padding columns, nothing is read back, and the device scalar A_out is
    returned as a sixth value (the caller compares it with out_capacity once the frame is done)."""
    indices = _dev(indices, "indices", torch.int32)
    L = _lib.lib()
    dev = indices.device
    A = indices.shape[0]
    K = int(np.prod(ksize))
    static = out_capacity is not None
    if static:
        bound = int(out_capacity)
    else:
        bound = L.srf_strided_max_outputs(A, level.batch, hi(level.shape), hi(ksize), hi(stride), hi(pad))
        if bound < 0:
            check(bound, "strided_max_outputs")
    oshape = out_spatial_shape(level.shape, ksize, stride, pad)
    out_lvl = BitmapLevel(oshape, level.batch, dev)
    cap = max(bound, 1)
    out_idx = _empty((cap, 4), torch.int32, dev)   # static: the rows past the count are written as -1 by the call
    num_out = _empty((1,), torch.int32, dev)
    ws, nbytes = out_lvl.workspace()
    outputs = L.srf_bitmap_strided_outputs_static if static else L.srf_bitmap_strided_outputs
    check(outputs(_ptr(indices), A, hi(level.shape), level.batch, hi(ksize), hi(stride), hi(pad),
                                       _ptr(out_lvl.bitmap), _ptr(out_lvl.prefix), _ptr(out_idx), bound, _ptr(num_out), _ptr(ws),
                                       nbytes, _stream()), "bitmap_strided_outputs")
    # phase 2 reads the count on the device: it is enqueued before the host learns A_out, so the read-back below
    # overlaps it instead of leaving the GPU idle
    nbr = _empty((K, cap), torch.int32, dev)
    counts = None if static else _empty((L.srf_bitmap_pair_count_ints(),), torch.int32, dev)  # bookkeeping only
    check(L.srf_bitmap_strided_pairs(_ptr(out_idx), _ptr(num_out), bound, hi(level.shape), level.batch, hi(ksize), hi(stride),
                                     hi(pad), _ptr(level.bitmap), _ptr(level.prefix), A, _ptr(nbr), cap, int(static), _ptr(counts),
                                     _stream()), "bitmap_strided_pairs")
    if static:
        return out_idx, nbr, None, out_lvl, oshape, num_out
    A_out = int(num_out.item())
    return out_idx[:A_out], nbr[:, :A_out], counts[:K], out_lvl, oshape


# ---------------------------------------------------------------------------------------------- sparse conv
# bench.py sets this to {"spconv": []}: every sparse-conv launch is then bracketed by HIP events on the launch stream
KERNEL_TIMING = None


# Which (K, Cin, Cout) has a packed-weight kernel, a bf16-product form and a row plan is ONE table of the library (srf_spconv_shape,
# csrc/spconv_frame.hpp); the four questions below are host calls into it, no GPU work.
def spconv_packed_supported(K, Cin, Cout):
    """True for the layer shapes with a packed-weight kernel."""
    return _lib.lib().srf_spconv_packed_weight_bytes(K, Cin, Cout) > 0


def spconv_plan_kind(K, Cin, Cout):
    """The plan the packed kernel of this shape takes as `tiles=`: 0 none, 1 row ranges (`spconv_tiles`), 2 a row order (`spconv_order`)."""
    return _lib.lib().srf_spconv_plan_kind(K, Cin, Cout)


def spconv_input_ok(rows, Cin):
    """An input the packed and the bf16-product kernels can address -- 32-bit byte offsets through a buffer descriptor: it has rows and
    lies below 2 GiB (`range32` of srf_spconv_check, csrc/spconv_frame.hpp); any other runs on srf_spconv_fwd."""
    return 0 < 4 * rows * Cin < (1 << 31)


def _rulebook(nbr):
    if not nbr.is_cuda or nbr.dtype != torch.int32 or nbr.stride(1) != 1:
        raise RuntimeError("srfdet3d_amd: `nbr` must be a GPU int32 tensor with unit inner stride")
    return nbr.shape


def pack_spconv_weights(weight):
    """(K,Cin,Cout) -> the operand layout srf_spconv_fwd_packed streams (once per layer; weights are constants), or None
    for a shape without a packed form."""
    weight = _dev(weight, "weight", torch.float32)
    K, Cin, Cout = weight.shape
    L = _lib.lib()
    nbytes = L.srf_spconv_packed_weight_bytes(K, Cin, Cout)
    if nbytes == 0:
        return None
    packed = _empty((nbytes // 4,), torch.float32, weight.device)
    check(L.srf_spconv_pack_weights(_ptr(weight), K, Cin, Cout, _ptr(packed), _stream()), "spconv_pack_weights")
    return packed


def spconv_bf16_supported(K, Cin, Cout):
    """True for the layer shapes `srf_spconv_fwd_bf16` takes."""
    return _lib.lib().srf_spconv_bf16_packed_weight_bytes(K, Cin, Cout) > 0


# (K, Cin, Cout) whose bf16-product form was NOT faster than the f32 route by more than the spread of three repeats
# (tools/bench_spconv_bf16.py, profiles/spconv_bf16_layer_bench.json): they keep the f32 route inside the mode
SPCONV_BF16_NOT_FASTER = frozenset()


def spconv_bf16_why_not(K, Cin, Cout):
    """None when the bf16-product mode (`sparse.mfma_dtype`) takes a layer of this shape, else the reason it keeps its f32 route."""
    if not spconv_bf16_supported(K, Cin, Cout):
        return "no bf16-product form for this shape"
    if (K, Cin, Cout) in SPCONV_BF16_NOT_FASTER:
        return "not faster (profiles/spconv_bf16_layer_bench.json)"
    return None


def pack_spconv_bf16_weights(weight):
    """(K,Cin,Cout) f32 -> the bf16 operand images `srf_spconv_fwd_bf16` stages (rounded once, here), or None for a shape without that
    form."""
    weight = _dev(weight, "weight", torch.float32)
    K, Cin, Cout = weight.shape
    L = _lib.lib()
    nbytes = L.srf_spconv_bf16_packed_weight_bytes(K, Cin, Cout)
    if nbytes == 0:
        return None
    packed = _empty((nbytes // 2,), torch.int16, weight.device)
    check(L.srf_spconv_bf16_pack_weights(_ptr(weight), K, Cin, Cout, _ptr(packed), _stream()), "spconv_bf16_pack_weights")
    return packed


def spconv_tiles_wanted(Cin, Cout):
    """True for the layer shapes whose packed kernel takes a row plan (`tiles=` of spconv_fwd): work-balanced row ranges
    (`spconv_tiles`) for the 64- / 128-channel kernels, a mask-sorted row order (`spconv_order`) for the 32-channel one."""
    return spconv_plan_kind(27, Cin, Cout) == 1 or spconv_order_wanted(Cin, Cout)


SPCONV_ORDER_MIN_ROWS = 100000   # rows of a level from which the sorted order pays for its launch (tools/spconv_order_probe.py, MI355X:
# nuScenes level 2, 60k rows: 32 -> 32 40.2 -> 35.5 us and 16 -> 32 22.7 -> 18.7 for 15-17 us of plan build per rulebook -- a loss;
# Waymo level 2, 226k rows: 145 -> 120 us and 70 -> 45 for 20 us -- 85 us per frame gained)


def spconv_order_wanted(Cin, Cout, K=27, rows=None):
    """rows=None: is this a layer shape the plan exists for; with rows: also, is the level large enough for it to pay
    (SRF_SPCONV_ORDER=0 / 2: never / at any size)."""
    mode = os.environ.get("SRF_SPCONV_ORDER", "1")
    if not (spconv_plan_kind(K, Cin, Cout) == 2 and mode != "0"):
        return False
    return rows is None or mode == "2" or rows >= SPCONV_ORDER_MIN_ROWS


def spconv_order(nbr, rows_dev=None):
    """The plan of `srf_spconv_order_build` for the rulebook nbr (K, A_out): int32 [order | sorted rulebook].  Built once per
    rulebook and passed as `tiles=` to every 32-channel spconv_fwd(..., packed=) that uses it."""
    K, A_out = _rulebook(nbr)
    L = _lib.lib()
    plan = _empty((max(L.srf_spconv_order_ints(A_out, K), 1),), torch.int32, nbr.device)
    check(L.srf_spconv_order_build(_ptr(nbr), nbr.stride(0) if A_out > 0 else 0, K, A_out, _ptr(rows_dev), _ptr(plan), _stream()),
          "spconv_order_build")
    return plan


def spconv_tiles(nbr, rows_dev=None):
    """Row ranges of equal pair count for the rulebook nbr (K, A_out): int32 (srf_spconv_tiles_count(A_out) + 1,).
    Built once per rulebook and passed to every spconv_fwd(..., packed=, tiles=) that uses it."""
    K, A_out = _rulebook(nbr)
    L = _lib.lib()
    tiles = _empty((L.srf_spconv_tiles_count(A_out) + 1,), torch.int32, nbr.device)
    ws = _empty((max(L.srf_spconv_tiles_workspace_bytes(A_out), 4),), torch.uint8, nbr.device)
    check(L.srf_spconv_tiles_build(_ptr(nbr), nbr.stride(0) if A_out > 0 else 0, K, A_out, _ptr(rows_dev), _ptr(ws), _ptr(tiles),
                                   _stream()), "spconv_tiles_build")
    return tiles


def spconv_fwd(feats, weight, nbr, alpha=None, beta=None, residual=None, relu=False, pair_counts=None, packed=None,
               rows_dev=None, tiles=None, subm=False):
    """feats (A_in,Cin); weight (K,Cin,Cout); nbr (K,A_out) (row stride nbr.stride(0)) -> (A_out,Cout).
    `packed` = pack_spconv_weights(weight) selects the packed-weight kernel for inputs below 2 GiB (larger ones and
    packed=None run srf_spconv_fwd, with the same bits); `tiles` = spconv_tiles(nbr) lets its 64- / 128-channel variants
    balance the workgroups by pair count."""
    if torch.is_grad_enabled() and (feats.requires_grad or weight.requires_grad or (residual is not None and residual.requires_grad)
                                    or (alpha is not None and alpha.requires_grad) or (beta is not None and beta.requires_grad)):
        # a gradient is wanted: plain convolution through the autograd Function (srf_spconv_bwd_data / _bwd_weight), the
        # epilogue as torch ops so that autograd differentiates it
        out = _SpconvFn.apply(feats, weight, nbr, bool(subm))
        if alpha is not None:
            out = out * alpha
        if beta is not None:
            out = out + beta
        if residual is not None:
            out = out + residual
        return torch.relu(out) if relu else out
    feats = _dev(feats, "feats", torch.float32)
    weight = _dev(weight, "weight", torch.float32)
    K, Cin, Cout = weight.shape
    if packed is not None and spconv_input_ok(feats.shape[0], Cin):
        return _spconv_launch("spconv_fwd_packed", feats, packed, weight.shape, nbr, alpha, beta, residual, relu, pair_counts, rows_dev,
                              _ptr(tiles) if spconv_tiles_wanted(Cin, Cout) else None)
    return _spconv_launch("spconv_fwd", feats, weight, weight.shape, nbr, alpha, beta, residual, relu, pair_counts, rows_dev)


def _spconv_launch(entry, feats, operand, wshape, nbr, alpha, beta, residual, relu, pair_counts, rows_dev, *plan):
    """One launch of the forward entry point srf_`entry`: rulebook check, output, timing bracket, record.  `operand`: the weights in the
    form that entry point reads; `plan`: its `tiles` argument, where it has one."""
    K, Cin, Cout = wshape
    A_out = _rulebook(nbr)[1]
    out = _empty((A_out, Cout), torch.float32, feats.device)
    if residual is not None:
        residual = _dev(residual, "residual", torch.float32)
    timing = KERNEL_TIMING
    if timing is not None and torch.cuda.is_current_stream_capturing():
        timing = None  # events recorded inside a graph capture are not timing events
    if timing is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    check(getattr(_lib.lib(), "srf_" + entry)(_ptr(feats), feats.shape[0], Cin, _ptr(operand), K, _ptr(nbr), nbr.stride(0) if A_out > 0 else 0,
                                              A_out, Cout, _ptr(alpha), _ptr(beta), _ptr(residual), int(bool(relu)), _ptr(out), _ptr(rows_dev),
                                              *plan, _stream()), entry)
    if timing is not None:
        ev1.record()
        timing["spconv"].append(_SpconvRecord(ev0, ev1, Cin, Cout, K, feats.shape[0], A_out, pair_counts, residual is not None))
    return out


def spconv_fwd_bf16(feats, weight, nbr, packed_bf16, alpha=None, beta=None, residual=None, relu=False, pair_counts=None,
                    rows_dev=None, tiles=None):
    """spconv_fwd on the bf16-product kernel (csrc/spconv_bf16.hip; OTHER values than spconv_fwd: inputs and weights rounded to bf16
    once, exact products, f32 accumulation and epilogue -- tests/spconv_bf16_ref.py is the definition).  `packed_bf16` =
    pack_spconv_bf16_weights(weight) -- `spconv_fwd(..., packed_bf16=)` as a function of its own, because the argument list of
    spconv_fwd is part of the recorded call sequence tests/test_sparse_calls.py holds the f32 encoder to.  Routed like `packed=`: an
    input of 2 GiB or more (or none) takes the f32 route srf_spconv_fwd.  `tiles` may be a plan of spconv_tiles(nbr); the kernel takes
    none and its bits do not depend on it.  Inference only: a wanted gradient raises."""
    if torch.is_grad_enabled() and (feats.requires_grad or weight.requires_grad or (residual is not None and residual.requires_grad)
                                    or (alpha is not None and alpha.requires_grad) or (beta is not None and beta.requires_grad)):
        raise RuntimeError("srfdet3d_amd: the bf16-product sparse convolution has no backward (inference under no_grad only)")
    if packed_bf16 is None:
        raise RuntimeError("srfdet3d_amd: spconv_fwd_bf16 needs pack_spconv_bf16_weights(weight); this shape has no bf16-product form")
    feats = _dev(feats, "feats", torch.float32)
    K, Cin, Cout = weight.shape
    if not spconv_input_ok(feats.shape[0], Cin):
        return spconv_fwd(feats, weight, nbr, alpha, beta, residual, relu, pair_counts=pair_counts, rows_dev=rows_dev)
    return _spconv_launch("spconv_fwd_bf16", feats, packed_bf16, weight.shape, nbr, alpha, beta, residual, relu, pair_counts, rows_dev,
                          _ptr(tiles))


class _SpconvRecord:
    """(start, end, Cin, Cout, K, algorithmic flops, algorithmic bytes) of one launch; the pair count is read from the
    rulebook's device counters only when the record is unpacked, after the timed region."""

    def __init__(self, ev0, ev1, cin, cout, K, a_in, a_out, pair_counts, has_residual=False):
        self.v = (ev0, ev1, cin, cout, K)
        self.a_in, self.a_out, self.pair_counts, self.has_residual = a_in, a_out, pair_counts, has_residual

    def __iter__(self):
        ev0, ev1, cin, cout, K = self.v
        pairs = int(self.pair_counts.sum().item()) if self.pair_counts is not None else 0
        flops = 2 * pairs * cin * cout
        byts = 4 * (self.a_in * cin + self.a_out * cout) + 4 * K * cin * cout + 8 * pairs
        if self.has_residual:
            byts += 4 * self.a_out * cout  # the residual rows are read once
        return iter((ev0, ev1, cin, cout, K, flops, byts))


def densify(feats, indices, batch, spatial_shape):
    if torch.is_grad_enabled() and feats.requires_grad:
        return _DensifyFn.apply(feats, indices, batch, tuple(spatial_shape))
    return _densify(feats, indices, batch, spatial_shape)


def densify_bev(feats, level, batch, spatial_shape):
    """sorted rows (A, C) + their BitmapLevel -> the BEV map (batch, C * D, H, W) with CHANNELS-LAST strides: dense() + the
    (N, C, D, H, W) -> (N, C * D, H, W) view in one pass (no zero fill, no transpose; srf_densify_bev).  Inference only."""
    feats = _dev(feats, "feats", torch.float32)
    A, C = feats.shape
    D, H, W = [int(v) for v in spatial_shape]
    if [int(v) for v in level.shape] != [D, H, W] or level.batch != batch:
        raise ValueError("densify_bev: the bitmap level belongs to another grid")
    out = torch.empty((batch, C * D, H, W), dtype=torch.float32, device=feats.device, memory_format=torch.channels_last)
    check(_lib.lib().srf_densify_bev(_ptr(feats), A, C, _ptr(level.bitmap), _ptr(level.prefix), batch, D, H, W, _ptr(out), _stream()),
          "densify_bev")
    return out


# ---------------------------------------------------------------------------------------------- pillar encoder
def pillar_enabled():
    """SRF_PILLAR=0 keeps `plugin.pillar.PillarFeatureNetCustom` and `PointPillarsScatter` on their torch / `densify` route on the GPU as
    well: what the pillar configs ran before csrc/pillar.hip, the route the tests and tools/bench_pillar.py alternate against.  Read at
    every call."""
    return os.environ.get("SRF_PILLAR", "1") != "0"


def pillar_vfe_ok(rows, P, nf, Cout):
    """The shapes `srf_pillar_vfe` takes (csrc/pillar.hip, the SRF_EUNSUPPORTED line of the entry point): a lane per output channel in
    waves of 64 and at most 4 channel groups, the point features in registers, a pillar's points in one LDS slab, `voxels` and `out`
    inside 32-bit byte ranges."""
    return Cout % 64 == 0 and 0 < Cout <= 256 and 3 <= nf <= 8 and 1 <= P <= 64 and below_2gb(rows, P * nf) and below_2gb(rows, Cout)


def pillar_scatter_ok(rows, C, B, H, W):
    """The shapes `srf_pillar_scatter_nhwc` takes: whole float4s per pillar, `feats` and the canvas inside 32-bit byte ranges."""
    return quads_ok(C) and below_2gb(rows, C) and below_2gb(B * H * W, C)


def pillar_vfe(voxels, num, coors4, weight, scale, shift, voxel_size, offset, cluster_center=True, voxel_center=True, legacy=True,
               rows_dev=None):
    """The single-layer, mode="max" pillar feature net in one launch (`srf_pillar_vfe`; definition in csrc/pillar.hip and, as numpy, in
    tests/pillar_ref.py).  voxels (rows, P, nf) zero-padded, num (rows) int32, coors4 (rows, 4) int32 (b, z, y, x), weight (Cout, K) with
    K = nf + 3 * cluster + 3 * centre, scale / shift (Cout) the folded eval BatchNorm, voxel_size / offset three host floats (x, y, z);
    rows_dev: device count of live rows (None: all).  -> (rows, Cout); padding rows are zeros."""
    voxels = _dev(voxels, "voxels", torch.float32)
    num = _dev(num, "num", torch.int32)
    coors4 = _dev(coors4, "coors4", torch.int32)
    weight = _dev(weight, "weight", torch.float32)
    scale = _dev(scale, "scale", torch.float32)
    shift = _dev(shift, "shift", torch.float32)
    rows, P, nf = voxels.shape
    Cout, K = weight.shape
    if K != nf + 3 * bool(cluster_center) + 3 * bool(voxel_center) or scale.numel() != Cout or shift.numel() != Cout:
        raise ValueError("pillar_vfe: weight must be (Cout, nf + 3 * cluster + 3 * centre), scale and shift (Cout)")
    if num.numel() != rows or tuple(coors4.shape) != (rows, 4):
        raise ValueError("pillar_vfe: num must be (rows,), coors4 (rows, 4)")
    if rows_dev is not None:
        rows_dev = _dev(rows_dev, "rows_dev", torch.int32)
    out = _empty((rows, Cout), torch.float32, voxels.device)
    check(_lib.lib().srf_pillar_vfe(_ptr(voxels), _ptr(num), _ptr(coors4), _ptr(rows_dev), rows, P, nf, hf(voxel_size), hf(offset),
                                    int(bool(cluster_center)), int(bool(voxel_center)), int(bool(legacy)), _ptr(weight), _ptr(scale),
                                    _ptr(shift), Cout, _ptr(out), _stream()), "pillar_vfe")
    return out


def pillar_scatter_nhwc(feats, coors4, batch, ny, nx, rows_dev=None, out=None):
    """PointPillarsScatter: pillar features (rows, C) + coors4 (rows, 4) int32 (b, z, y, x) -> the canvas (batch, C, ny, nx) with
    CHANNELS-LAST strides (`srf_pillar_scatter_nhwc`: zero fill and a 16-byte copy per quad, no transpose).  Rows with b < 0 or past
    `rows_dev` (a device count, None: all rows) are skipped.  `out`: a canvas of that shape and layout to write into.  Inference only."""
    feats = _dev(feats, "feats", torch.float32)
    coors4 = _dev(coors4, "coors4", torch.int32)
    rows, C = feats.shape
    if tuple(coors4.shape) != (rows, 4):
        raise ValueError("pillar_scatter_nhwc: coors4 must be (rows, 4)")
    if rows_dev is not None:
        rows_dev = _dev(rows_dev, "rows_dev", torch.int32)
    batch, ny, nx = int(batch), int(ny), int(nx)
    if out is None:
        out = torch.empty((batch, C, ny, nx), dtype=torch.float32, device=feats.device, memory_format=torch.channels_last)
    elif (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (batch, C, ny, nx)
          or not out.permute(0, 2, 3, 1).is_contiguous()):
        raise ValueError("pillar_scatter_nhwc: `out` must be an f32 GPU tensor (batch, C, ny, nx) with channels-last strides")
    check(_lib.lib().srf_pillar_scatter_nhwc(_ptr(feats), _ptr(coors4), _ptr(rows_dev), rows, C, batch, ny, nx, _ptr(out), _stream()),
          "pillar_scatter_nhwc")
    return out


# ---------------------------------------------------------------------------------------------- dynamic voxel encoder
def dvfe_enabled():
    """SRF_DVFE=0 keeps `plugin.voxel_encoders.DynamicVFECustom` on its torch route on the GPU as well: what the dynamic-voxelization
    configs ran before csrc/dvfe.hip, the route the tests and tools/bench_dvfe.py alternate against.  Read at every call."""
    return os.environ.get("SRF_DVFE", "1") != "0"


def dvfe_ok(n, rows, nf, d, C0, C1=0):
    """The shapes `srf_dvfe_fwd` takes (csrc/dvfe.hip, the SRF_EUNSUPPORTED line of the entry point): the raw features in 8 register
    slots, a position encoder of 16, 32 or 64 channels, layers of at most 16 channels (C1 = 0: one layer), `points`, the per-point
    workspace and `out` inside 32-bit byte ranges."""
    return (3 <= nf <= 8 and d in (16, 32, 64) and 1 <= C0 <= 16 and 0 <= C1 <= 16 and below_2gb(n, nf) and below_2gb(n, C0)
            and below_2gb(rows, C1 if C1 > 0 else C0))


def dvfe(points, vm, voxel_size, offset, voxel_center, pos_enc, layers):
    """DynamicVFECustom.forward in eval mode behind a `VoxelMap`, in two launches (`srf_dvfe_fwd`; definition in csrc/dvfe.hip and, as
    numpy, in tests/dvfe_ref.py).  points (n, nf) f32; vm the map of their (n, 4) coordinates; voxel_size / offset three host floats
    (x, y, z); pos_enc = (W1 (d, 3), scale1, shift1, W2 (d, d), scale2, shift2); layers = [(Wa (C0, nf + d + 3 * voxel_center), scale,
    shift)] or that and (Wb (C1, 2 * C0), scale, shift); scales and shifts are folded eval BatchNorms.  -> (vm.M, C_last); in static mode
    the rows past the device count are zeros."""
    points = _dev(points, "points", torch.float32)
    n, nf = points.shape
    if n != vm.n:
        raise ValueError("dvfe: the voxel map belongs to another point list")
    W1, s1, h1, W2, s2, h2 = [_dev(t, "pos_enc", torch.float32) for t in pos_enc]
    if not 1 <= len(layers) <= 2:
        raise ValueError("dvfe: one or two layers")
    Wa, sa, ha = [_dev(t, "layers[0]", torch.float32) for t in layers[0]]
    Wb, sb, hb = [_dev(t, "layers[1]", torch.float32) for t in layers[1]] if len(layers) == 2 else (None, None, None)
    d, C0 = W1.shape[0], Wa.shape[0]
    C1 = Wb.shape[0] if Wb is not None else 0
    centre = bool(voxel_center)
    if tuple(W1.shape) != (d, 3) or tuple(W2.shape) != (d, d) or any(t.numel() != d for t in (s1, h1, s2, h2)):
        raise ValueError("dvfe: pos_enc must be W1 (d, 3), W2 (d, d) and four vectors of d")
    if tuple(Wa.shape) != (C0, nf + d + 3 * centre) or sa.numel() != C0 or ha.numel() != C0:
        raise ValueError("dvfe: the first layer must be (C0, nf + d + 3 * voxel_center) with scale and shift (C0)")
    if C1 and (tuple(Wb.shape) != (C1, 2 * C0) or sb.numel() != C1 or hb.numel() != C1):
        raise ValueError("dvfe: the second layer must be (C1, 2 * C0) with scale and shift (C1)")
    C = C1 or C0
    out = _empty((vm.M, C), torch.float32, points.device)
    if n == 0 or vm.M == 0:
        return out
    L = _lib.lib()
    ws_bytes = L.srf_dvfe_workspace_bytes(n, C0)
    ws = _empty((max(ws_bytes, 1),), torch.uint8, points.device)
    check(L.srf_dvfe_fwd(_ptr(points), n, nf, _ptr(vm.point2voxel), _ptr(vm.order), _ptr(vm.offsets), _ptr(vm.counts), _ptr(vm.num_dev),
                         _ptr(vm.coors), vm.M, hf(voxel_size), hf(offset), int(centre), _ptr(W1), _ptr(s1), _ptr(h1), _ptr(W2), _ptr(s2),
                         _ptr(h2), d, _ptr(Wa), _ptr(sa), _ptr(ha), C0, _ptr(Wb), _ptr(sb), _ptr(hb), C1, _ptr(out), _ptr(ws), ws_bytes,
                         _stream()), "dvfe_fwd")
    return out


def _densify(feats, indices, batch, spatial_shape):
    feats = _dev(feats, "feats", torch.float32)
    indices = _dev(indices, "indices", torch.int32)
    A, C = feats.shape
    D, H, W = spatial_shape
    out = _empty((batch, C, D, H, W), torch.float32, feats.device)
    check(_lib.lib().srf_densify(_ptr(feats), _ptr(indices), A, C, batch, D, H, W, _ptr(out), 1, _stream()), "densify")
    return out


# ---------------------------------------------------------------------------------------------- gradients of the sparse half
def spconv_transpose_rulebook(nbr, a_in):
    """(K, A_out) output-stationary table -> (K, A_in): nbrT[k][i] = o <=> nbr[k][o] = i."""
    K, A_out = nbr.shape
    nbrT = _empty((K, max(a_in, 1)), torch.int32, nbr.device)
    check(_lib.lib().srf_spconv_transpose_rulebook(_ptr(nbr), nbr.stride(0) if A_out > 0 else 0, K, A_out, _ptr(nbrT), a_in,
                                                   _stream()), "spconv_transpose_rulebook")
    return nbrT[:, :a_in]


def _spconv_plain(feats, weight, nbr):
    """out[o] = sum_k W[k]^T in[nbr[k][o]] without epilogue; output widths below 16 run zero-padded on the 16-wide kernel."""
    K, Cin, Cout = weight.shape
    pad = 0
    if Cout not in (16, 32, 64, 128):
        if Cout > 16:
            raise RuntimeError(f"srfdet3d spconv: no kernel for {Cout} output channels")
        pad = 16 - Cout
        weight = torch.nn.functional.pad(weight, (0, pad))
    with torch.no_grad():
        out = spconv_fwd(feats.detach().contiguous(), weight.detach().contiguous(), nbr)
    return out[:, :Cout].contiguous() if pad else out


class _SpconvFn(torch.autograd.Function):
    """Sparse convolution with gradients: data gradient = the forward kernel on the transposed rulebook with transposed
    weights, weight gradient = srf_spconv_bwd_weight (csrc/spconv_bwd.hip)."""

    @staticmethod
    def forward(ctx, feats, weight, nbr, subm):
        ctx.save_for_backward(feats, weight, nbr)
        ctx.subm = subm
        return _spconv_plain(feats, weight, nbr)

    @staticmethod
    def backward(ctx, g):
        feats, weight, nbr = ctx.saved_tensors
        g = g.contiguous()
        K, Cin, Cout = weight.shape
        gf = gw = None
        if ctx.needs_input_grad[0]:
            wt = weight.detach().transpose(1, 2)
            if ctx.subm:   # symmetric rulebook: offset k of the transpose is offset K - 1 - k of the table itself
                nbrT, wt = nbr, wt.flip(0)
            else:
                nbrT = spconv_transpose_rulebook(nbr, feats.shape[0])
            gf = _spconv_plain(g, wt.contiguous(), nbrT)
        if ctx.needs_input_grad[1]:
            gw = _empty((K, Cin, Cout), torch.float32, g.device)
            f = feats.detach().contiguous()
            nbr_ld = nbr.stride(0) if nbr.shape[1] > 0 else 0
            if deterministic_enabled():   # the row ranges' partial sums stored and added in ascending order: no float atomics
                L = _lib.lib()
                ws_bytes = L.srf_spconv_bwd_weight_ordered_workspace_bytes(g.shape[0], Cin, Cout, K)
                ws = _empty((max(ws_bytes, 4) // 4,), torch.float32, g.device)
                check(L.srf_spconv_bwd_weight_ordered(_ptr(f), f.shape[0], Cin, _ptr(g), g.shape[0], Cout, _ptr(nbr), nbr_ld, K, _ptr(gw),
                                                      _ptr(ws), ws_bytes, _stream()), "spconv_bwd_weight_ordered")
            else:
                check(_lib.lib().srf_spconv_bwd_weight(_ptr(f), f.shape[0], Cin, _ptr(g), g.shape[0], Cout, _ptr(nbr), nbr_ld, K, _ptr(gw),
                                                       _stream()), "spconv_bwd_weight")
        return gf, gw, None, None


class _DensifyFn(torch.autograd.Function):
    """SparseConvTensor.dense(): scatter forward, gather backward."""

    @staticmethod
    def forward(ctx, feats, indices, batch, spatial_shape):
        ctx.save_for_backward(indices)
        return _densify(feats.detach(), indices, batch, spatial_shape)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        i = idx.long()
        ok = (i[:, 0] >= 0).unsqueeze(1)
        i = i.clamp(min=0)
        return g[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] * ok, None, None, None


class _ScatterReduceFn(torch.autograd.Function):
    """DynamicScatter mean / max over the points of a voxel.  mean: every point receives d_voxel / count; max: the gradient
    of a (voxel, channel) goes to the first point (in input order) that attains the maximum."""

    @staticmethod
    def forward(ctx, feats, vmap, mode):
        out = vmap._reduce(feats.detach(), mode)
        ctx.vmap, ctx.mode = vmap, mode
        ctx.save_for_backward(feats, out)
        return out

    @staticmethod
    def backward(ctx, g):
        feats, out = ctx.saved_tensors
        vm = ctx.vmap
        p2v = vm.point2voxel.long()
        ok = p2v >= 0
        pv = p2v.clamp(min=0)
        if ctx.mode == "mean":
            cnt = vm.counts[:vm.M].clamp(min=1).to(g.dtype).unsqueeze(1)
            return (g / cnt)[pv] * ok.unsqueeze(1), None, None
        n, C = feats.shape
        hit = (feats.detach() == out[pv]) & ok.unsqueeze(1)
        cand = torch.where(hit, torch.arange(n, device=g.device).unsqueeze(1).expand(n, C), torch.full((1, 1), n, device=g.device))
        first = torch.full((vm.M, C), n, dtype=torch.long, device=g.device).scatter_reduce(0, pv.unsqueeze(1).expand(n, C), cand, "amin")
        sel = hit & (first[pv] == torch.arange(n, device=g.device).unsqueeze(1))
        return g[pv] * sel, None, None


# ---------------------------------------------------------------------------------------------- RoI gather
def _featmap(t, scale):
    """4-D tensor in any dense layout (NCHW or channels-last) -> srf_featmap."""
    if t.dim() != 4 or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError("srfdet3d_amd: feature maps must be 4-D float32 GPU tensors")
    sn, sc, sh, sw = t.stride()
    return FeatMap(t.data_ptr(), t.shape[0], t.shape[2], t.shape[3], sn, sc, sh, sw, float(scale))


def roi_extract(feats, rois, strides, out_size=7, sampling_ratio=2, finest_scale=56.0, out=None, accumulate=False,
                bin_major=False, return_levels=False, n_sum=1):
    """SingleRoIExtractor over len(strides) maps.  out: (R,C,out_size,out_size), or (R,out_size^2,C) if bin_major; a given `out` may
    be a strided view (e.g. a channel slice of a wider buffer).  n_sum > 1: `rois` holds n_sum groups of R RoIs (group-major) and
    row r of the result is the sum of the gathers of rois[s * R + r], s ascending (`srf_roi_extract_sum`: the camera sum of
    srfdet_head.py:2543-2562 in the gather itself)."""
    rois = _dev(rois, "rois", torch.float32)
    if rois.shape[0] % n_sum:
        raise ValueError("roi_extract: the number of RoIs must be a multiple of n_sum")
    R = rois.shape[0] // n_sum
    C = feats[0].shape[1]
    nl = len(strides)
    fm = (FeatMap * nl)(*[_featmap(f, 1.0 / s) for f, s in zip(feats, strides)])
    bins = out_size * out_size
    shape = (R, bins, C) if bin_major else (R, C, out_size, out_size)
    if out is None:
        out = _empty(shape, torch.float32, rois.device)
        accumulate = False
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"roi_extract: out must be a float32 GPU tensor of shape {shape}")
    if bin_major:
        so_r, so_b, so_c = out.stride(0) if R > 1 else bins * C, out.stride(1), out.stride(2) if C > 1 else 1
    else:
        if out.stride(3) != 1 or out.stride(2) != out_size:
            raise ValueError("roi_extract: the bins of a channel must be contiguous in `out`")
        so_r, so_c, so_b = out.stride(0) if R > 1 else C * bins, out.stride(1) if C > 1 else bins, 1
    if n_sum > 1:
        if accumulate or return_levels:
            raise ValueError("roi_extract: n_sum excludes accumulate / return_levels")
        check(_lib.lib().srf_roi_extract_sum(fm, nl, C, _ptr(rois), R, n_sum, out_size, sampling_ratio, float(finest_scale), _ptr(out),
                                             so_r, so_c, so_b, _stream()), "roi_extract_sum")
        return out
    lv = _empty((max(R, 1),), torch.int32, rois.device) if return_levels else None
    check(_lib.lib().srf_roi_extract(fm, nl, C, _ptr(rois), R, out_size, sampling_ratio, float(finest_scale), _ptr(out),
                                     so_r, so_c, so_b, int(bool(accumulate)), _ptr(lv), _stream()), "roi_extract")
    return (out, lv[:R]) if return_levels else out


def box_rois(boxes, pc_range, voxel_size, mutate_centres=True, want_bev=True, lidar2img=None):
    """boxes (B,P,>=8) normalised centres -> rois_bev (B*P,5) and/or rois_img (n_cam*B*P,5)."""
    boxes = _dev(boxes, "boxes", torch.float32)
    B, P, D = boxes.shape
    dev = boxes.device
    rb = _empty((B * P, 5), torch.float32, dev) if want_bev else None
    ri, n_cam = None, 0
    if lidar2img is not None:
        lidar2img = _dev(lidar2img, "lidar2img", torch.float32)
        n_cam = lidar2img.shape[1]
        ri = _empty((n_cam * B * P, 5), torch.float32, dev)
    check(_lib.lib().srf_box_rois(_ptr(boxes), B, P, D, hf(pc_range), hf(voxel_size), int(bool(mutate_centres)), _ptr(rb),
                                  _ptr(lidar2img), n_cam, _ptr(ri), _stream()), "box_rois")
    return rb, ri


# ---------------------------------------------------------------------------------------------- NMS
def nms_rotated(boxes_xywhr, scores, iou_threshold, classes=None):
    """Greedy rotated NMS; returns indices (into the input) of the kept boxes, in descending score order.  classes (n,)
    int64: a box only suppresses boxes of its own class (per-class NMS in one pass)."""
    boxes_xywhr = _dev(boxes_xywhr, "boxes", torch.float32)
    n = boxes_xywhr.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.long, device=boxes_xywhr.device)
    order = scores.sort(dim=0, descending=True, stable=True)[1]  # equal scores (equal proposals): lower index first
    sorted_boxes = boxes_xywhr[order].contiguous()
    L = _lib.lib()
    keep = _empty((n,), torch.int32, boxes_xywhr.device)
    ws_bytes = L.srf_nms_rotated_workspace_bytes(n)
    ws = _empty((ws_bytes,), torch.uint8, boxes_xywhr.device)
    if classes is None:
        check(L.srf_nms_rotated(_ptr(sorted_boxes), n, float(iou_threshold), _ptr(keep), _ptr(ws), ws_bytes, _stream()),
              "nms_rotated")
    else:
        cls = _dev(classes, "classes", torch.int64)[order].contiguous()
        check(L.srf_nms_rotated_classes(_ptr(sorted_boxes), _ptr(cls), n, None, float(iou_threshold), _ptr(keep), _ptr(ws), ws_bytes,
                                        _stream()), "nms_rotated_classes")
    return order[keep.bool()]


def nms_rotated_counted(sorted_boxes_xywhr, n_live, iou_threshold, classes=None):
    """Greedy rotated NMS over the first n_live (device int32 scalar) rows of boxes already in descending score order;
    returns keep flags (n,) int32, zero past n_live.  Fixed shapes, nothing read back: graph-capturable.  classes (n,) int64:
    suppression only inside a class."""
    b = _dev(sorted_boxes_xywhr, "boxes", torch.float32)
    n = b.shape[0]
    keep = _empty((max(n, 1),), torch.int32, b.device)
    if n == 0:
        return keep[:0]
    L = _lib.lib()
    ws_bytes = L.srf_nms_rotated_workspace_bytes(n)
    ws = _empty((ws_bytes,), torch.uint8, b.device)
    if classes is None:
        check(L.srf_nms_rotated_counted(_ptr(b), n, _ptr(_dev(n_live, "n_live", torch.int32)), float(iou_threshold), _ptr(keep),
                                        _ptr(ws), ws_bytes, _stream()), "nms_rotated_counted")
    else:
        cls = _dev(classes, "classes", torch.int64)
        if cls.shape != (n,) or not cls.is_contiguous():
            raise ValueError("nms_rotated_counted: classes must be a contiguous (n,) int64 tensor")
        check(L.srf_nms_rotated_classes(_ptr(b), _ptr(cls), n, _ptr(_dev(n_live, "n_live", torch.int32)), float(iou_threshold),
                                        _ptr(keep), _ptr(ws), ws_bytes, _stream()), "nms_rotated_classes")
    return keep


def nms_select(boxes, scores, score_thr, capacity):
    """(n, D) boxes, (n, C) scores -> the L = min(n*C, capacity) best (box, class) pairs above score_thr in descending score:
    cand (L, D), top_s (L,), cls (L,) int64, bev (L, 5) for the rotated NMS, m (1,) int32 = pairs above the threshold.
    One single-workgroup launch (pairs above the threshold compacted, rank-sorted in LDS when <= 1024 of them, else a bitonic sort of
    all pairs), nothing read back: graph-capturable.  n*C <= 16384."""
    boxes = _dev(boxes, "boxes", torch.float32).contiguous()
    scores = _dev(scores, "scores", torch.float32).contiguous()
    n, D = boxes.shape
    C = scores.shape[1]
    L = min(n * C, int(capacity))
    dev = boxes.device
    cand, top_s = _empty((L, D), torch.float32, dev), _empty((L,), torch.float32, dev)
    cls, bev, m = _empty((L,), torch.int64, dev), _empty((L, 5), torch.float32, dev), _empty((1,), torch.int32, dev)
    check(_lib.lib().srf_nms_select(_ptr(boxes), _ptr(scores), n, C, D, float(score_thr), L, _ptr(cand), _ptr(top_s), _ptr(cls),
                                    _ptr(bev), _ptr(m), _stream()), "nms_select")
    return cand, top_s, cls, bev, m


def nms_finish(cand, top_s, cls, keep, m=None):
    """keep flags of the NMS over nms_select's candidates -> (boxes (L, D), scores (L,), labels (L,) int64, kept (1,) int32):
    survivors first, class-major, descending score inside a class.  With m (nms_select's count) also the packed form of the
    same rows, (L, D+2) [box, score, label], and counts (2,) int32 [kept, m]: one D2H copy per frame."""
    L, D = cand.shape
    dev = cand.device
    ob, os_, ol, kept = (_empty((L, D), torch.float32, dev), _empty((L,), torch.float32, dev), _empty((L,), torch.int64, dev),
                         _empty((1,), torch.int32, dev))
    packed = _empty((L, D + 2), torch.float32, dev) if m is not None else None
    counts = _empty((2,), torch.int32, dev) if m is not None else None
    check(_lib.lib().srf_nms_finish(_ptr(cand), _ptr(top_s), _ptr(cls), _ptr(_dev(keep, "keep", torch.int32)), L, D, _ptr(ob),
                                    _ptr(os_), _ptr(ol), _ptr(kept), _ptr(packed), _ptr(m), _ptr(counts), _stream()), "nms_finish")
    if m is not None:
        return ob, os_, ol, kept, packed, counts
    return ob, os_, ol, kept


# ---------------------------------------------------------------------------------------------- decoder stage
def _ln(ln):
    """nn.LayerNorm or (gamma, beta, eps) or None -> (ptr_g, ptr_b, eps)."""
    if ln is None:
        return None, None, 0.0
    if isinstance(ln, tuple):
        return _ptr(ln[0]), _ptr(ln[1]), float(ln[2])
    return _ptr(ln.weight), _ptr(ln.bias), float(ln.eps)


def linear(x, weight, bias=None, ln1=None, relu1=False, residual=None, ln2=None, relu2=False):
    """Y = [LN2]([residual +] relu1?([LN1](x @ weight.T + bias))), then relu2? -- one launch (two when K >= 2048 or N > 128
    with a row epilogue).  x (M,K), weight (N,K), both with unit inner stride."""
    x = _dev(x, "x", torch.float32)
    if not weight.is_cuda or weight.stride(1) != 1:
        raise RuntimeError("srfdet3d_amd: `weight` must be a GPU tensor with unit inner stride")
    M, K = x.shape
    N = weight.shape[0]
    L = _lib.lib()
    y = _empty((M, N), torch.float32, x.device)
    if residual is not None:
        residual = _dev(residual, "residual", torch.float32)
    need_ws = K >= 2048 or ((ln1 is not None or ln2 is not None or residual is not None or relu2) and N > 128)
    ws_bytes = L.srf_linear_workspace_bytes(M, N, K) if need_ws else 0
    ws = _empty((ws_bytes,), torch.uint8, x.device) if ws_bytes else None
    g1, b1, e1 = _ln(ln1)
    g2, b2, e2 = _ln(ln2)
    check(L.srf_linear(_ptr(x), M, K, x.stride(0), _ptr(weight), N, weight.stride(0), _ptr(bias), g1, b1, e1, int(bool(relu1)),
                       _ptr(residual), residual.stride(0) if residual is not None else 0, g2, b2, e2, int(bool(relu2)),
                       _ptr(y), N, _ptr(ws), ws_bytes, _stream()), "linear")
    return y


def self_attention(qkv, num_heads, out=None, batch=1):
    """qkv (batch * P, 3E) rows [q|k|v], sample-major -> (batch * P, E): softmax(q k^T / sqrt(d)) v per head among the P rows of
    each sample, one launch for the whole batch.  out: a contiguous (batch * P, E) tensor written in place."""
    qkv = _dev(qkv, "qkv", torch.float32)
    R, E3 = qkv.shape
    E = E3 // 3
    if batch < 1 or R % batch:
        raise ValueError("self_attention: rows must be batch * P")
    if out is None:
        out = _empty((R, E), torch.float32, qkv.device)
    elif tuple(out.shape) != (R, E) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != qkv.device:
        raise ValueError("self_attention: out must be a contiguous float32 (rows, E) tensor on the input's device")
    check(_lib.lib().srf_self_attention_batched(_ptr(qkv), batch, R // batch, E, num_heads, _ptr(out), _stream()), "self_attention")
    return out


def dynconv_mid(feats, params, ln1, ln2):
    """feats (R,S,C), params (R, 2*C*D) -> relu(LN_C(relu(LN_D(feats @ W1)) @ W2)), (R,S,C)."""
    feats = _dev(feats, "feats", torch.float32)
    params = _dev(params, "params", torch.float32)
    R, S, C = feats.shape
    D = params.shape[1] // (2 * C)
    out = _empty((R, S, C), torch.float32, feats.device)
    g1, b1, e1 = _ln(ln1)
    g2, b2, e2 = _ln(ln2)
    check(_lib.lib().srf_dynconv_mid(_ptr(feats), _ptr(params), R, S, C, D, g1, b1, e1, g2, b2, e2, _ptr(out), _stream()),
          "dynconv_mid")
    return out


def apply_deltas(deltas, boxes, weights6, pc_range, scale_clamp):
    deltas = _dev(deltas, "deltas", torch.float32)
    boxes = _dev(boxes, "boxes", torch.float32)
    R, Dd = deltas.shape
    out = _empty((R, Dd), torch.float32, deltas.device)
    check(_lib.lib().srf_apply_deltas(_ptr(deltas), _ptr(boxes), R, Dd, hf(weights6), hf(pc_range), float(scale_clamp),
                                      _ptr(out), _stream()), "apply_deltas")
    return out


def host_pack(packed, counts, level_counts):
    """float32 vector [packed.flatten(), counts, level_counts] (the ints converted; all < 2^24) in one launch."""
    a = _dev(packed, "packed", torch.float32)
    b = _dev(counts, "counts", torch.int32)
    c = _dev(level_counts, "level_counts", torch.int32)
    out = _empty((a.numel() + b.numel() + c.numel(),), torch.float32, a.device)
    check(_lib.lib().srf_host_pack(_ptr(a), a.numel(), _ptr(b), b.numel(), _ptr(c), c.numel(), _ptr(out), _stream()), "host_pack")
    return out


def decode_boxes(logits, pred, pc_range):
    """last-stage logits (..., ncls) and boxes (..., Dd) with normalised centres -> (scores, boxes (..., Dd - 1) in metres with
    bottom-centre z): the end of `forward` + SRFDetHead.decode (srfdet_head.py:1002-1006, :1246-1271) as one launch."""
    logits = _dev(logits, "logits", torch.float32)
    pred = _dev(pred, "pred", torch.float32)
    lead, ncls, Dd = logits.shape[:-1], logits.shape[-1], pred.shape[-1]
    R = int(np.prod(lead)) if len(lead) else 1
    scores = _empty((*lead, ncls), torch.float32, logits.device)
    boxes = _empty((*lead, Dd - 1), torch.float32, logits.device)
    check(_lib.lib().srf_decode_boxes(_ptr(logits), _ptr(pred), R, ncls, Dd, hf(pc_range), _ptr(scores), _ptr(boxes), _stream()),
          "decode_boxes")
    return scores, boxes


def upsample_add_supported(lateral, top):
    return (lateral.is_cuda and lateral.dtype == torch.float32 and top.dtype == torch.float32 and lateral.dim() == 4
            and lateral.shape[:2] == top.shape[:2] and lateral.shape[3] % 4 == 0 and lateral.is_contiguous() and top.is_contiguous()
            and not (torch.is_grad_enabled() and (lateral.requires_grad or top.requires_grad)))


def upsample_add(lateral, top):
    """lateral + F.interpolate(top, size=lateral.shape[2:], mode='nearest') in one pass (the FPN top-down step)."""
    lateral = _dev(lateral, "lateral", torch.float32)
    top = _dev(top, "top", torch.float32)
    N, C, H, W = lateral.shape
    out = _empty((N, C, H, W), torch.float32, lateral.device)
    check(_lib.lib().srf_upsample_add(_ptr(lateral), _ptr(top), N * C, H, W, top.shape[2], top.shape[3], _ptr(out), _stream()),
          "upsample_add")
    return out


def dwconv3x3s2(x, weight, scale=None, shift=None, relu=False):
    """Depthwise 3x3 / stride 2 / padding 1 convolution (weight (C, 1, 3, 3)) + per-channel scale/shift + ReLU."""
    x = _dev(x, "x", torch.float32).contiguous()
    N, C, H, W = x.shape
    w = _dev(weight, "weight", torch.float32).reshape(C, 9).contiguous()
    y = _empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), torch.float32, x.device)
    check(_lib.lib().srf_dwconv3x3s2(_ptr(x), N, C, H, W, _ptr(w), _ptr(scale), _ptr(shift), int(bool(relu)), _ptr(y), _stream()),
          "dwconv3x3s2")
    return y


def to_channels_last(x):
    """x.contiguous(memory_format=torch.channels_last) for a contiguous NCHW f32 GPU tensor with H*W % 4 == 0 (anything
    else goes through torch): same values, same strides, a faster transposing copy."""
    if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and (x.shape[2] * x.shape[3]) % 4 == 0
            and x.shape[1] > 1 and not (torch.is_grad_enabled() and x.requires_grad)):
        N, C, H, W = x.shape
        y = torch.empty((N, C, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        check(_lib.lib().srf_nchw_to_nhwc(_ptr(x), N, C, H * W, _ptr(y), _stream()), "nchw_to_nhwc")
        return y
    return x.contiguous(memory_format=torch.channels_last)


def ese_gate(mean, weight, bias):
    """(N, C) global averages, (C, C[, 1, 1]) fc weight, (C,) bias -> hsigmoid(fc(mean)) (N, C): VoVNet's eSE gate."""
    mean = _dev(mean, "mean", torch.float32).contiguous()
    N, C = mean.shape
    w = _dev(weight, "weight", torch.float32).reshape(C, C).contiguous()
    gate = _empty((N, C), torch.float32, mean.device)
    for n0 in range(0, N, 8):   # the GEMV kernel takes up to 8 rows per launch (6 cameras; 12 images at batch size 2)
        n1 = min(N, n0 + 8)
        check(_lib.lib().srf_ese_gate(_ptr(mean[n0:n1]), n1 - n0, C, _ptr(w), _ptr(bias), _ptr(gate[n0:n1]), _stream()), "ese_gate")
    return gate


def maxpool3s2_ceil(x):
    """nn.MaxPool2d(3, stride=2, ceil_mode=True) on a contiguous NCHW f32 tensor."""
    x = _dev(x, "x", torch.float32).contiguous()
    N, C, H, W = x.shape

    def osz(n):
        o = (n - 3 + 1) // 2 + 1 if n >= 3 else 1
        return o - 1 if (o - 1) * 2 >= n else o
    y = _empty((N, C, osz(H), osz(W)), torch.float32, x.device)
    check(_lib.lib().srf_maxpool3s2_ceil(_ptr(x), N * C, H, W, _ptr(y), _stream()), "maxpool3s2_ceil")
    return y


def channel_affine(x, scale, shift, relu, out=None, residual=None):
    """y = x * scale + shift (+ residual) (+ ReLU) on a contiguous NCHW tensor; scale / shift hold C values (per
    channel) or N*C values (per sample and channel); shift may be None.  `out` may be x itself or a channel slice of a
    wider contiguous NCHW tensor (same N, H, W)."""
    x = _dev(x, "x", torch.float32)
    N, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if out is None:
        out = torch.empty_like(x)
    if out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device:
        raise ValueError("channel_affine: out must match x")
    if HW and (out.stride(1) != HW or not out[0, 0].is_contiguous()):
        raise ValueError("channel_affine: out must be NCHW with contiguous channel planes")
    y_sn = out.stride(0) if N > 1 else C * HW
    if scale.numel() not in (C, N * C) or (shift is not None and shift.numel() != scale.numel()):
        raise ValueError("channel_affine: scale/shift must hold C or N*C values")
    per_sample = int(scale.numel() != C)
    if residual is not None:
        residual = _dev(residual, "residual", torch.float32)
        if residual.shape != x.shape:
            raise ValueError("channel_affine: residual must match x")
    check(_lib.lib().srf_channel_affine(_ptr(x), N, C, HW, C * HW, _ptr(_dev(scale, "scale", torch.float32)), _opt(shift, "shift"), per_sample,
                                        _ptr(residual), int(bool(relu)), _ptr(out), max(y_sn, C * HW), _stream()), "channel_affine")
    return out


def pack_conv1x1_weights(weight):
    """(Cout, K) or (Cout, K, 1, 1) -> the per-lane MFMA operand order srf_conv1x1 streams (once per layer)."""
    weight = _dev(weight.reshape(weight.shape[0], -1), "weight", torch.float32)
    Cout, K = weight.shape
    L = _lib.lib()
    nbytes = L.srf_conv1x1_packed_weight_bytes(Cout, K)
    if nbytes == 0:
        raise ValueError("conv1x1: Cout and K must be multiples of 32")
    packed = _empty((nbytes // 4,), torch.float32, weight.device)
    check(L.srf_conv1x1_pack_weights(_ptr(weight), Cout, K, _ptr(packed), _stream()), "conv1x1_pack_weights")
    return packed


def conv1x1_supported(xs, Cout):
    """Shapes srf_conv1x1 takes: contiguous NCHW f32 sources of equal N, H, W, channels % 32 == 0, H*W % 4 == 0."""
    x0 = xs[0]
    hw = x0.shape[2] * x0.shape[3]
    return (Cout % 128 == 0 and hw % 4 == 0 and hw >= 4 and 0 < len(xs) <= 8
            and all(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.shape[1] % 32 == 0
                    and x.shape[0] == x0.shape[0] and x.shape[2:] == x0.shape[2:] for x in xs))


def conv1x1(xs, packed_weight, Cout, scale=None, shift=None, relu=False):
    """1x1 convolution of cat(xs, dim=1) (never materialised) + per-channel scale/shift + ReLU -> (N, Cout, H, W)."""
    if not conv1x1_supported(xs, Cout):
        raise ValueError("conv1x1: unsupported shapes (see conv1x1_supported)")
    N, _, H, W = xs[0].shape
    out = _empty((N, Cout, H, W), torch.float32, xs[0].device)
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    chans = (ctypes.c_int * len(xs))(*[x.shape[1] for x in xs])
    K = sum(x.shape[1] for x in xs)
    if packed_weight.numel() != Cout * K:
        raise ValueError("conv1x1: packed weight does not match the sources")
    check(_lib.lib().srf_conv1x1(ptrs, chans, len(xs), N, H * W, _ptr(packed_weight), Cout, _opt(scale, "scale"), _opt(shift, "shift"),
                                 int(bool(relu)), _ptr(out), _stream()), "conv1x1")
    return out


# ---- channels-last (NHWC) dense convolutions (csrc/conv.hip) ---------------------------------------------------------
def _dense_timing(key):
    """(start event, record list) when bench.py asked for per-launch times of the dense kernels (KERNEL_TIMING[key]), else None."""
    t = KERNEL_TIMING
    if t is None or key not in t or torch.cuda.is_current_stream_capturing():
        return None
    ev0 = torch.cuda.Event(enable_timing=True)
    ev0.record()
    return ev0, t[key]


def _dense_timed(records, start, label, flops, executed, nbytes):
    """Closes a timed launch: records the end event and appends (start, end, label, FLOPs of the direct convolution, FLOPs the kernel
    executes, bytes moved) to `records` (None: the event only); returns the end event."""
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    if records is not None:
        records.append((start, end, label, flops, executed, nbytes))
    return end


def _dw_vectors(name, C, weight, scale, shift):
    """Lengths of a depthwise convolution's per-channel operands: weight C * 9, scale / shift C."""
    if weight.numel() != C * 9:
        raise ValueError(f"{name}: weight must be (C, 1, 3, 3)")
    for v, what in ((scale, "scale"), (shift, "shift")):
        if v is not None and v.numel() != C:
            raise ValueError(f"{name}: {what} must have C elements")


def nhwc_ld(x):
    """Floats per pixel of an (N, H, W, C) f32 view whose channels are a slice of a pixel-major buffer; raises if the
    view is not of that form."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise RuntimeError("srfdet3d: expected a 4-d f32 GPU tensor (N, H, W, C)")
    N, H, W, C = x.shape
    ld = x.stride(2) if W > 1 else (x.stride(1) if H > 1 else max(C, 1))
    ok = (C == 1 or x.stride(3) == 1) and ld >= C and (W == 1 or x.stride(2) == ld) and (H == 1 or x.stride(1) == W * ld) \
        and (N == 1 or x.stride(0) == H * W * ld)
    if not ok:
        raise RuntimeError(f"srfdet3d: tensor of shape {tuple(x.shape)} / strides {x.stride()} is not a channel slice of an NHWC buffer")
    return ld


def pack_wino3x3_weights(weight):
    """(Cout, Cin, 3, 3) -> G g G^T in the LDS operand order srf_wino3x3 copies (once per layer)."""
    weight = _dev(weight, "weight", torch.float32)
    Cout, Cin, kh, kw = weight.shape
    L = _lib.lib()
    nbytes = L.srf_wino3x3_packed_weight_bytes(Cout, Cin)
    if (kh, kw) != (3, 3) or nbytes == 0:
        raise ValueError("wino3x3: needs a (Cout, Cin, 3, 3) weight with Cin % 8 == 0")
    packed = _empty((nbytes // 4,), torch.float32, weight.device)
    check(L.srf_wino3x3_pack_weights(_ptr(weight), Cout, Cin, _ptr(packed), _stream()), "wino3x3_pack_weights")
    return packed


def quads_ok(n):
    """A channel count or pixel pitch in whole float4s: `x_ld & 3` of every channels-last entry (csrc/conv.hip:946; csrc/gemm_host.hpp,
    `srf_gemm_check_1x1` and `srf_gemm_check_conv`: `x_ld & 3`), `C & 3` of the streaming kernels (csrc/nhwc.hip:65)."""
    return n % 4 == 0


def operand_ok(ld, addr):
    """An operand the kernels read in float4s: pitch `ld` in quads from a 16-byte aligned address (csrc/conv.hip:946; csrc/gemm_host.hpp,
    `srf_gemm_check_1x1` and `srf_gemm_check_conv`: `x_ld & 3`, `(uintptr_t)x & 15`)."""
    return quads_ok(ld) and addr % 16 == 0


def wino3x3_channels_ok(Cin):
    """srf_wino3x3 packs its operand in chunks of 8 input channels (csrc/conv.hip:924, :946)."""
    return Cin % 8 == 0


def wino3x3_range_ok(pixels, ld):
    """One image, `pixels` of pitch `ld` floats, inside the 2^30 bytes the per-lane offsets of srf_wino3x3 reach (csrc/conv.hip:948)."""
    return 4 * pixels * ld < (1 << 30)


def stem_channels_ok(Cin, Cout):
    """srf_stem_conv_nchw: up to 4 image planes into exactly 64 channels (csrc/conv.hip:1410)."""
    return Cin <= 4 and Cout == 64


def stem7_channels_ok(Cin, Cout):
    """srf_stem_conv7_nchw: up to 4 image planes into exactly 64 channels (csrc/conv.hip:1547)."""
    return Cin <= 4 and Cout == 64


def stem7_range_ok(pixels, ld):
    """One image of srf_stem_conv7_nchw's output, `pixels` of pitch `ld` floats, inside the 2^31 bytes of its buffer descriptor
    (csrc/conv.hip:1551)."""
    return 4 * pixels * ld < (1 << 31)


def ese_channels_ok(C):
    """Channels of an eSE block's output: quads for srf_ese_gate (csrc/decoder.hip:445) and srf_nhwc_affine (csrc/nhwc.hip:65); C <= 1024
    as the gate held it (the bound of srf_nhwc_colmean, csrc/nhwc.hip:137, which took the eSE mean before the GEMM's epilogue did)."""
    return quads_ok(C) and C <= 1024


def wino3x3_supported(x):
    return (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and wino3x3_channels_ok(x.shape[3]) and operand_ok(x.stride(2), x.data_ptr())
            and wino3x3_range_ok(x.shape[1] * x.shape[2], x.stride(2)))


def wino3x3(x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None):
    """3x3 / stride 1 / padding 1 convolution of the NHWC slice x (N, H, W, Cin) + per-channel scale / shift + ReLU into
    `out` (an (N, H, W, Cout) slice of an NHWC buffer; a new contiguous tensor when None)."""
    x_ld = nhwc_ld(x)
    N, H, W, Cin = x.shape
    if out is None:
        out = _empty((N, H, W, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, H, W, Cout):
        raise ValueError("wino3x3: out has the wrong shape")
    y_ld = nhwc_ld(out)
    L = _lib.lib()
    if packed_weight.numel() * 4 != L.srf_wino3x3_packed_weight_bytes(Cout, Cin):
        raise ValueError("wino3x3: packed weight does not match (Cout, Cin)")
    timing = _dense_timing("wino")
    check(L.srf_wino3x3(_ptr(x), N, H, W, Cin, x_ld, _ptr(packed_weight), Cout, _opt(scale, "scale"), _opt(shift, "shift"), int(bool(relu)),
                        _ptr(out), y_ld, _stream()), "wino3x3")
    if timing is not None:
        # direct-convolution FLOPs, FLOPs the Winograd kernel executes on the MFMA (16 of 36 products), bytes in + out + weights
        direct = 2.0 * 9 * Cin * Cout * N * H * W
        _dense_timed(timing[1], timing[0], f"{Cin}->{Cout} @{N}x{H}x{W}", direct, direct / 2.25,
                     4.0 * N * H * W * (Cin + Cout) + 4.0 * 16 * Cin * Cout)
    return out


def pack_wino43_weights(weight):
    """(Cout, Cin, 3, 3) -> U = G g G^T of Winograd F(4x4, 3x3) in the operand order srf_wino43 streams (once per layer)."""
    weight = _dev(weight, "weight", torch.float32)
    Cout, Cin, kh, kw = weight.shape
    L = _lib.lib()
    nbytes = L.srf_wino43_packed_weight_bytes(Cout, Cin)
    if (kh, kw) != (3, 3) or nbytes == 0:
        raise ValueError("wino43: needs a (Cout, Cin, 3, 3) weight with Cin % 8 == 0")
    packed = _empty((nbytes // 4,), torch.float32, weight.device)
    check(L.srf_wino43_pack_weights(_ptr(weight), Cout, Cin, _ptr(packed), _stream()), "wino43_pack_weights")
    return packed


def wino43_channels_ok(Cin, Cout):
    """srf_wino43's channel multiples: 8 input channels per operand chunk (csrc/wino43.hip:461), output quads (:402)."""
    return Cin % 8 == 0 and Cout % 4 == 0


def wino43_range_ok(pixels, ld):
    """The images one slab of srf_wino43 touches, `pixels` of pitch `ld` floats, inside its 32-bit byte offsets (csrc/wino43.hip:561)."""
    return 4 * pixels * ld < (1 << 32) - 16


def wino43_tiles_ok(N, H, W):
    """The 4 x 4 output tiles of srf_wino43 inside an int: refused from 2^31 - 64 here, from 2^31 - 32 by the kernel (csrc/wino43.hip:546)."""
    return N * ((H + 3) // 4) * ((W + 3) // 4) < (1 << 31) - 64


def wino43_supported(x, Cout, out=None):
    """Shape / layout limits of srf_wino43 (csrc/wino43.hip: w43_make_args, w43_slab_args)."""
    if not (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and wino43_channels_ok(x.shape[3], Cout)):
        return False
    try:
        ld = nhwc_ld(x)
        old = nhwc_ld(out) if out is not None else Cout
    except RuntimeError:
        return False
    if not (operand_ok(ld, x.data_ptr()) and operand_ok(old, 0 if out is None else out.data_ptr())):
        return False
    N, H, W, _ = x.shape
    # one slab = the whole layer below 2 GB of V: its images must span less than 4 GB of x and of y
    return wino43_range_ok(N * H * W, max(ld, old)) and wino43_tiles_ok(N, H, W)


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def wino43(x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None):
    """3x3 / stride 1 / padding 1 convolution of the NHWC slice x (N, H, W, Cin) as Winograd F(4x4, 3x3) + per-channel scale /
    shift + ReLU into `out` (an (N, H, W, Cout) slice of an NHWC buffer; a new contiguous tensor when None)."""
    x_ld = nhwc_ld(x)
    N, H, W, Cin = x.shape
    if out is None:
        out = _empty((N, H, W, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, H, W, Cout):
        raise ValueError("wino43: out has the wrong shape")
    y_ld = nhwc_ld(out)
    L = _lib.lib()
    if packed_weight.numel() * 4 != L.srf_wino43_packed_weight_bytes(Cout, Cin):
        raise ValueError("wino43: packed weight does not match (Cout, Cin)")
    if N == 0:
        return out
    ws_bytes = L.srf_wino43_workspace_bytes(N, H, W, Cin, Cout)
    ws = _empty((ws_bytes // 4,), torch.float32, x.device)
    sc = None if scale is None else _aligned16(_dev(scale, "scale", torch.float32))
    sh = None if shift is None else _aligned16(_dev(shift, "shift", torch.float32))
    scp, shp = _ptr(sc), _ptr(sh)
    timing = _dense_timing("w43m")
    if timing is None:
        check(L.srf_wino43(_ptr(x), N, H, W, Cin, x_ld, _ptr(packed_weight), Cout, scp, shp, int(bool(relu)), _ptr(out), y_ld, _ptr(ws),
                           ws_bytes, _stream()), "wino43")
        return out
    # bench.py asked for per-launch times: the transform (HBM-bound) and the multiply (MFMA-bound) as separate calls
    rc = L.srf_wino43_transform(_ptr(x), N, H, W, Cin, x_ld, Cout, _ptr(ws), ws_bytes, _stream())
    if rc != 0:   # a layer cut into slabs cannot be timed apart
        check(L.srf_wino43(_ptr(x), N, H, W, Cin, x_ld, _ptr(packed_weight), Cout, scp, shp, int(bool(relu)), _ptr(out), y_ld, _ptr(ws),
                           ws_bytes, _stream()), "wino43")
        return out
    direct = 2.0 * 9 * Cin * Cout * N * H * W
    label = f"{Cin}->{Cout} @{N}x{H}x{W}"
    # transform: reads the input once, writes V (2.25x the input, padded to whole tile blocks)
    ev1 = _dense_timed(KERNEL_TIMING.get("w43x"), timing[0], label, 0.0, 0.0, 4.0 * N * H * W * Cin + ws_bytes)
    check(L.srf_wino43_multiply(_ptr(ws), ws_bytes, N, H, W, Cin, _ptr(packed_weight), Cout, scp, shp, int(bool(relu)), _ptr(out), y_ld,
                                _stream()), "wino43_multiply")
    # multiply: executes direct / 4 FLOPs on the MFMA; reads V and U once, writes the output
    _dense_timed(timing[1], ev1, label, direct, direct / 4.0, float(ws_bytes) + 4.0 * 36 * Cin * Cout + 4.0 * N * H * W * Cout)
    return out


# The three dense GEMM families behind conv1x1_nhwc / conv_gemm_nhwc (csrc/gemm_host.hpp): the C entry points of each by name, the
# element of its packed weight, what the error messages call that weight and what the timing labels add.  residual: the form that adds
# a bottleneck's identity before the ReLU (`conv1x1_nhwc_residual`); the bf16-product family has none.
_GEMM_KINDS = {
    "lds": dict(packed_bytes="srf_conv1x1_nhwc_packed_weight_bytes", pack="srf_conv1x1_nhwc_pack_weights", esize=4, dtype=torch.float32,
                plain="srf_conv1x1_nhwc", topdown="srf_conv1x1_nhwc_topdown", pooled="srf_conv1x1_nhwc_pooled", conv="srf_conv_gemm_nhwc",
                residual="srf_conv1x1_nhwc_residual", what="packed", tag=""),
    "direct": dict(packed_bytes="srf_conv1x1_nhwc_direct_packed_weight_bytes", pack="srf_conv1x1_nhwc_direct_pack_weights", esize=4,
                   dtype=torch.float32, plain="srf_conv1x1_nhwc_direct", topdown="srf_conv1x1_nhwc_direct_topdown",
                   pooled="srf_conv1x1_nhwc_direct_pooled", conv=None, residual="srf_conv1x1_nhwc_direct_residual", what="direct-packed",
                   tag=" direct"),
    "split": dict(packed_bytes="srf_conv1x1_nhwc_split_packed_weight_bytes", pack="srf_conv1x1_nhwc_split_pack_weights", esize=2,
                  dtype=torch.int16, plain="srf_conv1x1_nhwc_split", topdown="srf_conv1x1_nhwc_split_topdown",
                  pooled="srf_conv1x1_nhwc_split_pooled", conv="srf_conv_gemm_nhwc_split", residual="srf_conv1x1_nhwc_split_residual",
                  what="split-packed", tag=" split"),
    "bf16": dict(packed_bytes="srf_conv1x1_nhwc_bf16_packed_weight_bytes", pack="srf_conv1x1_nhwc_bf16_pack_weights", esize=2,
                 dtype=torch.int16, plain="srf_conv1x1_nhwc_bf16", topdown="srf_conv1x1_nhwc_bf16_topdown",
                 pooled="srf_conv1x1_nhwc_bf16_pooled", conv="srf_conv_gemm_nhwc_bf16", residual=None, what="bf16-packed", tag=" bf16"),
}


def gemm_k_ok(K):
    """Every family reads K in chunks of 32 (csrc/gemm_host.hpp, `srf_gemm_check_1x1`: `K & 31`; `srf_gemm_check_conv`: `Cin & 31`)."""
    return K % 32 == 0


def gemm_rows_ok(ld):
    """128 rows of pitch `ld` floats inside the 2^31-byte descriptor of the direct, split and bf16 families (csrc/gemm_host.hpp,
    `srf_gemm_check_1x1`: `x_ld * f.tile_rows * 4 >= 2^31`)."""
    return ld * 512 < (1 << 31)


def below_2gb(pixels, ld):
    """`pixels` rows of `ld` floats below 2 GB: the implicit-im2col input (csrc/gemm_host.hpp, `srf_gemm_check_conv`: `*x_bytes >= 2^31`), the weight
    gradient's operands (csrc/wgrad.hip:337)."""
    return 4 * pixels * ld < (1 << 31)


def gemm_bf16_why_not(x, Cout, out=None, im2col=False, dgrad=False):
    """None when the bf16 family takes the layer x (N, H, W, Cin) -> Cout channels [written into the channel slice `out`], else the
    reason it keeps its f32 route.  im2col: `srf_conv_gemm_nhwc_bf16`, which also holds one image of x to 2 GB, not the 1x1 GEMM.
    dgrad (the training nodes): the layer's data gradient is asked too -- the same kernel with K = Cout over a dense tensor of Cout
    channels -- and `out`'s alignment, for a layer that keeps both directions on one route."""
    N, H, W, Cin = x.shape
    try:
        x_ld, y_ld = nhwc_ld(x), (nhwc_ld(out) if out is not None else Cout)
    except RuntimeError:
        return "not a channel slice of a pixel-major buffer"
    if not (gemm_k_ok(Cin) and (not dgrad or gemm_k_ok(Cout))):
        return "input or output channels are no multiple of 32" if dgrad else "input channels are no multiple of 32"
    if not (operand_ok(x_ld, x.data_ptr()) and (not dgrad or out is None or operand_ok(y_ld, out.data_ptr()))):
        return "operand alignment"
    if not gemm_rows_ok(max(x_ld, y_ld)) or (im2col and not below_2gb(H * W, max(x_ld, Cout) if dgrad else x_ld)) or (dgrad and N == 0):
        return "beyond the 32-bit ranges"
    return None


def _pack_gemm(kind, weight):
    k = _GEMM_KINDS[kind]
    weight = _dev(weight.reshape(weight.shape[0], -1), "weight", torch.float32)
    Cout, K = weight.shape
    L = _lib.lib()
    nbytes = getattr(L, k["packed_bytes"])(Cout, K)
    if nbytes == 0:
        raise ValueError("conv1x1_nhwc: K must be a multiple of 32")
    if kind == "split" and not gemm_split_weight_in_domain(weight):
        return None     # callers keep such a layer on the f32-MFMA kernels
    packed = _empty((nbytes // k["esize"],), k["dtype"], weight.device)
    check(getattr(L, k["pack"])(_ptr(weight), Cout, K, _ptr(packed), _stream()), k["pack"][len("srf_"):])
    return packed


def _choose_gemm(op, layer, M, Cout, K, packed_weight, packed_direct=None, packed_split=None, packed_bf16=None):
    """The family a launch of M rows runs on and its packed weight -> (kind, row of _GEMM_KINDS, tensor).  Callables are called only for
    the family that is taken (the split one also when it is merely wanted: it may answer None).  packed_bf16 is the caller's explicit
    choice of the reduced-precision family (csrc/gemm_bf16.hip) and precedes the rules of the f32-accurate ones."""
    kind, packed = "lds", packed_weight
    if packed_bf16 is not None:
        kind, packed = "bf16", packed_bf16
    elif packed_split is not None and gemm_split_wanted(M, Cout):
        if callable(packed_split):
            packed_split = packed_split()
        if packed_split is not None:     # None: a weight outside the split's exact domain (gemm_split_weight_in_domain)
            kind, packed = "split", packed_split
    if kind == "lds" and packed_direct is not None and conv1x1_direct_wanted(M, Cout):
        kind, packed = "direct", packed_direct
    k = _GEMM_KINDS[kind]
    if callable(packed):
        packed = packed()
    if packed.numel() * k["esize"] != getattr(_lib.lib(), k["packed_bytes"])(Cout, K):
        raise ValueError(f"{op}: {k['what']} weight does not match {layer}")
    return kind, k, packed


def pack_conv1x1_nhwc_weights(weight):
    """(Cout, K) or (Cout, K, 1, 1) -> the LDS operand order srf_conv1x1_nhwc copies (once per layer)."""
    return _pack_gemm("lds", weight)


def pack_conv1x1_nhwc_direct_weights(weight):
    """(Cout, K) or (Cout, K, 1, 1) -> the operand order srf_conv1x1_nhwc_direct streams from L2 (once per layer)."""
    return _pack_gemm("direct", weight)


def pack_conv1x1_nhwc_bf16_weights(weight):
    """(Cout, K) or (Cout, K, 1, 1) -> the weight rounded to bf16 (round to nearest even) in the LDS operand order srf_conv1x1_nhwc_bf16
    copies (once per layer); an int16 tensor (2 bytes per weight, K padded to a multiple of 64)."""
    return _pack_gemm("bf16", weight)


def pack_conv1x1_nhwc_split_weights(weight):
    """(Cout, K) or (Cout, K, 1, 1) -> the three bf16 planes of the weight (w = wh + wm + wl exactly) in the LDS operand order
    srf_conv1x1_nhwc_split copies (once per layer); an int16 tensor (6 bytes per weight)."""
    return _pack_gemm("split", weight)


GEMM_SPLIT_MAX = float.fromhex("0x1.FEp127")   # the largest bf16 (3.3895e38): above it the first plane rounds to infinity


def gemm_split_weight_in_domain(weight):
    """The three-way bf16 split is exact for finite values of magnitude <= GEMM_SPLIT_MAX (csrc/gemm_split.hip, "Domain"); a weight
    outside that range (larger, infinite or NaN) would turn whole output columns into NaN where the f32 fma chain stays finite or
    propagates an infinity, so such a layer is kept on the f32-MFMA kernels.  Checked once per packed weight (one reduction and one
    device -> host read; skipped -- the weight taken as in range -- while a stream capture is running, where a read-back is illegal:
    the graphs are captured after an eager warm-up that has packed, and checked, every layer)."""
    if weight.is_cuda and torch.cuda.is_current_stream_capturing():
        return True
    return bool((weight.abs().max() <= GEMM_SPLIT_MAX).item()) if weight.numel() else True   # NaN compares False


def gemm_split_enabled():
    """SRF_GEMM_SPLIT=0 keeps the 1x1 convolutions on the f32-MFMA kernels (`srf_conv1x1_nhwc` / `_direct`: one k-ordered fma chain per
    output); the default runs them on `srf_conv1x1_nhwc_split` -- the same f32 GEMM through an exact three-way bf16 split of both
    operands on the bf16 MFMA (csrc/gemm_split.hip: error against float64 equal to the f32 chain's, 1.4-1.5x its rate)."""
    return os.environ.get("SRF_GEMM_SPLIT", "1") != "0"


GEMM_SPLIT_MIN_TILES = 128   # 128 x 128 tiles of a launch from which the split kernel is taken (tools/small_gemm_ab.py)


def gemm_split_wanted(M, Cout):
    """The split GEMM has one tile form (128 x 128, three workgroups per CU); a launch of fewer than ~half a round of tiles (the BEV
    FPN's laterals and stride-2 extras, the coarse image laterals) fills the chip better on the 64 x 64 tiles of the f32-MFMA kernels:
    nusc_L, whose GEMMs are all of that size, ran 1.5-2 % slower with everything on the split kernel (same box, alternating runs:
    229.7 / 233.7 against 234.8 / 237.1 frames/s).  SRF_GEMM_SPLIT_MIN overrides the threshold (A/B switch)."""
    if not gemm_split_enabled():
        return False
    thr = int(os.environ.get("SRF_GEMM_SPLIT_MIN", GEMM_SPLIT_MIN_TILES))
    return ((M + 127) // 128) * ((Cout + 127) // 128) >= thr


GEMM_DIRECT_MIN_TILES = 1024   # 128 x 128 tiles of a launch from which the LDS-free kernel wins (tools/micro/gemm_direct_bench.hip)


def conv1x1_direct_wanted(M, Cout):
    """The LDS-free GEMM (`srf_conv1x1_nhwc_direct`) pays on launches of more than a round of 128 x 128 tiles at three workgroups
    per CU (VoVNet stages 2-4: 122-135 against 110-117 TFLOP/s); below that the 64 x 64 tiles of `srf_conv1x1_nhwc` fill the chip
    better (stage 5: 104 against 93).  SRF_GEMM_DIRECT=0 / 1 forces the choice (A/B switch for tests and benchmarks)."""
    force = os.environ.get("SRF_GEMM_DIRECT")
    if force is not None:
        return force != "0"
    return ((M + 127) // 128) * ((Cout + 127) // 128) >= GEMM_DIRECT_MIN_TILES


def conv1x1_nhwc(x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None, pool=False, top=None, packed_direct=None,
                 packed_split=None, packed_bf16=None):
    """1x1 convolution of the NHWC slice x (N, H, W, K) + per-channel scale / shift + ReLU into `out` ((N, H, W, Cout) slice
    of an NHWC buffer; new contiguous tensor when None).  pool=True: returns (out, mean (N, Cout) over the pixels of each
    image) from the same pass (`srf_conv1x1_nhwc_pooled`).  top: an (N, Ht, Wt, Cout) NHWC slice whose nearest-neighbour
    upsampling to (H, W) is added to the result in the epilogue (`srf_conv1x1_nhwc_topdown`: the FPN top-down step).
    packed_direct: the same weight packed by `pack_conv1x1_nhwc_direct_weights`, or a callable returning it; large launches then
    run on the LDS-free kernel (`srf_conv1x1_nhwc_direct*`: the same bits in `out`).  packed_split: the weight packed by
    `pack_conv1x1_nhwc_split_weights` (or a callable): unless SRF_GEMM_SPLIT=0 the layer runs on `srf_conv1x1_nhwc_split*` (f32 GEMM
    on the bf16 MFMA through an exact three-way split; f32-accurate, not the bits of the fma chain).  packed_bf16: the weight packed by
    `pack_conv1x1_nhwc_bf16_weights` (or a callable): the layer runs on `srf_conv1x1_nhwc_bf16*` -- both operands rounded to bf16 once,
    exact products, f32 accumulation and epilogue (csrc/gemm_bf16.hip; reduced precision, the caller's explicit choice; packed_weight
    may then be None).  Tensors beyond the 32-bit ranges of that family keep the f32 route."""
    x_ld = nhwc_ld(x)
    N, H, W, K = x.shape
    if out is None:
        out = _empty((N, H, W, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, H, W, Cout):
        raise ValueError("conv1x1_nhwc: out has the wrong shape")
    y_ld = nhwc_ld(out)
    L = _lib.lib()
    if not gemm_rows_ok(max(x_ld, y_ld)):     # beyond the 128-row descriptors of the direct and the split family
        packed_direct = packed_split = packed_bf16 = None
    kind, k, packed = _choose_gemm("conv1x1_nhwc", "(Cout, K)", N * H * W, Cout, K, packed_weight, packed_direct, packed_split, packed_bf16)
    split, wp = kind == "split", _ptr(packed)
    timing = _dense_timing("gsplit" if kind in ("split", "bf16") else "gemm")
    sc, sh = _opt(scale, "scale"), _opt(shift, "shift")
    mean = None
    if top is not None:
        if pool or top.dim() != 4 or top.shape[0] != N or top.shape[3] != Cout:
            raise ValueError("conv1x1_nhwc: top must be (N, Ht, Wt, Cout) and excludes pool")
        check(getattr(L, k["topdown"])(_ptr(x), N, H, W, K, x_ld, wp, Cout, sc, sh, int(bool(relu)), _ptr(top), top.shape[1], top.shape[2],
                                    nhwc_ld(top), _ptr(out), y_ld, _stream()), "conv1x1_nhwc_topdown")
    elif pool:
        mean = _empty((N, Cout), torch.float32, x.device)
        nbytes = L.srf_conv1x1_nhwc_pooled_workspace_bytes(N, H * W, Cout)
        ws = _empty((max(nbytes, 4) // 4,), torch.float32, x.device)
        check(getattr(L, k["pooled"])(_ptr(x), N, H * W, K, x_ld, wp, Cout, sc, sh, int(bool(relu)), _ptr(out), y_ld, _ptr(mean), _ptr(ws), nbytes,
                                   _stream()), "conv1x1_nhwc_pooled")
    else:
        check(getattr(L, k["plain"])(_ptr(x), N * H * W, K, x_ld, wp, Cout, sc, sh, int(bool(relu)), _ptr(out), y_ld, _stream()), "conv1x1_nhwc")
    if timing is not None:
        fl = 2.0 * K * Cout * N * H * W
        # split: six bf16 products per f32 product are issued on the bf16 MFMA; the weights are 6 bytes each
        _dense_timed(timing[1], timing[0], f"{K}->{Cout} @{N}x{H}x{W}" + k["tag"], fl, 6.0 * fl if split else fl,
                     4.0 * N * H * W * (K + Cout) + (6.0 if split else 2.0 if kind == "bf16" else 4.0) * K * Cout)
    return (out, mean) if pool else out


def conv1x1_nhwc_residual(x, packed_weight, Cout, res, scale=None, shift=None, relu=False, out=None, packed_direct=None, packed_split=None):
    """conv3 of a ResNet bottleneck: out = act(conv1x1(x) * scale + shift + res), the identity `res` ((N, H, W, Cout) NHWC slice, not
    overlapping out) added BEFORE the ReLU, in the GEMM's epilogue (`srf_conv1x1_nhwc_residual` / `_direct_residual` / `_split_residual`).
    The family is chosen exactly as `conv1x1_nhwc` chooses it; bit for bit `conv1x1_nhwc(relu=False)` + res, then the ReLU.  There is
    no bf16-product form."""
    x_ld = nhwc_ld(x)
    N, H, W, K = x.shape
    if out is None:
        out = _empty((N, H, W, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, H, W, Cout):
        raise ValueError("conv1x1_nhwc_residual: out has the wrong shape")
    if tuple(res.shape) != (N, H, W, Cout):
        raise ValueError("conv1x1_nhwc_residual: res must be (N, H, W, Cout)")
    y_ld, res_ld = nhwc_ld(out), nhwc_ld(res)
    if not gemm_rows_ok(max(x_ld, y_ld, res_ld)):     # beyond the 128-row descriptors of the direct and the split family
        packed_direct = packed_split = None
    kind, k, packed = _choose_gemm("conv1x1_nhwc_residual", "(Cout, K)", N * H * W, Cout, K, packed_weight, packed_direct, packed_split)
    split = kind == "split"
    timing = _dense_timing("gsplit" if split else "gemm")
    check(getattr(_lib.lib(), k["residual"])(_ptr(x), N * H * W, K, x_ld, _ptr(packed), Cout, _opt(scale, "scale"), _opt(shift, "shift"),
                                             int(bool(relu)), _ptr(out), y_ld, _ptr(res), res_ld, _stream()), "conv1x1_nhwc_residual")
    if timing is not None:
        fl = 2.0 * K * Cout * N * H * W
        _dense_timed(timing[1], timing[0], f"{K}->{Cout} @{N}x{H}x{W}" + k["tag"] + " +res", fl, 6.0 * fl if split else fl,
                     4.0 * N * H * W * (K + 2 * Cout) + (6.0 if split else 4.0) * K * Cout)
    return out


def nhwc_affine(x, scale=None, shift=None, relu=False, residual=None, out=None):
    """out = x * scale + shift (+ residual), optional ReLU, on NHWC slices.  scale: (C,) or per sample (N, C)."""
    x_ld = nhwc_ld(x)
    N, H, W, C = x.shape
    if out is None:
        out = _empty((N, H, W, C), torch.float32, x.device)
    elif tuple(out.shape) != (N, H, W, C):
        raise ValueError("nhwc_affine: out has another shape")
    if residual is not None and tuple(residual.shape) != (N, H, W, C):
        raise ValueError("nhwc_affine: residual has another shape")
    per_sample = int(scale is not None and scale.dim() == 2) | (2 if (shift is not None and shift.dim() == 2) else 0)
    if scale is not None and scale.numel() != (N * C if per_sample & 1 else C):
        raise ValueError("nhwc_affine: scale has the wrong size")
    if shift is not None and shift.numel() != (N * C if per_sample & 2 else C):
        raise ValueError("nhwc_affine: shift has the wrong size")
    check(_lib.lib().srf_nhwc_affine(_ptr(x), x_ld, N, H * W, C, _opt(scale, "scale"), per_sample, _opt(shift, "shift"),
                                     _ptr(residual),
                                     0 if residual is None else nhwc_ld(residual), int(bool(relu)), _ptr(out), nhwc_ld(out),
                                     _stream()), "nhwc_affine")
    return out


def nhwc_colmean(x):
    """(N, H, W, C) NHWC slice -> (N, C) mean over the pixels."""
    x_ld = nhwc_ld(x)
    N, H, W, C = x.shape
    L = _lib.lib()
    ws = _empty((max(L.srf_nhwc_colmean_workspace_bytes(N, C) // 4, 1),), torch.float32, x.device)
    mean = _empty((N, C), torch.float32, x.device)
    check(L.srf_nhwc_colmean(_ptr(x), x_ld, N, H * W, C, _ptr(mean), _ptr(ws), ws.numel() * 4, _stream()), "nhwc_colmean")
    return mean


def nhwc_colsum_prod(a, b):
    """(N, H, W, C) NHWC slices a, b -> (N, C): the sum over the pixels of a * b (deterministic two-level sum)."""
    a_ld, b_ld = nhwc_ld(a), nhwc_ld(b)
    N, H, W, C = a.shape
    if tuple(b.shape) != (N, H, W, C):
        raise ValueError("nhwc_colsum_prod: shapes differ")
    L = _lib.lib()
    ws = _empty((max(L.srf_nhwc_colmean_workspace_bytes(N, C) // 4, 1),), torch.float32, a.device)
    out = _empty((N, C), torch.float32, a.device)
    check(L.srf_nhwc_colsum_prod(_ptr(a), a_ld, _ptr(b), b_ld, N, H * W, C, _ptr(out), _ptr(ws), ws.numel() * 4, _stream()), "nhwc_colsum_prod")
    return out


def pool3s2_out(h):
    ho = 1 if h < 3 else (h - 3 + 1) // 2 + 1
    return ho - 1 if (ho - 1) * 2 >= h else ho


def pool3s2p1_out(h):
    """Output extent of MaxPool2d(3, stride 2, padding 1) in floor mode: (h + 2 - 3) // 2 + 1 (csrc/nhwc.hip:257)."""
    return (h - 1) // 2 + 1


def nhwc_maxpool3s2_pad1(x, out=None):
    """MaxPool2d(3, stride 2, padding 1), floor mode, on an NHWC slice (`srf_nhwc_maxpool3s2_pad1`): the pool behind a ResNet stem."""
    x_ld = nhwc_ld(x)
    N, H, W, C = x.shape
    Ho, Wo = pool3s2p1_out(H), pool3s2p1_out(W)
    if out is None:
        out = _empty((N, Ho, Wo, C), torch.float32, x.device)
    elif tuple(out.shape) != (N, Ho, Wo, C):
        raise ValueError("nhwc_maxpool3s2_pad1: out has the wrong shape")
    check(_lib.lib().srf_nhwc_maxpool3s2_pad1(_ptr(x), x_ld, N, H, W, C, _ptr(out), nhwc_ld(out), _stream()), "nhwc_maxpool3s2_pad1")
    return out


def nhwc_maxpool3s2_ceil(x, out=None):
    x_ld = nhwc_ld(x)
    N, H, W, C = x.shape
    Ho, Wo = pool3s2_out(H), pool3s2_out(W)
    if out is None:
        out = _empty((N, Ho, Wo, C), torch.float32, x.device)
    elif tuple(out.shape) != (N, Ho, Wo, C):
        raise ValueError("nhwc_maxpool3s2_ceil: out has the wrong shape")
    check(_lib.lib().srf_nhwc_maxpool3s2_ceil(_ptr(x), x_ld, N, H, W, C, _ptr(out), nhwc_ld(out), _stream()), "nhwc_maxpool3s2_ceil")
    return out


def nhwc_upsample_add(lat, top, out=None):
    """lat (N, H, W, C) + nearest-upsampled top (N, Ht, Wt, C); out defaults to lat (in place)."""
    N, H, W, C = lat.shape
    if top.dim() != 4 or top.shape[0] != N or top.shape[3] != C:
        raise ValueError("nhwc_upsample_add: top has another batch size or channel count")
    if out is None:
        out = lat
    elif tuple(out.shape) != (N, H, W, C):
        raise ValueError("nhwc_upsample_add: out has another shape")
    check(_lib.lib().srf_nhwc_upsample_add(_ptr(lat), nhwc_ld(lat), _ptr(top), nhwc_ld(top), N, H, W, top.shape[1], top.shape[2], C,
                                           _ptr(out), nhwc_ld(out), _stream()), "nhwc_upsample_add")
    return out


def nhwc_dwconv3x3s2(x, weight, scale=None, shift=None, relu=False, out=None):
    """Depthwise 3x3 / stride 2 / padding 1 on an NHWC slice; weight (C, 1, 3, 3)."""
    x_ld = nhwc_ld(x)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = _empty((N, Ho, Wo, C), torch.float32, x.device)
    elif tuple(out.shape) != (N, Ho, Wo, C):
        raise ValueError("nhwc_dwconv3x3s2: out has the wrong shape")
    _dw_vectors("nhwc_dwconv3x3s2", C, weight, scale, shift)
    w = _dev(weight.reshape(C, 9), "weight", torch.float32)
    check(_lib.lib().srf_nhwc_dwconv3x3s2(_ptr(x), x_ld, N, H, W, C, _ptr(w), _opt(scale, "scale"), _opt(shift, "shift"),
                                          int(bool(relu)), _ptr(out), nhwc_ld(out), _stream()), "nhwc_dwconv3x3s2")
    return out


def nhwc_dwconv3x3s2_cat(x, weight, scale, shift, relu, side, out):
    """One step of the proposal generator's stair: out (N, Ho, Wo, Cs + C) = cat([side, dwconv(x)], -1) in one launch."""
    x_ld = nhwc_ld(x)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Cs = side.shape[3]
    if tuple(side.shape[:3]) != (N, Ho, Wo) or tuple(out.shape) != (N, Ho, Wo, Cs + C):
        raise ValueError("nhwc_dwconv3x3s2_cat: side / out have the wrong shape")
    _dw_vectors("nhwc_dwconv3x3s2_cat", C, weight, scale, shift)
    w = _dev(weight.reshape(C, 9), "weight", torch.float32)
    check(_lib.lib().srf_nhwc_dwconv3x3s2_cat(_ptr(x), x_ld, N, H, W, C, _ptr(w), _opt(scale, "scale"), _opt(shift, "shift"),
                                              int(bool(relu)), _ptr(out[..., Cs:]), nhwc_ld(out), _ptr(side), nhwc_ld(side), Cs,
                                              _ptr(out), _stream()), "nhwc_dwconv3x3s2_cat")
    return out


def nhwc_affine_relu_bwd(gy, y, scale, relu, gy2=None):
    """Backward of y = relu(z * scale + shift) on NHWC tensors (N, H, W, C): -> gz (N, H, W, C) = masked gy * scale, and the column
    sums (2, C) [sum gu, sum gu * y] (gu = gy where y > 0); one streaming pass + a finish launch (srf_nhwc_affine_relu_bwd).
    gy2: a second gradient of the same output, added to gy on the way in."""
    N, H, W, C = gy.shape
    gy_ld, y_ld = nhwc_ld(gy), nhwc_ld(y)
    if gy2 is not None and tuple(gy2.shape) != tuple(gy.shape):
        raise ValueError("nhwc_affine_relu_bwd: gy2 has another shape")
    if tuple(y.shape) != tuple(gy.shape):
        raise ValueError("nhwc_affine_relu_bwd: y has another shape")
    if scale is not None and scale.numel() != C:
        raise ValueError("nhwc_affine_relu_bwd: scale must have C elements")
    M = N * H * W
    L = _lib.lib()
    gz = _empty((N, H, W, C), torch.float32, gy.device)
    sums = _empty((2, C), torch.float32, gy.device)
    nbytes = L.srf_nhwc_affine_relu_bwd_workspace_bytes(M, C)
    ws = _empty((max(nbytes, 4) // 4,), torch.float32, gy.device)
    sc = None if scale is None else _aligned16(_dev(scale, "scale", torch.float32))
    check(L.srf_nhwc_affine_relu_bwd2(_ptr(gy), gy_ld, _ptr(gy2), 0 if gy2 is None else nhwc_ld(gy2), _ptr(y), y_ld, M, C, _ptr(sc),
                                      int(bool(relu)), _ptr(gz), C, _ptr(sums), _ptr(ws), nbytes, _stream()), "nhwc_affine_relu_bwd")
    return gz, sums


def bn_eval_fold(gamma, beta, mean, var, eps):
    """(3, C): s = gamma / sqrt(var + eps), t0 = beta - mean s, inv = 1 / sqrt(var + eps) of an eval-mode BatchNorm (one launch)."""
    C = gamma.numel()
    if not (beta.numel() == mean.numel() == var.numel() == C):
        raise ValueError("bn_eval_fold: gamma, beta, mean and var must have one length")
    out = _empty((3, C), torch.float32, gamma.device)
    check(_lib.lib().srf_bn_eval_fold(_ptr(_dev(gamma, "gamma", torch.float32)), _ptr(_dev(beta, "beta", torch.float32)),
                                      _ptr(_dev(mean, "mean", torch.float32)), _ptr(_dev(var, "var", torch.float32)), float(eps), C, _ptr(out),
                                      _stream()), "bn_eval_fold")
    return out


def bn_eval_grads(sums, fold, mean):
    """(2, C): d gamma, d beta of an eval-mode BatchNorm from nhwc_affine_relu_bwd's column sums and bn_eval_fold's vectors (one launch)."""
    C = mean.numel()
    if sums.numel() != 2 * C or fold.numel() != 3 * C:
        raise ValueError("bn_eval_grads: sums must be (2, C) and fold (3, C)")
    out = _empty((2, C), torch.float32, sums.device)
    check(_lib.lib().srf_bn_eval_grads(_ptr(sums), _ptr(fold), _ptr(_dev(mean, "mean", torch.float32)), C, _ptr(out), _stream()), "bn_eval_grads")
    return out


def nhwc_pool_sum(x, n_cam=1, size=None, pad_to=4):
    """x (B * n_cam, H, W, C) channels-last -> (B, pad(Ho * Wo)): per output pixel the sum over cameras and channels at its `nearest`
    source pixel (size = (Ho, Wo); None: the map itself); columns past Ho * Wo are zeros (row length rounded up to pad_to)."""
    x_ld = nhwc_ld(x)
    Nimg, H, W, C = x.shape
    if n_cam < 1 or Nimg % n_cam:
        raise ValueError("nhwc_pool_sum: the image count is not a multiple of n_cam")
    B = Nimg // n_cam
    Ho, Wo = (H, W) if size is None else (int(size[0]), int(size[1]))
    out_ld = -(-(Ho * Wo) // pad_to) * pad_to
    out = _empty((B, out_ld), torch.float32, x.device)
    check(_lib.lib().srf_nhwc_pool_sum(_ptr(x), x_ld, B, n_cam, H, W, C, Ho, Wo, _ptr(out), out_ld, _stream()), "nhwc_pool_sum")
    return out


def dpg_mix(wl, wi, boxes_w, feats_w, E, P):
    """expert logits (B, E * P) (+ the camera half's) -> proposal boxes (B, P, D) with sigmoid centres, features (B, P, C)."""
    wl = _dev(wl, "wl", torch.float32)
    wi = _dev(wi, "wi", torch.float32) if wi is not None else None
    boxes_w = _dev(boxes_w, "boxes_w", torch.float32)
    feats_w = _dev(feats_w, "feats_w", torch.float32)
    B, D, C = wl.shape[0], boxes_w.shape[1], feats_w.shape[1]
    if wl.shape[1] != E * P or boxes_w.shape[0] != E * P or feats_w.shape[0] != E * P or (wi is not None and wi.shape != wl.shape):
        raise ValueError("dpg_mix: shapes disagree")
    boxes = _empty((B, P, D), torch.float32, wl.device)
    feats = _empty((B, P, C), torch.float32, wl.device)
    check(_lib.lib().srf_dpg_mix(_ptr(wl), _ptr(wi), B, E, P, _ptr(boxes_w), D, _ptr(feats_w), C, _ptr(boxes), _ptr(feats), _stream()),
          "dpg_mix")
    return boxes, feats


def pack_conv_gemm_weights(weight):
    """(Cout, Cin, kh, kw) -> packed operand of srf_conv_gemm_nhwc: k = (tap, input channel), tap slowest."""
    Cout = weight.shape[0]
    return pack_conv1x1_nhwc_weights(weight.detach().permute(0, 2, 3, 1).reshape(Cout, -1).contiguous())


def pack_conv_gemm_split_weights(weight):
    """(Cout, Cin, kh, kw) -> packed operand of srf_conv_gemm_nhwc_split (bf16 planes): k = (tap, input channel), tap slowest."""
    Cout = weight.shape[0]
    return pack_conv1x1_nhwc_split_weights(weight.detach().permute(0, 2, 3, 1).reshape(Cout, -1).contiguous())


def pack_conv_gemm_bf16_weights(weight):
    """(Cout, Cin, kh, kw) -> packed operand of srf_conv_gemm_nhwc_bf16 (one bf16 plane): k = (tap, input channel), tap slowest."""
    Cout = weight.shape[0]
    return pack_conv1x1_nhwc_bf16_weights(weight.detach().permute(0, 2, 3, 1).reshape(Cout, -1).contiguous())


def conv_gemm_nhwc(x, packed_weight, Cout, ksize, stride, pad, scale=None, shift=None, relu=False, out=None, packed_split=None,
                   packed_bf16=None):
    """Conv2d on an NHWC slice as an implicit-im2col GEMM (the strided 3x3 layers); -> (N, Ho, Wo, Cout).  On the f32 MFMA
    (`srf_conv_gemm_nhwc`, packed_weight) or, when packed_split (from `pack_conv_gemm_split_weights`, or a callable) is given and
    SRF_GEMM_SPLIT is not 0, on the split GEMM (`srf_conv_gemm_nhwc_split`: f32-accurate on the bf16 MFMA).  packed_bf16 (from
    `pack_conv_gemm_bf16_weights`, or a callable): on `srf_conv_gemm_nhwc_bf16` -- operands rounded to bf16 once, f32 accumulation and
    epilogue (reduced precision, the caller's explicit choice; any stride, so the 3x3 / stride 1 layers of the bf16 image mode too)."""
    x_ld = nhwc_ld(x)
    N, H, W, Cin = x.shape
    kh, kw = ksize
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    if out is None:
        out = _empty((N, Ho, Wo, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, Ho, Wo, Cout):
        raise ValueError("conv_gemm_nhwc: out has the wrong shape")
    kind, k, packed_weight = _choose_gemm("conv_gemm_nhwc", "the layer", N * Ho * Wo, Cout, kh * kw * Cin, packed_weight,
                                          packed_split=packed_split, packed_bf16=packed_bf16)
    split, fn = kind == "split", getattr(_lib.lib(), k["conv"])
    # the kernel addresses its whole input through ONE 32-bit buffer descriptor (N H W x_ld 4 < 2^31 bytes): larger batches
    # run in groups of images (VoVNet stem_3 reads 464 x 800 x 64 per camera: 23 images reach the limit -- LC inference at
    # batch 4, the frozen prefix of config 4 at bs >= 4)
    per_img = 4 * H * W * x_ld
    group = N if N * per_img < (1 << 31) else max(1, ((1 << 31) - 1) // per_img)
    sc, sh = _opt(scale, "scale"), _opt(shift, "shift")
    timing = _dense_timing("cgemm")
    for n0 in range(0, max(N, 1), max(group, 1)):
        xs, os_ = x[n0:n0 + group], out[n0:n0 + group]
        check(fn(_ptr(xs), xs.shape[0], H, W, Cin, x_ld, _ptr(packed_weight), Cout, kh, kw, stride, pad, sc, sh,
                 int(bool(relu)), _ptr(os_), nhwc_ld(out), _stream()), "conv_gemm_nhwc")
    if timing is not None:
        fl = 2.0 * kh * kw * Cin * Cout * N * Ho * Wo
        _dense_timed(timing[1], timing[0], f"{Cin}->{Cout} {kh}x{kw}/s{stride} @{N}x{H}x{W}" + k["tag"], fl, 6.0 * fl if split else fl,
                     4.0 * N * (H * W * Cin + Ho * Wo * Cout) + (6.0 if split else 2.0 if kind == "bf16" else 4.0) * kh * kw * Cin * Cout)
    return out


def conv_wgrad_supported(g, x, ksize):
    """Shapes `conv_wgrad_nhwc` takes: (N, H, W, C) channel slices of channels-last f32 buffers, ksize 1 or 3, W >= 32, channel counts
    and pixel pitches multiples of 4, every tensor below 2 GB."""
    try:
        g_ld, x_ld = nhwc_ld(g), nhwc_ld(x)
    except RuntimeError:
        return False
    N, H, W, Cin = x.shape
    Cout = g.shape[3]
    return (ksize in (1, 3) and tuple(g.shape[:3]) == (N, H, W) and W >= 32 and Cin % 4 == 0 and Cout % 4 == 0 and g_ld % 4 == 0
            and x_ld % 4 == 0 and g.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and below_2gb(N * H * W, max(g_ld, x_ld)))


def conv_wgrad_nhwc(g, x, ksize):
    """Weight gradient of a stride-1 Conv2d (ksize 1 / padding 0, or ksize 3 / padding 1) from the channels-last output gradient
    g (N, H, W, Cout) and input x (N, H, W, Cin): -> (Cout, Cin, ksize, ksize), `srf_conv_wgrad_nhwc` (an f32 GEMM over the pixels on
    the bf16 MFMA, exact three-way split of both operands, fixed summation order: deterministic)."""
    if not conv_wgrad_supported(g, x, ksize):
        raise ValueError("conv_wgrad_nhwc: unsupported shapes / layout")
    N, H, W, Cin = x.shape
    Cout = g.shape[3]
    L = _lib.lib()
    nbytes = L.srf_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout, ksize)
    ws = _empty((max(nbytes, 4) // 4,), torch.float32, x.device)
    dW = _empty((Cout, Cin, ksize, ksize), torch.float32, x.device)
    check(L.srf_conv_wgrad_nhwc(_ptr(g), nhwc_ld(g), _ptr(x), nhwc_ld(x), N, H, W, Cin, Cout, ksize, _ptr(ws), nbytes, _ptr(dW), _stream()),
          "conv_wgrad_nhwc")
    return dW


def conv_wgrad_bf16_supported(g, x, ksize):
    """Shapes `conv_wgrad_nhwc_bf16` takes: as `conv_wgrad_supported`, at any map width."""
    try:
        g_ld, x_ld = nhwc_ld(g), nhwc_ld(x)
    except RuntimeError:
        return False
    N, H, W, Cin = x.shape
    Cout = g.shape[3]
    return (ksize in (1, 3) and tuple(g.shape[:3]) == (N, H, W) and N * H * W > 0 and Cin > 0 and Cout > 0 and Cin % 4 == 0 and Cout % 4 == 0
            and g_ld % 4 == 0 and x_ld % 4 == 0 and g.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and below_2gb(N * H * W, max(g_ld, x_ld)))


def conv_wgrad_nhwc_bf16(g, x, ksize):
    """Weight gradient of a stride-1 Conv2d as `conv_wgrad_nhwc`, on one bf16 product per f32 product: `srf_conv_wgrad_nhwc_bf16` (both
    operands rounded to bf16 once, exact products, f32 accumulation, fixed summation order: deterministic; csrc/wgrad_bf16.hip).  Reduced
    precision, the caller's explicit choice."""
    if not conv_wgrad_bf16_supported(g, x, ksize):
        raise ValueError("conv_wgrad_nhwc_bf16: unsupported shapes / layout")
    N, H, W, Cin = x.shape
    Cout = g.shape[3]
    L = _lib.lib()
    nbytes = L.srf_conv_wgrad_bf16_workspace_bytes(N, H, W, Cin, Cout, ksize)
    ws = _empty((max(nbytes, 4) // 4,), torch.float32, x.device)
    dW = _empty((Cout, Cin, ksize, ksize), torch.float32, x.device)
    check(L.srf_conv_wgrad_nhwc_bf16(_ptr(g), nhwc_ld(g), _ptr(x), nhwc_ld(x), N, H, W, Cin, Cout, ksize, _ptr(ws), nbytes, _ptr(dW), _stream()),
          "conv_wgrad_nhwc_bf16")
    return dW


def conv_gemm_nhwc_supported(x):
    """Layout / size limits of srf_conv_gemm_nhwc as `conv_gemm_nhwc` drives it (batches are split, one image must fit)."""
    try:
        ld = nhwc_ld(x)
    except RuntimeError:
        return False
    return gemm_k_ok(x.shape[3]) and operand_ok(ld, x.data_ptr()) and below_2gb(x.shape[1] * x.shape[2], ld)


# ---- modulated deformable convolution, DCNv2 (csrc/dcn.hip) ------------------------------------------------------------
def dcn_enabled():
    """SRF_DCN=0 keeps `compat.dcn.ModulatedDeformConv2dPack` on its torch route (one grid_sample, mask multiply, 1x1 conv2d and add per
    kernel tap) on the GPU as well: the parity reference the tests and tools/bench_dcn.py alternate against, the role SRF_GEMM_SPLIT=0
    has for the split GEMM.  Read at every call."""
    return os.environ.get("SRF_DCN", "1") != "0"


def dcnv2_out_size(H, W, ksize, stride=1, padding=0, dilation=1):
    kh, kw = (ksize, ksize) if isinstance(ksize, int) else ksize
    return (H + 2 * padding - dilation * (kh - 1) - 1) // stride + 1, (W + 2 * padding - dilation * (kw - 1) - 1) // stride + 1


def dcnv2_supported(N, C, H, W, groups=1, deform_groups=1, x_ld=None):
    """Shapes `srf_dcnv2_nhwc` takes, from the shape alone: an (N, C, H, W) input (logical shape; x_ld = floats per pixel of the
    channels-last buffer, C when None) with convolution groups == 1, C divisible by deform_groups into groups of a multiple of 32
    channels, H >= 2 and W >= 2 (on a one-row or one-column map compat/dcn.py's normalised grid collapses every position), x_ld % 4 == 0
    and the whole input below 2 GiB."""
    ld = C if x_ld is None else x_ld
    return (groups == 1 and deform_groups >= 1 and C > 0 and C % deform_groups == 0 and (C // deform_groups) % 32 == 0 and H >= 2 and W >= 2
            and N >= 0 and ld >= C and ld % 4 == 0 and 4 * N * H * W * ld < (1 << 31))


def dcnv2_nhwc(x, offset, mask, packed_weight, Cout, ksize, stride=1, pad=0, dilation=1, deform_groups=1, mask_is_logit=False,
               scale=None, shift=None, relu=False, out=None):
    """DCNv2 forward on an NHWC slice (`srf_dcnv2_nhwc`): x (N, H, W, Cin); offset (N, Ho, Wo, 2 K G) and mask (N, Ho, Wo, K G) NHWC slices
    (both may be views of one (N, Ho, Wo, 3 K G) `conv_offset` output); packed_weight from `pack_conv_gemm_weights`; -> (N, Ho, Wo, Cout).
    mask_is_logit: the kernel applies the sigmoid.  scale / shift / relu: the epilogue of `conv_gemm_nhwc` (fold a bias into shift).
    No host synchronisation, no allocation outside torch's allocator: capturable in a hipGraph."""
    x_ld = nhwc_ld(x)
    N, H, W, Cin = x.shape
    kh, kw = ksize
    K, G = kh * kw, int(deform_groups)
    Ho, Wo = dcnv2_out_size(H, W, ksize, stride, pad, dilation)
    off_ld, mask_ld = nhwc_ld(offset), nhwc_ld(mask)
    if tuple(offset.shape) != (N, Ho, Wo, 2 * K * G) or tuple(mask.shape) != (N, Ho, Wo, K * G):
        raise ValueError(f"dcnv2_nhwc: offset / mask must be (N, Ho, Wo, 2 K G) / (N, Ho, Wo, K G) = {(N, Ho, Wo, 2 * K * G)} / "
                         f"{(N, Ho, Wo, K * G)}, got {tuple(offset.shape)} / {tuple(mask.shape)}")
    if out is None:
        out = _empty((N, Ho, Wo, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, Ho, Wo, Cout):
        raise ValueError("dcnv2_nhwc: out has the wrong shape")
    L = _lib.lib()
    if callable(packed_weight):
        packed_weight = packed_weight()
    if packed_weight.numel() * 4 != L.srf_conv1x1_nhwc_packed_weight_bytes(Cout, K * Cin):
        raise ValueError("dcnv2_nhwc: packed weight does not match the layer")
    timing = _dense_timing("dcn")
    check(L.srf_dcnv2_nhwc(_ptr(x), N, H, W, Cin, x_ld, _ptr(offset), off_ld, _ptr(mask), mask_ld, int(bool(mask_is_logit)),
                           _ptr(packed_weight), Cout, kh, kw, stride, pad, dilation, 1, G, _opt(scale, "scale"), _opt(shift, "shift"),
                           int(bool(relu)), _ptr(out), nhwc_ld(out), _stream()), "dcnv2_nhwc")
    if timing is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        M = N * Ho * Wo
        fl = 2.0 * K * Cin * Cout * M + 8.0 * K * Cin * M     # the GEMM + the blend (4 multiply-adds per gathered element)
        timing[1].append((timing[0], ev1, f"dcn {Cin}->{Cout} {kh}x{kw}/s{stride}/d{dilation}/g{G} @{N}x{H}x{W}", fl, fl,
                          4.0 * (N * H * W * Cin + M * (Cout + 3 * K * G)) + 4.0 * K * Cin * Cout))
    return out


def modulated_deform_conv2d(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
    """mmcv's functional `modulated_deform_conv2d` on NCHW tensors: x (N, C, H, W), offset (N, 2 K G, Ho, Wo) interleaved (dy, dx) per
    tap and deformable group, mask (N, K G, Ho, Wo) used as given, weight (Cout, C, kh, kw) -> (N, Cout, Ho, Wo) NCHW-contiguous.
    Converts the layouts, packs the weight and calls `srf_dcnv2_nhwc`; raises on CPU tensors and on shapes the kernel does not take
    (`dcnv2_supported`).  Forward only."""
    x = _dev(x, "x", torch.float32)
    offset, mask = _dev(offset, "offset", torch.float32), _dev(mask, "mask", torch.float32)
    weight = _dev(weight, "weight", torch.float32)
    stride, padding, dilation = (v if isinstance(v, int) else v[0] for v in (stride, padding, dilation))
    N, C, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    if not dcnv2_supported(N, C, H, W, groups, deform_groups) or Cg != C:
        raise RuntimeError(f"srfdet3d_amd: modulated_deform_conv2d does not take x {tuple(x.shape)}, weight {tuple(weight.shape)}, "
                           f"groups {groups}, deform_groups {deform_groups} (see ops.dcnv2_supported)")
    xh = to_channels_last(x).permute(0, 2, 3, 1)
    oh = offset.permute(0, 2, 3, 1).contiguous()
    mh = mask.permute(0, 2, 3, 1).contiguous()
    y = dcnv2_nhwc(xh, oh, mh, pack_conv_gemm_weights(weight), Cout, (kh, kw), stride, padding, dilation, deform_groups, False,
                   None, None if bias is None else _dev(bias, "bias", torch.float32), False)
    return y.permute(0, 3, 1, 2).contiguous()


# ---- multi-scale deformable attention (csrc/msda.hip) ------------------------------------------------------------------
def msda_enabled():
    """SRF_MSDA=0 keeps `compat.transformer.MultiScaleDeformableAttention` (and the encoder around it) on its torch route (one
    grid_sample per level) on the GPU as well: the parity reference the tests and tools/bench_msda.py alternate against, as SRF_DCN=0 is
    for the DCNv2 kernel.  Read at every call."""
    return os.environ.get("SRF_MSDA", "1") != "0"


def msda_supported(B, S, Q, heads, head_dim, levels, points, value_ld=None, offs_ld=None, logits_ld=None, out_ld=None, more=()):
    """Shapes `srf_msda_fwd` takes, from the shapes alone: head_dim 16 or 32, 1 <= levels <= 4, 1 <= points <= 4, every pitch (floats per
    row; the row's width when None) at least the row's width and a multiple of 4, and each of value (B S rows), offs, logits, out and
    ref (B Q rows) below 2 GiB.  `more`: (pitch, width, rows) of further tensors held to the same rule (the gradients of
    `srf_msda_bwd`).  The 16-byte alignment of the bases is checked at the call."""
    if not (B >= 0 and S > 0 and Q >= 0 and heads > 0 and head_dim in (16, 32) and 1 <= levels <= 4 and 1 <= points <= 4):
        return False
    C, ns = heads * head_dim, heads * levels * points
    lds = ((C if value_ld is None else value_ld, C, B * S), (2 * ns if offs_ld is None else offs_ld, 2 * ns, B * Q),
           (ns if logits_ld is None else logits_ld, ns, B * Q), (C if out_ld is None else out_ld, C, B * Q), *more)
    if any(ld < width or ld % 4 for ld, width, _ in lds):
        return False
    lim = (1 << 31) // 4 - 1
    return S < (1 << 31) and all(rows <= lim // ld for ld, _, rows in lds) and B * Q <= lim // (2 * levels)


def _rows(t, name, width):
    """A 2-d float32 GPU tensor (or view) with unit inner stride and `width` columns -> its row pitch."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"srfdet3d_amd: `{name}` must be a GPU tensor (no CPU fallback exists)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"msda: `{name}` must be float32 rows of {width} columns with unit inner stride, got {tuple(t.shape)} "
                         f"strides {tuple(t.stride())} {t.dtype}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), width)


def _msda_inputs(value, shapes, ref, offs, logits, heads, points):
    """The checks `msda` and `msda_backward` share -> (shapes flattened for the ABI, ref, (B, S, Q, rows, C, d, L, P, ns),
    (value_ld, offs_ld, logits_ld))."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    L, P, heads = len(shapes), int(points), int(heads)
    S = sum(h * w for h, w in shapes)
    for t, name in ((value, "value"), (ref, "ref"), (offs, "offs"), (logits, "logits")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"srfdet3d_amd: `{name}` must be a GPU tensor (no CPU fallback exists)")
    if value.dim() != 2 or heads <= 0 or value.shape[1] % heads or S <= 0 or value.shape[0] % S:
        raise ValueError(f"msda: value {tuple(value.shape)} is not (B S, heads d) rows for S = {S}, heads = {heads}")
    C = value.shape[1]
    d, B = C // heads, value.shape[0] // S
    rows = offs.shape[0]
    ns = heads * L * P
    value_ld, offs_ld, logits_ld = _rows(value, "value", C), _rows(offs, "offs", 2 * ns), _rows(logits, "logits", ns)
    ref = _dev(ref, "ref", torch.float32)
    if tuple(ref.shape) != (rows, L, 2) or logits.shape[0] != rows or (B and rows % B) or (B == 0 and rows):
        raise ValueError(f"msda: ref {tuple(ref.shape)} / logits {tuple(logits.shape)} do not match {rows} query rows, {L} levels, B = {B}")
    Q = rows // B if B else 0
    return [v for hw in shapes for v in hw], ref, (B, S, Q, rows, C, d, L, P, ns), (value_ld, offs_ld, logits_ld)


def msda(value, shapes, ref, offs, logits, heads, points, out=None):
    """Multi-scale deformable attention forward (`srf_msda_fwd`, definition in include/srfdet3d.h).  value (B S, heads d) rows of the
    flattened channels-last pyramid, shapes [(H_l, W_l)] host list, ref (B Q, L, 2) normalised (x, y), offs (B Q, heads L P 2) pixel
    offsets, logits (B Q, heads L P) raw; value, offs, logits and out may be column slices of wider row buffers (offs and logits of one).
    -> out (B Q, heads d).  B is B S / S.  No host synchronisation, no allocation outside torch's allocator: capturable."""
    flat, ref, (B, S, Q, rows, C, d, L, P, ns), (value_ld, offs_ld, logits_ld) = _msda_inputs(value, shapes, ref, offs, logits, heads, points)
    if out is None:
        out = _empty((rows, C), torch.float32, value.device)
    out_ld = _rows(out, "out", C)
    if out.shape[0] != rows:
        raise ValueError("msda: out has the wrong number of rows")
    if not msda_supported(B, S, Q, heads, d, L, P, value_ld, offs_ld, logits_ld, out_ld):
        raise RuntimeError(f"srfdet3d_amd: msda does not take B {B}, S {S}, Q {Q}, heads {heads}, head_dim {d}, levels {L}, points {P}, "
                           f"pitches {(value_ld, offs_ld, logits_ld, out_ld)} (see ops.msda_supported)")
    check(_lib.lib().srf_msda_fwd(_ptr(value), value_ld, B, hi(flat), L, _ptr(ref), _ptr(offs), offs_ld, _ptr(logits), logits_ld, Q, heads, d,
                                  P, _ptr(out), out_ld, _stream()), "msda_fwd")
    return out


def msda_train_enabled():
    """Whether `compat.transformer.MultiScaleDeformableAttention` trains through `_MsdaFn` (srf_msda_fwd / srf_msda_bwd) where it can.
    SRF_MSDA_TRAIN=0 keeps training on the torch core; SRF_MSDA=0 does so as well.  Read at every call."""
    return msda_enabled() and os.environ.get("SRF_MSDA_TRAIN", "1") != "0"


def msda_backward(value, shapes, ref, offs, logits, heads, points, grad_out, need=(True, True, True), out=(None, None, None)):
    """Gradient of `msda` (`srf_msda_bwd`, definition in include/srfdet3d.h): the forward's inputs and grad_out (B Q, heads d) ->
    (d_value (B S, heads d), d_offs (B Q, heads L P 2), d_logits (B Q, heads L P)); an entry of `need` that is False skips that gradient
    and returns None in its place.  There is no gradient for ref.  `out` may hold caller-owned row buffers (or column slices of wider
    ones; d_offs and d_logits of one) for the three gradients: the kernel ADDS into d_value, so a caller who passes one zeroes it;
    d_value allocated here is zeroed here.  d_offs and d_logits are bit-reproducible, d_value is summed by float atomics.  The same
    domain as `msda` (ops.msda_supported).  No host synchronisation."""
    flat, ref, (B, S, Q, rows, C, d, L, P, ns), (value_ld, offs_ld, logits_ld) = _msda_inputs(value, shapes, ref, offs, logits, heads, points)
    if not isinstance(grad_out, torch.Tensor) or not grad_out.is_cuda:
        raise RuntimeError("srfdet3d_amd: `grad_out` must be a GPU tensor (no CPU fallback exists)")
    gout_ld = _rows(grad_out, "grad_out", C)
    if grad_out.shape[0] != rows:
        raise ValueError("msda_backward: grad_out has the wrong number of rows")
    bufs, lds, given = [], [], []
    for want, buf, name, nrows, width, zero in zip(need, out, ("d_value", "d_offs", "d_logits"), (B * S, rows, rows), (C, 2 * ns, ns),
                                                   (True, False, False)):
        if not want:
            buf = None
        elif buf is None:
            buf = (torch.zeros if zero else torch.empty)((nrows, width), dtype=torch.float32, device=value.device)
        elif buf.shape[0] != nrows:
            raise ValueError(f"msda_backward: {name} has the wrong number of rows")
        bufs.append(buf)
        lds.append(width if buf is None else _rows(buf, name, width))
        if buf is not None:
            given.append((lds[-1], width, nrows))
    if not msda_supported(B, S, Q, heads, d, L, P, value_ld, offs_ld, logits_ld, gout_ld, more=given):
        raise RuntimeError(f"srfdet3d_amd: msda_backward does not take B {B}, S {S}, Q {Q}, heads {heads}, head_dim {d}, levels {L}, "
                           f"points {P}, pitches {(value_ld, offs_ld, logits_ld, gout_ld, *lds)} (see ops.msda_supported)")
    check(_lib.lib().srf_msda_bwd(_ptr(value), value_ld, B, hi(flat), L, _ptr(ref), _ptr(offs), offs_ld, _ptr(logits), logits_ld, Q, heads, d,
                                  P, _ptr(grad_out), gout_ld, _ptr(bufs[0]), lds[0], _ptr(bufs[1]), lds[1], _ptr(bufs[2]), lds[2],
                                  _stream()), "msda_bwd")
    return tuple(bufs)


class _MsdaFn(torch.autograd.Function):
    """`msda` with its gradient (`msda_backward`) for value, offs and logits; ref carries none.  Only the four inputs are saved: the
    softmax and the sample positions are recomputed in the backward kernel."""

    @staticmethod
    def forward(ctx, value, ref, offs, logits, shapes, heads, points):
        out = msda(value, shapes, ref, offs, logits, heads, points)
        ctx.save_for_backward(value, ref, offs, logits)
        ctx.cfg = (shapes, heads, points)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        value, ref, offs, logits = ctx.saved_tensors
        shapes, heads, points = ctx.cfg
        if grad_out.stride(-1) != 1 or (grad_out.shape[0] > 1 and grad_out.stride(0) % 4) or grad_out.data_ptr() % 16:
            grad_out = grad_out.clone(memory_format=torch.contiguous_format)
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        d_value, d_offs, d_logits = msda_backward(value, shapes, ref, offs, logits, heads, points, grad_out, need)
        return d_value, None, d_offs, d_logits, None, None, None


def msda_autograd(value, shapes, ref, offs, logits, heads, points):
    """`msda` under torch.autograd: gradients for value, offs and logits through `srf_msda_bwd`."""
    return _MsdaFn.apply(value, ref.detach(), offs, logits, [(int(h), int(w)) for h, w in shapes], int(heads), int(points))


def stem_conv_nchw(x, weight, scale=None, shift=None, relu=False, out=None):
    """Conv2d(Cin <= 4, 64, 3, stride 2, padding 1) + affine + ReLU from contiguous NCHW images to an NHWC tensor."""
    x = _dev(x, "x", torch.float32)
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = _empty((N, Ho, Wo, Cout), torch.float32, x.device)
    check(_lib.lib().srf_stem_conv_nchw(_ptr(x), N, Cin, H, W, _ptr(_dev(weight.detach(), "weight", torch.float32)), Cout,
                                        _opt(scale, "scale"), _opt(shift, "shift"), int(bool(relu)), _ptr(out), nhwc_ld(out),
                                        _stream()), "stem_conv_nchw")
    return out


def stem_conv7_nchw(x, weight, scale=None, shift=None, relu=False, out=None):
    """Conv2d(Cin <= 4, 64, 7, stride 2, padding 3) + affine + ReLU from contiguous NCHW images to an NHWC tensor (`srf_stem_conv7_nchw`:
    the stem of a ResNet image backbone)."""
    x = _dev(x, "x", torch.float32)
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if tuple(weight.shape[1:]) != (Cin, 7, 7):
        raise ValueError("stem_conv7_nchw: weight must be (Cout, Cin, 7, 7)")
    if out is None:
        out = _empty((N, Ho, Wo, Cout), torch.float32, x.device)
    elif tuple(out.shape) != (N, Ho, Wo, Cout):
        raise ValueError("stem_conv7_nchw: out has the wrong shape")
    check(_lib.lib().srf_stem_conv7_nchw(_ptr(x), N, Cin, H, W, _ptr(_dev(weight.detach(), "weight", torch.float32)), Cout,
                                         _opt(scale, "scale"), _opt(shift, "shift"), int(bool(relu)), _ptr(out), nhwc_ld(out),
                                         _stream()), "stem_conv7_nchw")
    return out


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def stage_tail(obj, ffn, norm3, cls_layers, reg_layers, logits_fc, deltas_fc, boxes, weights6, pc_range, scale_clamp, split_ffn=True):
    """FFN + residual + norm3, both towers, class_logits, bboxes_delta and apply_deltas: the FFN as one workgroup per (32 rows,
    128 hidden units), everything after it in one launch per 32 rows (split_ffn=False: the FFN in line, a single launch).
    ffn = (linear1, linear2); cls_layers / reg_layers = [(Linear(bias=False), LayerNorm), ...].
    Returns obj_out (R,C), logits (R,ncls), pred (R,Dd)."""
    obj = _dev(obj, "obj", torch.float32)
    boxes = _dev(boxes, "boxes", torch.float32)
    R, C = obj.shape
    lin1, lin2 = ffn
    F = lin1.weight.shape[0]
    ncls, Dd = logits_fc.weight.shape[0], deltas_fc.weight.shape[0]
    if boxes.shape != (R, Dd):
        raise ValueError("boxes must be (R, Dd)")
    obj_out = _empty((R, C), torch.float32, obj.device)
    logits = _empty((R, ncls), torch.float32, obj.device)
    pred = _empty((R, Dd), torch.float32, obj.device)
    cw, cg, cb = ([m.weight for m, _ in cls_layers], [n.weight for _, n in cls_layers], [n.bias for _, n in cls_layers])
    rw, rg, rb = ([m.weight for m, _ in reg_layers], [n.weight for _, n in reg_layers], [n.bias for _, n in reg_layers])
    for t in [lin1.weight, lin1.bias, lin2.weight, lin2.bias, norm3.weight, norm3.bias, logits_fc.weight, logits_fc.bias,
              deltas_fc.weight, deltas_fc.bias] + cw + cg + cb + rw + rg + rb:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != obj.device:
            raise ValueError("stage_tail: parameters must be contiguous float32 on the input's device")
    L = _lib.lib()
    ws, ws_bytes = None, 0
    if split_ffn:
        ws_bytes = L.srf_stage_tail_workspace_bytes(R, C, F)
        ws = _empty((max(ws_bytes, 4) // 4,), torch.float32, obj.device)
    check(L.srf_stage_tail(
        _ptr(obj), R, C, F, _ptr(lin1.weight), _ptr(lin1.bias), _ptr(lin2.weight), _ptr(lin2.bias), _ptr(norm3.weight),
        _ptr(norm3.bias), float(norm3.eps), len(cls_layers), _ptr_array(cw), _ptr_array(cg), _ptr_array(cb),
        hf([n.eps for _, n in cls_layers] or [0.0]), len(reg_layers), _ptr_array(rw), _ptr_array(rg), _ptr_array(rb),
        hf([n.eps for _, n in reg_layers] or [0.0]), _ptr(logits_fc.weight), _ptr(logits_fc.bias), ncls, _ptr(deltas_fc.weight),
        _ptr(deltas_fc.bias), Dd, _ptr(boxes), hf(weights6), hf(pc_range), float(scale_clamp), _ptr(obj_out), _ptr(logits),
        _ptr(pred), None if ws is None else _ptr(ws), ws_bytes, _stream()), "stage_tail")
    return obj_out, logits, pred


# ---------------------------------------------------------------------------------------------- training support
class _RoIExtractFn(torch.autograd.Function):
    """roi_extract with a gradient for the feature maps (RoIs carry none, as in mmcv)."""

    @staticmethod
    def forward(ctx, rois, strides, out_size, sampling_ratio, finest_scale, bin_major, *feats):
        out = roi_extract(list(feats), rois, strides, out_size, sampling_ratio, finest_scale, bin_major=bin_major)
        ctx.save_for_backward(rois, *feats)
        ctx.cfg = (strides, out_size, sampling_ratio, finest_scale, bin_major)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rois, *feats = ctx.saved_tensors
        strides, out_size, sampling_ratio, finest_scale, bin_major = ctx.cfg
        grad_out = grad_out.contiguous()
        R, C, nl = rois.shape[0], feats[0].shape[1], len(strides)
        grads = [torch.zeros_like(f) for f in feats]
        fm = (FeatMap * nl)(*[_featmap(f, 1.0 / s) for f, s in zip(feats, strides)])
        gp = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in grads])
        bins = out_size * out_size
        so_c, so_b = (1, C) if bin_major else (bins, 1)
        if deterministic_enabled():   # every map element's adds in a fixed order; a shape the entry refuses raises (no fall-back)
            L = _lib.lib()
            ws_bytes = L.srf_roi_extract_bwd_ordered_workspace_bytes(R, out_size, sampling_ratio)
            ws = _empty((max(ws_bytes, 4) // 4,), torch.float32, grad_out.device)
            check(L.srf_roi_extract_bwd_ordered(fm, gp, nl, C, _ptr(rois), R, out_size, sampling_ratio, float(finest_scale), _ptr(grad_out),
                                                C * bins, so_c, so_b, _ptr(ws), ws_bytes, _stream()),
                  "roi_extract_bwd_ordered (SRF_DETERMINISTIC=1)")
        else:
            check(_lib.lib().srf_roi_extract_bwd(fm, gp, nl, C, _ptr(rois), R, out_size, sampling_ratio, float(finest_scale),
                                                 _ptr(grad_out), C * bins, so_c, so_b, _stream()), "roi_extract_bwd")
        return (None, None, None, None, None, None, *grads)


def deterministic_enabled():
    """SRF_DETERMINISTIC=1: a gradient that would need one of this library's float-atomic kernels takes a fixed-order kernel instead
    (`srf_roi_extract_bwd_ordered`, `srf_spconv_bwd_weight_ordered`) or raises (`srf_msda_bwd`, compat/transformer.py): two passes give
    the same bytes.  Unset or 0: the routes of before.  Independent of torch's own determinism flags.  Read at every call."""
    return os.environ.get("SRF_DETERMINISTIC", "0") == "1"


def roi_extract_autograd(feats, rois, strides, out_size=7, sampling_ratio=2, finest_scale=56.0, bin_major=False):
    feats = [f if f.is_contiguous() or f.is_contiguous(memory_format=torch.channels_last) else f.contiguous() for f in feats]
    return _RoIExtractFn.apply(rois.detach(), list(strides), out_size, sampling_ratio, finest_scale, bin_major, *feats)


def box_iou_rotated(a, b):
    """pairwise rotated BEV IoU: a (n,5), b (m,5) as (cx, cy, w, h, angle) -> (n, m)."""
    a = _dev(a, "a", torch.float32)
    b = _dev(b, "b", torch.float32)
    out = _empty((a.shape[0], b.shape[0]), torch.float32, a.device)
    check(_lib.lib().srf_box_iou_rotated(_ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out), _stream()), "box_iou_rotated")
    return out


# ------------------------------------------------------------------------------------------------------- OTA label assignment
OTA_MAX_P, OTA_MAX_G, OTA_MAX_C, OTA_MAX_PAIRS = 4096, 512, 64, 65535


def ota_enabled():
    """SRF_OTA=0 keeps `plugin.training.OTAssignerSRFDet` on its torch route on the GPU as well: what training ran before csrc/ota.hip, the
    route the tests and tools/bench_ota.py alternate against.  Read at every call."""
    return os.environ.get("SRF_OTA", "1") != "0"


def ota_assign_ok(S, B, P, D, C, Gpad, candidate_topk=1):
    """The shapes `srf_ota_assign` takes (csrc/ota.hip, the SRF_EINVAL and SRF_EUNSUPPORTED lines of the entry point): at most 4096
    predictions (a byte of LDS per row) and 512 padded ground-truth boxes (an int of LDS per column), at most 65535 (stage, sample) pairs,
    boxes of 8 or 10 columns, at most 64 classes, the cost matrix and the logits inside 32-bit byte ranges."""
    return (S >= 1 and B >= 1 and 1 <= P <= OTA_MAX_P and 1 <= Gpad <= OTA_MAX_G and S * B <= OTA_MAX_PAIRS and D in (8, 10)
            and 1 <= C <= OTA_MAX_C and candidate_topk >= 1 and below_2gb(S * B * P, Gpad) and below_2gb(S * B * P, C))


def _ota_inputs(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt):
    pred_boxes = _dev(pred_boxes, "pred_boxes", torch.float32)
    pred_logits = _dev(pred_logits, "pred_logits", torch.float32)
    gt_boxes = _dev(gt_boxes, "gt_boxes", torch.float32)
    gt_labels = _dev(gt_labels, "gt_labels", torch.int32)
    n_gt = _dev(n_gt, "n_gt", torch.int32)
    if pred_boxes.dim() != 4 or pred_logits.dim() != 4 or pred_logits.shape[:3] != pred_boxes.shape[:3]:
        raise ValueError("ota: pred_boxes (S, B, P, D) and pred_logits (S, B, P, C)")
    S, B, P, D = pred_boxes.shape
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 7 or tuple(gt_labels.shape) != tuple(gt_boxes.shape[:2]) or \
            tuple(n_gt.shape) != (B,):
        raise ValueError("ota: gt_boxes (B, Gpad, 7), gt_labels (B, Gpad) and n_gt (B)")
    C, G = pred_logits.shape[3], gt_boxes.shape[1]
    if not ota_assign_ok(S, B, P, D, C, G):
        raise ValueError(f"ota: shape S {S} B {B} P {P} D {D} C {C} Gpad {G} is outside the limits of srf_ota_assign (ops.ota_assign_ok)")
    return pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, (S, B, P, D, C, G)


def ota_assign(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, head_idx, cost_weights, alpha, gamma, eps, center_radius, candidate_topk,
               num_heads):
    """The dynamic-k OTA assignment of S decoder stages x B samples in one call (`srf_ota_assign`; definition in csrc/ota.hip and, as numpy, in
    tests/ota_ref.py).  pred_boxes (S, B, P, 8 | 10) normalised boxes; pred_logits (S, B, P, C); gt_boxes (B, Gpad, 7) gravity-centre
    [x, y, z, dx, dy, dz, yaw], padded; gt_labels (B, Gpad) int32; n_gt (B) int32; head_idx (S) int32; cost_weights the three weights of
    (FocalLossCost, BBox3DL1Cost, IoU3DCost).  -> count (S, B), pred_idx (S, B, P), gt_idx (S, B, P), status (S, B), all int32: the matched
    predictions ascending in the first count slots with the ground truth of each, -1 behind them; status 1 where the repair loop hit its
    cap.  count and status are the two halves of one tensor (`count._base`), so that one copy brings both to the host.  Nothing is read
    back here."""
    pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, (S, B, P, D, C, G) = _ota_inputs(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt)
    head_idx = _dev(head_idx, "head_idx", torch.int32)
    if tuple(head_idx.shape) != (S,) or candidate_topk < 1:
        raise ValueError("ota: head_idx (S) and candidate_topk >= 1")
    dev = pred_boxes.device
    both = _empty((2, S, B), torch.int32, dev)
    count, status = both[0], both[1]
    pred_idx, gt_idx = _empty((S, B, P), torch.int32, dev), _empty((S, B, P), torch.int32, dev)
    L = _lib.lib()
    ws_bytes = L.srf_ota_workspace_bytes(S, B, P, G)
    ws = _empty((max(ws_bytes, 1),), torch.uint8, dev)
    w_cls, w_reg, w_iou = cost_weights
    check(L.srf_ota_assign(_ptr(pred_boxes), _ptr(pred_logits), _ptr(gt_boxes), _ptr(gt_labels), _ptr(n_gt), _ptr(head_idx), S, B, P, D, C, G,
                           w_cls, w_reg, w_iou, alpha, gamma, eps, center_radius, candidate_topk, num_heads, _ptr(count), _ptr(pred_idx),
                           _ptr(gt_idx), _ptr(status), _ptr(ws), ws_bytes, _stream()), "ota_assign")
    return count, pred_idx, gt_idx, status


def ota_cost(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, cost_weights, alpha, gamma, eps, center_radius):
    """The first stage of `ota_assign` alone (`srf_ota_cost`): -> cost, iou (S, B, Gpad, P) f32, g-major as the matching reads them; the
    columns g >= n_gt[b] are not written."""
    pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, (S, B, P, D, C, G) = _ota_inputs(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt)
    cost, iou = _empty((S, B, G, P), torch.float32, pred_boxes.device), _empty((S, B, G, P), torch.float32, pred_boxes.device)
    w_cls, w_reg, w_iou = cost_weights
    check(_lib.lib().srf_ota_cost(_ptr(pred_boxes), _ptr(pred_logits), _ptr(gt_boxes), _ptr(gt_labels), _ptr(n_gt), S, B, P, D, C, G, w_cls, w_reg,
                                  w_iou, alpha, gamma, eps, center_radius, _ptr(cost), _ptr(iou), _stream()), "ota_cost")
    return cost, iou


def ota_match(cost, iou, n_gt, head_idx, candidate_topk, num_heads):
    """The second stage of `ota_assign` alone (`srf_ota_match`) on g-major matrices cost, iou (S, B, Gpad, P) f32.  `cost` is left as it was:
    the kernel works on a copy (it adds to the rows it repairs).  -> count, pred_idx, gt_idx, status as `ota_assign`."""
    cost = _dev(cost, "cost", torch.float32).clone()
    iou = _dev(iou, "iou", torch.float32)
    n_gt, head_idx = _dev(n_gt, "n_gt", torch.int32), _dev(head_idx, "head_idx", torch.int32)
    if cost.dim() != 4 or cost.shape != iou.shape or tuple(n_gt.shape) != (cost.shape[1],) or tuple(head_idx.shape) != (cost.shape[0],):
        raise ValueError("ota_match: cost and iou (S, B, Gpad, P), n_gt (B), head_idx (S)")
    S, B, G, P = cost.shape
    if not ota_assign_ok(S, B, P, 8, 1, G, candidate_topk):
        raise ValueError("ota_match: shape outside the limits of srf_ota_match (ops.ota_assign_ok)")
    dev = cost.device
    both = _empty((2, S, B), torch.int32, dev)
    pred_idx, gt_idx = _empty((S, B, P), torch.int32, dev), _empty((S, B, P), torch.int32, dev)
    L = _lib.lib()
    ws_bytes = L.srf_ota_match_workspace_bytes(S, B, P, G)
    ws = _empty((max(ws_bytes, 1),), torch.uint8, dev)
    check(L.srf_ota_match(_ptr(cost), _ptr(iou), _ptr(n_gt), _ptr(head_idx), S, B, P, G, candidate_topk, num_heads, _ptr(both[0]), _ptr(pred_idx), _ptr(gt_idx), _ptr(both[1]),
                          _ptr(ws), ws_bytes, _stream()), "ota_match")
    return both[0], pred_idx, gt_idx, both[1]


# ------------------------------------------------------------------------------------------------------- decoder losses of a step
SET_LOSS_MAX_P, SET_LOSS_MAX_G, SET_LOSS_MAX_C, SET_LOSS_MAX_PAIRS = 4096, 512, 64, 65535
SET_LOSS_BOX_COLUMNS = ((8, 8, 7), (10, 8, 7), (10, 8, 9), (10, 10, 9))        # (D, Dw, Dg)


def set_loss_enabled():
    """SRF_SET_LOSS=1 sends the focal and L1 losses of `SRFDetHead.loss_ota` through `set_loss` (csrc/setloss.hip).  Off by default: the
    default route's losses are held bit for bit to the torch operators, and another summation order cannot keep those bits.  Read at every
    call."""
    return os.environ.get("SRF_SET_LOSS", "0") == "1"


def set_loss_ok(S, B, P, C, D, Dw, Gpad, Dg, gamma=2.0, alpha=0.25):
    """The arguments `srf_set_loss` takes (csrc/setloss.hip, the SRF_EINVAL and SRF_EUNSUPPORTED lines of the entry point): at most 4096
    predictions, 512 padded ground-truth boxes, 65535 (stage, sample) pairs and 64 classes, the box columns (D, Dw, Dg) one of
    `SET_LOSS_BOX_COLUMNS`, gamma >= 1 and finite, alpha in [0, 1], every tensor inside a 32-bit byte range."""
    return (S >= 1 and B >= 1 and 1 <= P <= SET_LOSS_MAX_P and 1 <= Gpad <= SET_LOSS_MAX_G and S * B <= SET_LOSS_MAX_PAIRS
            and 1 <= C <= SET_LOSS_MAX_C and (D, Dw, Dg) in SET_LOSS_BOX_COLUMNS and 1.0 <= gamma < float("inf") and 0.0 <= alpha <= 1.0
            and below_2gb(S * B * P, C) and below_2gb(S * B * P, D) and below_2gb(B * Gpad, Dg))


def set_loss(pred_logits, pred_boxes, count, pred_idx, gt_idx, gt_boxes, gt_labels, code_weights, num, alpha, gamma, w_cls, w_box):
    """The sigmoid focal loss and the weighted L1 loss of S decoder stages x B samples on the assignment `ota_assign` returned, values and
    gradients in one call (`srf_set_loss`; definition in csrc/setloss.hip and, as numpy, in tests/set_loss_ref.py).  pred_logits (S, B, P, C);
    pred_boxes (S, B, P, 8 | 10); count (S, B), pred_idx / gt_idx (S, B, P) int32; gt_boxes (B, Gpad, 7 | 9) gravity-centre boxes, padded;
    gt_labels (B, Gpad) int32; code_weights (8 | 10) on the device; num: S pairs of host numbers, the divisors of the class and of the box
    loss.  -> loss (S, 2), grad_logits (S, B, P, C), grad_boxes (S, B, P, D), all float32.  Nothing is read back here."""
    pred_logits, pred_boxes = _dev(pred_logits, "pred_logits", torch.float32), _dev(pred_boxes, "pred_boxes", torch.float32)
    count, pred_idx, gt_idx = _dev(count, "count", torch.int32), _dev(pred_idx, "pred_idx", torch.int32), _dev(gt_idx, "gt_idx", torch.int32)
    gt_boxes, gt_labels = _dev(gt_boxes, "gt_boxes", torch.float32), _dev(gt_labels, "gt_labels", torch.int32)
    code_weights = _dev(code_weights, "code_weights", torch.float32)
    if pred_logits.dim() != 4 or pred_boxes.dim() != 4 or pred_logits.shape[:3] != pred_boxes.shape[:3]:
        raise ValueError("set_loss: pred_logits (S, B, P, C) and pred_boxes (S, B, P, D)")
    S, B, P, C = pred_logits.shape
    D, Dw = pred_boxes.shape[3], code_weights.numel()
    if tuple(count.shape) != (S, B) or tuple(pred_idx.shape) != (S, B, P) or tuple(gt_idx.shape) != (S, B, P):
        raise ValueError("set_loss: count (S, B), pred_idx and gt_idx (S, B, P)")
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or tuple(gt_labels.shape) != tuple(gt_boxes.shape[:2]) or code_weights.dim() != 1:
        raise ValueError("set_loss: gt_boxes (B, Gpad, Dg), gt_labels (B, Gpad) and code_weights (Dw)")
    G, Dg = gt_boxes.shape[1], gt_boxes.shape[2]
    num = [float(v) for pair in num for v in pair]
    if len(num) != 2 * S or not all(0.0 < v < float("inf") for v in num):
        raise ValueError("set_loss: num is S pairs of positive finite numbers")
    if not set_loss_ok(S, B, P, C, D, Dw, G, Dg, gamma, alpha):
        raise ValueError(f"set_loss: S {S} B {B} P {P} C {C} D {D} Dw {Dw} Gpad {G} Dg {Dg} gamma {gamma} alpha {alpha} is outside the limits "
                         "of srf_set_loss (ops.set_loss_ok)")
    dev = pred_logits.device
    loss = _empty((S, 2), torch.float32, dev)
    grad_logits, grad_boxes = _empty((S, B, P, C), torch.float32, dev), _empty((S, B, P, D), torch.float32, dev)
    L = _lib.lib()
    ws_bytes = L.srf_set_loss_workspace_bytes(S, B, P, C, D)
    ws = _empty((max(ws_bytes, 1),), torch.uint8, dev)
    check(L.srf_set_loss(_ptr(pred_logits), _ptr(pred_boxes), _ptr(count), _ptr(pred_idx), _ptr(gt_idx), _ptr(gt_boxes), _ptr(gt_labels),
                         _ptr(code_weights), hf(num), S, B, P, C, D, Dw, G, Dg, alpha, gamma, w_cls, w_box, _ptr(loss), _ptr(grad_logits),
                         _ptr(grad_boxes), _ptr(ws), ws_bytes, _stream()), "set_loss")
    return loss, grad_logits, grad_boxes
