"""Plain numpy restatements around K1 hard voxelization, K2 dynamic voxelization and K3 dynamic scatter that the C oracle does not
have: the fixed-shape (static) form of K1, the point lists of K3, the row order of `ops.spatial_order`, the coordinate rule of
`srf_voxel_unique`, and the hash of the K1 table.  The hash is here only to CHOOSE inputs (keys whose probe chain wraps around the
table); no output is ever judged with it.  No torch, no GPU."""
import numpy as np


# ------------------------------------------------------------------------------------------------ K1, static form
def static_form(voxels, coors, num, mean, rows, batch_index):
    """(voxels, coors zyx, num) of oracle.hard_voxelize and the oracle's vfe_mean -> the `rows` rows srf_hard_voxelize_static writes:
    the live rows first, then padding (zeros, num 0, coordinates -1); coordinates as (batch_index, z, y, x)."""
    M = voxels.shape[0]
    assert M <= rows
    v = np.zeros((rows,) + voxels.shape[1:], np.float32)
    c = np.full((rows, 4), -1, np.int32)
    k = np.zeros((rows,), np.int32)
    m = np.zeros((rows, mean.shape[1]), np.float32)
    v[:M], k[:M], m[:M] = voxels, num, mean
    c[:M, 0] = batch_index
    c[:M, 1:] = coors
    return v, c, k, m


# ------------------------------------------------------------------------------------------------ K3
def drop_outside(coors, grid_zyx, batch):
    """The coordinate rule of srf_voxel_unique: a (b, z, y, x) row is kept iff 0 <= b < batch and 0 <= z, y, x < D, H, W.
    -> bool (n,), True for the rows that are kept."""
    c = np.asarray(coors, np.int64).reshape(-1, 4)
    hi = np.array([batch] + [int(g) for g in grid_zyx], np.int64)
    return ((c >= 0) & (c < hi)).all(1)


def linear_key(coors, grid_zyx):
    """((b * D + z) * H + y) * W + x in exact integers, whatever the row holds"""
    c = np.asarray(coors, np.int64).reshape(-1, 4)
    D, H, W = (int(g) for g in grid_zyx)
    return ((c[:, 0] * D + c[:, 1]) * H + c[:, 2]) * W + c[:, 3]


def point_lists(point2voxel, M):
    """point -> voxel map (-1: dropped) -> counts (M,), offsets (M,), order (kept,): the points of voxel m are
    order[offsets[m] : offsets[m] + counts[m]], ascending."""
    p = np.asarray(point2voxel, np.int64)
    kept = np.nonzero(p >= 0)[0]
    counts = np.bincount(p[kept], minlength=M).astype(np.int32)
    offsets = (np.cumsum(counts) - counts).astype(np.int32)
    order = kept[np.argsort(p[kept], kind="stable")].astype(np.int32)
    return counts, offsets, order


def spatial_order(indices):
    """ops.spatial_order: the stable argsort of DISTINCT (b, z, y, x) rows by (b, y, x, z)"""
    i = np.asarray(indices, np.int64)
    assert len(np.unique(i, axis=0)) == len(i)
    return np.lexsort((i[:, 1], i[:, 3], i[:, 2], i[:, 0])).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the K1 table (input choice only)
def hash32(key):
    """srf_hash32 of csrc/common.hpp"""
    k = int(key) & 0xFFFFFFFF
    k ^= k >> 16
    k = (k * 0x7FEB352D) & 0xFFFFFFFF
    k ^= k >> 15
    k = (k * 0x846CA68B) & 0xFFFFFFFF
    k ^= k >> 16
    return k


def table_capacity(n):
    """srf_hv_capacity of csrc/voxelize.hip: the power of two >= 2 n, at least 1024"""
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    return cap


def home_slot(key, cap):
    return hash32(key) & (cap - 1)


def replay_inserts(keys, cap):
    """Linear probing of `keys` in the order given into an empty table of `cap` slots -> (slot of every distinct key, the number of
    probe steps that went from the last slot to slot 0)."""
    table, slot, wraps = {}, {}, 0
    for k in keys:
        k = int(k)
        if k in slot:
            continue
        h = home_slot(k, cap)
        while h in table:
            wraps += h == cap - 1
            h = (h + 1) & (cap - 1)
        table[h] = k
        slot[k] = h
    return slot, wraps
