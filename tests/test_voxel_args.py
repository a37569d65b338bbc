"""Return codes of the entry points of csrc/voxelize.hip (K1 hard voxelization, K2 dynamic voxelization) and csrc/scatter.hip (K3 dynamic
scatter) and their host queries.  The library decides every refusal on the host before it enqueues anything, so it answers on a machine
without a GPU.

Every pointer handed in is a made-up address that no kernel may ever see: each call below is the entry point's VALID call (which is never
made) with exactly one thing wrong, and `refusal` will not make a call with nothing wrong.  Every call has n >= 1 (rows >= 1 for the
reduce): the n == 0 paths enqueue a fill of the voxel count."""
import ctypes

import pytest

from srfdet3d_amd import _lib
from srfdet3d_amd._lib import hf, hi

EINVAL, EWORKSPACE = -1, -2
PTR = ctypes.c_void_p(0x10000)       # never dereferenced: not a device address
BIG = 1 << 30                        # a workspace size no check objects to
N, NF, MAX_POINTS, MAX_VOXELS = 1000, 5, 10, 400
VS, RANGE, GRID = [0.5, 0.25, 1.0], [-1.0, -2.0, -1.0, 17.5, 13.25, 4.0], [37, 61, 5]
GRID_ZYX, BATCH = [5, 61, 37], 3
GRID_2_32 = [2048, 2048, 1024]       # 2^32 cells
CELLS_2_32_M1 = [65535, 65537, 1]    # 2^32 - 1 cells: the first count a 32-bit key with an empty value cannot hold
CELLS_2_32_M2 = [2, 2147483647, 1]   # 2^32 - 2 cells: the last one it can

_K1 = ("points n nf vs range grid max_points max_voxels voxels coors num voxel_num mean mean_features",
       dict(points=PTR, n=N, nf=NF, vs=VS, range=RANGE, grid=GRID, max_points=MAX_POINTS, max_voxels=MAX_VOXELS, voxels=PTR, coors=PTR,
            num=PTR, voxel_num=PTR, mean=PTR, mean_features=NF))
# entry point -> (argument names in ABI order without the stream, the valid call)
ENTRIES = {
    "srf_hard_voxelize": (_K1[0] + " workspace workspace_bytes", dict(_K1[1], workspace=PTR, workspace_bytes=BIG)),
    "srf_hard_voxelize_static": (_K1[0] + " batch_index workspace workspace_bytes", dict(_K1[1], batch_index=1, workspace=PTR, workspace_bytes=BIG)),
    "srf_dynamic_voxelize": ("points n nf vs range grid coors", dict(points=PTR, n=N, nf=NF, vs=VS, range=RANGE, grid=GRID, coors=PTR)),
    "srf_voxel_unique": ("coors n grid_zyx batch out_coors point2voxel counts offsets order num_voxels workspace workspace_bytes",
                         dict(coors=PTR, n=N, grid_zyx=GRID_ZYX, batch=BATCH, out_coors=PTR, point2voxel=PTR, counts=PTR, offsets=PTR, order=PTR,
                              num_voxels=PTR, workspace=PTR, workspace_bytes=BIG)),
    "srf_scatter_reduce": ("feats order offsets counts num_voxels rows C mode out",
                           dict(feats=PTR, order=PTR, offsets=PTR, counts=PTR, num_voxels=PTR, rows=N, C=4, mode=0, out=PTR)),
}
HOST_FLOATS, HOST_INTS = ("vs", "range"), ("grid", "grid_zyx")
K1 = ("srf_hard_voxelize", "srf_hard_voxelize_static")


def refusal(entry, **wrong):
    """the code of the valid call of `entry` with `wrong` put in its place"""
    names, valid = ENTRIES[entry]
    kw = dict(valid, **wrong)
    assert set(kw) == set(valid) and any(v is None or v != valid[k] for k, v in wrong.items()), (entry, wrong)
    conv = lambda n, v: v if v is None else hf(v) if n in HOST_FLOATS else hi(v) if n in HOST_INTS else v
    return getattr(_lib.lib(), entry)(*[conv(n, kw[n]) for n in names.split()], None)


def rows(entry):
    """(what is wrong, code) for `entry`: the rows every entry point with that argument shares, then its own"""
    names, valid = ENTRIES[entry]
    names = names.split()
    L = _lib.lib()
    out = [({n: None}, EINVAL) for n in names if (valid[n] is PTR or n in HOST_FLOATS + HOST_INTS) and n != "mean"]
    out += [({n: -1}, EINVAL) for n in ("n", "rows") if n in names]
    if "nf" in names:
        out += [(dict(nf=2), EINVAL), (dict(nf=65), EINVAL), (dict(nf=0), EINVAL)]
        out += [(dict(vs=[0.5, 0.0, 1.0]), EINVAL), (dict(vs=[-0.5, 0.25, 1.0]), EINVAL), (dict(vs=[0.5, 0.25, float("nan")]), EINVAL)]
        out += [(dict(grid=g), EINVAL) for g in ([37, 0, 5], [0, 61, 5], [37, 61, -5], GRID_2_32, CELLS_2_32_M1)]
    if entry in K1:
        out += [(dict(max_points=0), EINVAL), (dict(max_points=65), EINVAL), (dict(max_points=-1), EINVAL)]
        out += [(dict(max_voxels=0), EINVAL), (dict(max_voxels=-1), EINVAL)]
        out += [(dict(mean_features=0), EINVAL), (dict(mean_features=NF + 1), EINVAL), (dict(mean_features=-1), EINVAL)]
        out += [(dict(nf=3, mean_features=4), EINVAL), (dict(nf=64, mean_features=65, max_points=64), EINVAL)]
        need = L.srf_hard_voxelize_workspace_bytes(N, MAX_POINTS)
        assert need > 0
        out += [(dict(workspace_bytes=need - 1), EWORKSPACE), (dict(workspace_bytes=0), EWORKSPACE)]
        # the need grows with n and with max_points: what suffices for one fewer does not suffice
        out += [(dict(n=2 * N, workspace_bytes=need), EWORKSPACE), (dict(max_points=MAX_POINTS + 1, workspace_bytes=need), EWORKSPACE)]
    if entry == "srf_hard_voxelize_static":
        out += [(dict(n=0), EINVAL)]                                     # a fixed-shape result has at least one row
    if entry == "srf_voxel_unique":
        out += [(dict(grid_zyx=g), EINVAL) for g in ([0, 61, 37], [5, -61, 37], [5, 61, 0], GRID_2_32, CELLS_2_32_M1)]
        out += [(dict(batch=0), EINVAL), (dict(batch=-2), EINVAL), (dict(grid_zyx=[2048, 2048, 512], batch=2), EINVAL)]
        need = L.srf_voxel_unique_workspace_bytes(N, hi(GRID_ZYX), BATCH)
        assert need > 0
        out += [(dict(workspace_bytes=need - 1), EWORKSPACE), (dict(workspace_bytes=0), EWORKSPACE)]
    if entry == "srf_scatter_reduce":
        out += [(dict(C=0), EINVAL), (dict(C=-4), EINVAL), (dict(mode=2), EINVAL), (dict(mode=-1), EINVAL)]
    return out


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals(entry):
    table = rows(entry)
    assert len(table) >= 10
    for wrong, code in table:
        assert refusal(entry, **wrong) == code, (entry, wrong)


def test_every_argument_has_n_at_least_one():
    for entry, (_, valid) in ENTRIES.items():
        for wrong, _ in rows(entry):
            kw = dict(valid, **wrong)
            assert kw.get("n", 1) != 0 or entry == "srf_hard_voxelize_static", (entry, wrong)      # the one entry point that refuses n == 0
            assert kw.get("rows", 1) != 0, (entry, wrong)


def test_hard_voxelize_workspace_bytes():
    ws = _lib.lib().srf_hard_voxelize_workspace_bytes
    for n, mp in ((-1, 10), (100, 0), (100, -3), (-5, -5)):
        assert ws(n, mp) == 0, (n, mp)
    ns = [0, 1, 255, 256, 257, 511, 512, 513, 2048, 2049, 8192, 8193, 100000, 1 << 20]
    for mp in (1, 2, 10, 64):
        sizes = [ws(n, mp) for n in ns]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], mp
    for n in (1, 500, 513, 8193):
        sizes = [ws(n, mp) for mp in range(1, 65)]
        assert sizes == sorted(sizes) and len(set(sizes)) == 64, n                 # the lists of every slot: strictly more for each point
    # at least: keys and first-point index of a table of >= 2 n slots, max_points list entries per slot, two ints per point
    for n, mp in ((500, 10), (513, 3), (8193, 64)):
        cap = 1024
        while cap < 2 * n:
            cap *= 2
        assert ws(n, mp) >= cap * 4 * (2 + mp) + 8 * n


def test_voxel_unique_workspace_bytes():
    ws = _lib.lib().srf_voxel_unique_workspace_bytes
    for grid, batch in (([0, 61, 37], 1), ([5, 0, 37], 1), ([5, 61, -1], 1), (GRID_ZYX, 0), (GRID_ZYX, -1), (GRID_2_32, 1), (CELLS_2_32_M1, 1),
                        ([2048, 2048, 512], 2), ([65535, 1, 1], 65537)):
        assert ws(N, hi(grid), batch) == 0, (grid, batch)
    assert ws(N, None, 1) == 0 and ws(-1, hi(GRID_ZYX), BATCH) == 0
    assert ws(N, hi(CELLS_2_32_M2), 1) >= 2 * ((1 << 32) - 2) // 8                 # the largest grid: a bitmap and its prefix words
    for grid, batch in (([3, 5, 7], 1), ([3, 5, 7], 3), ([4, 256, 256], 1), ([4, 256, 257], 1)):
        words = -(-batch * grid[0] * grid[1] * grid[2] // 32)
        sizes = [ws(n, hi(grid), batch) for n in (1, 257, 8192, 8193, 100000)]
        assert sizes == sorted(sizes) and sizes[0] >= 8 * words + 4 and sizes[-1] >= 8 * words + 4 * 100000
