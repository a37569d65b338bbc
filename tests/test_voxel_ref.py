"""tests/voxel_ref.py against brute force, the coordinate rule of the oracle's dynamic scatter, and -- on any machine -- the conditions
that the inputs of tests/test_gpu_voxel_front.py have to meet for their cases to prove anything: the oracle's voxel count on the
max_voxels clamp, a voxel that fills up, a probe chain that wraps, a sum that depends on its order, offending rows whose keys stay
inside the bitmap."""
import numpy as np
import pytest

import test_gpu_voxel_front as F
import voxel_ref as R
from oracle import oracle as O


def test_hash_and_home_slots():
    assert R.hash32(0) == 0 and 0 <= R.hash32(0xFFFFFFFE) < 1 << 32
    assert [R.table_capacity(n) for n in (0, 1, 500, 512, 513, 1024, 1025)] == [1024, 1024, 1024, 1024, 2048, 2048, 4096]
    at_end = [k for k in range(11285) if R.home_slot(k, 1024) == 1023]
    assert at_end == [293, 722, 1014, 4539, 5874, 6242, 6657, 9020]
    assert len({R.hash32(k) for k in range(1 << 12)}) == 1 << 12                     # xor-shifts and odd multipliers: one to one


def test_replay_inserts_counts_wraps():
    slot, wraps = R.replay_inserts([722, 1014, 4539, 722], 1024)
    assert slot == {722: 1023, 1014: 0, 4539: 1} and wraps == 2                      # 1014 and 4539 each step from slot 1023 to slot 0
    slot, wraps = R.replay_inserts(range(100), 1024)
    assert wraps == 0 and len(set(slot.values())) == 100


def test_static_form_and_point_lists():
    v = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    c = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
    num, mean = np.array([3, 1], np.int32), np.ones((2, 2), np.float32)
    sv, sc, sn, sm = R.static_form(v, c, num, mean, 4, 7)
    assert sv.shape == (4, 3, 4) and (sv[:2] == v).all() and (sv[2:] == 0).all() and (sm[2:] == 0).all()
    assert sc.tolist() == [[7, 1, 2, 3], [7, 4, 5, 6], [-1] * 4, [-1] * 4] and sn.tolist() == [3, 1, 0, 0]
    counts, offsets, order = R.point_lists([2, -1, 0, 2, 0, -1, 2], 3)
    assert counts.tolist() == [2, 0, 3] and offsets.tolist() == [0, 2, 2] and order.tolist() == [2, 4, 0, 3, 6]


def test_spatial_order_is_the_sort_by_b_y_x_z():
    idx = np.array(F.distinct_rows((5, 7, 9), 2, 400, 59))
    want = sorted(range(400), key=lambda i: (idx[i, 0], idx[i, 2], idx[i, 3], idx[i, 1]))
    assert R.spatial_order(idx).tolist() == want
    with pytest.raises(AssertionError):
        R.spatial_order(np.concatenate([idx, idx[:1]]))


def test_coordinate_rule_of_the_oracle():
    grid, batch = [3, 5, 7], 2
    rng = np.random.default_rng(5)
    coors = rng.integers(-1, [batch + 1, 4, 6, 8], size=(4000, 4), endpoint=False).astype(np.int32)
    keep = R.drop_outside(coors, grid, batch)
    assert keep.tolist() == [bool(0 <= b < batch and 0 <= z < 3 and 0 <= y < 5 and 0 <= x < 7) for b, z, y, x in coors.tolist()]
    assert 0.1 < keep.mean() < 0.5                                                   # 2/4 * 3/5 * 5/7 * 7/9 of the rows
    f = rng.standard_normal((4000, 3)).astype(np.float32)
    for mode in ("mean", "max"):
        rf, rc, rp = O.dynamic_scatter(f, coors, grid, mode, batch=batch)
        assert np.array_equal(rp >= 0, keep)
        masked = np.where(keep[:, None], coors, -1).astype(np.int32)                  # the same rows marked the old way
        for got, want in zip((rf, rc, rp), O.dynamic_scatter(f, masked, grid, mode)):
            assert got.tobytes() == want.tobytes()
        assert np.array_equal(np.unique(coors[keep], axis=0), rc)                    # lexicographic, distinct
    # without a batch count the oracle is the op as it was: only negative entries drop a row
    old = O.dynamic_scatter(f, coors, grid, "mean")
    assert np.array_equal(old[2] >= 0, (coors >= 0).all(1)) and (old[2] >= 0).sum() > keep.sum()


def test_geometries():
    for name, g in F.GEOM.items():
        assert O.grid_size(g["voxel_size"], g["pc_range"]).tolist() == F.GRID[name]
        for x in g["voxel_size"] + g["pc_range"]:
            assert float(np.float32(x)) == x
    assert int(np.prod(F.GRID["A"])) == 525 and int(np.prod(F.GRID["B"])) == 11285


@pytest.mark.parametrize("nf,max_points,mean_features", F.K1_PARAMS)
def test_inputs_shape_sweep(nf, max_points, mean_features):
    for n in (1, 255, 2049, 8193):
        for max_voxels in (100, 40000):
            pts, (v, c, num) = F.sweep_case(nf, max_points, n, max_voxels)
            assert pts.shape == (n, nf) and v.shape[1:] == (max_points, nf) and 1 <= mean_features <= nf
    assert np.isnan(pts[:, 0]).sum() == 1 and np.isposinf(pts[:, 1]).sum() == 1 and np.isneginf(pts[:, 2]).sum() == 1
    assert num.max() == min(max_points, 5) or num.max() >= 2


def test_inputs_k1_cases():
    for delta in (-1, 0, 1):
        F.clamp_case(F.CLAMP_V + delta)
    for max_points in (1, 10, 64):
        F.heavy_case(max_points)
    F.wrap_case()
    for max_points, max_voxels in ((64, 1), (3, 5)):
        F.one_cell_case(max_points, max_voxels)
    assert len(F.hard_ref("outside", "B", 300, 5, 10, 100)[0]) == 0
    assert len(F.sweep_case(5, 10, 8193, 40000)[1][0]) > 3000 and len(F.sweep_case(5, 10, 1, 100)[1][0]) == 1


def test_inputs_k2_and_filter():
    for geom in ("A", "B"):
        for n in F.K2_N[1:]:
            ref = O.dynamic_voxelize(F.cloud(geom, n, 4), **F.GEOM[geom])
            assert (ref[:, 0] < 0).any() and len({tuple(r) for r in ref[ref[:, 0] >= 0]}) > 50
    for n in F.FILTER_N:
        F.filter_case(n)


def test_inputs_k3_cases():
    F.order_case()
    F.max_case()
    F.heavy_scatter_coors()
    for name in F.OUTSIDE_ROWS:
        F.outside_case(name)
    for name, (grid, batch) in F.K3_GRIDS.items():
        total = int(np.prod(grid)) * batch
        assert -(-total // 32) == {"105": 4, "315": 10, "8192w": 8192, "8224w": 8224}[name]
        for n in F.K3_N:
            coors = F.scatter_coors(name, n)
            assert coors.shape == (n, 4) and coors.dtype == np.int32 and coors.max(0).tolist() <= [batch - 1] + [g - 1 for g in grid]
            if n > 1:
                M = len(O.dynamic_scatter(F.feats(n, 1), coors, grid, "max", batch=batch)[1])
                assert M > 50 and (n != 257 or name not in ("105", "8224w") or 40 < M <= 257 - 37)     # room for the static map's padding
    assert 105 % 32 == 9
