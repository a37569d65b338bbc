"""GT-database sampling and object noise, host side (no GPU): ObjectSample / ObjectNoise / DataBaseSampler build from every
reference config dict against a synthetic database, the database filters, BatchSampler's order and remainder quirk, the
object loader, the refused options, the numpy draw order, the host geometry, and the new C entry points' argument checks.
The device half is tests/test_gpu_object_sample.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import objsample_ref as R
from srfdet3d_amd import _lib
from srfdet3d_amd.compat.registry import OBJECTSAMPLERS, PIPELINES
from srfdet3d_amd.plugin import object_sample as OS

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def _decode(o):
    if isinstance(o, dict):
        if set(o) == {"__tuple__"}:
            return tuple(_decode(v) for v in o["__tuple__"])
        return {k: _decode(v) for k, v in o.items()}
    return [_decode(v) for v in o] if isinstance(o, list) else o


def _pipelines():
    with open(os.path.join(HERE, "golden", "reference_pipelines.json")) as f:
        return {k: _decode(v) for k, v in json.load(f).items()}


def _db_for(cfg, root):
    """write a synthetic database matching a db_sampler dict and point the dict at it"""
    loader = cfg.get("points_loader", {})
    load_dim = loader.get("load_dim", 4)
    dim = 9 if "car" in cfg["classes"] else 7
    info_path, data_root = R.write_db(str(root), cfg["classes"], 6, dim, load_dim, pts=(1, 30))
    return dict(cfg, info_path=info_path, data_root=data_root)


def test_the_new_transforms_are_registered():
    assert PIPELINES.get("ObjectSample") is OS.ObjectSample and PIPELINES.get("ObjectNoise") is OS.ObjectNoise
    assert OBJECTSAMPLERS.get("DataBaseSampler") is OS.DataBaseSampler


@pytest.mark.parametrize("name", sorted(_pipelines()))
def test_both_transforms_build_from_every_config(name, tmp_path):
    seen = 0
    for t in _pipelines()[name]["train_pipeline"]:
        if t["type"] == "ObjectSample":
            t = dict(t, db_sampler=_db_for(t["db_sampler"], tmp_path))
            obj = PIPELINES.build(t)
            assert isinstance(obj.db_sampler, OS.DataBaseSampler)
            assert obj.db_sampler.sample_classes == sorted(t["db_sampler"]["sample_groups"])  # the fixture's (sorted) order
            seen += 1
        elif t["type"] == "ObjectNoise":
            obj = PIPELINES.build(t)
            assert obj.num_try == 100 and obj.rot_range == [-0.78539816, 0.78539816]
            seen += 1
    assert seen == {"srfdet_voxel_nusc_L": 1, "srfdet_voxel_kitti_L": 2}.get(name, 0)


def test_nusc_sample_groups_keep_config_order(tmp_path):
    cfg = [t for t in _pipelines()["srfdet_voxel_nusc_L"]["train_pipeline"] if t["type"] == "ObjectSample"][0]
    db = _db_for(dict(cfg["db_sampler"], sample_groups=R.NUSC_GROUPS), tmp_path)
    s = OBJECTSAMPLERS.build(dict(db, type="DataBaseSampler"))
    assert s.sample_classes == list(R.NUSC_GROUPS) and s.sample_max_nums == list(R.NUSC_GROUPS.values())
    assert s.cat2label == {n: i for i, n in enumerate(R.NUSC_CLASSES)}
    assert s.points_loader.load_dim == 5 and s.points_loader.use_dim == [0, 1, 2, 3, 4]
    kitti = [t for t in _pipelines()["srfdet_voxel_kitti_L"]["train_pipeline"] if t["type"] == "ObjectSample"][0]
    k = OBJECTSAMPLERS.build(dict(_db_for(kitti["db_sampler"], tmp_path / "k"), type="DataBaseSampler"))
    assert k.points_loader.load_dim == 4 and k.points_loader.use_dim == [0, 1, 2, 3]  # the default loader


def test_database_filters(tmp_path):
    info_path, root = R.write_db(str(tmp_path), ["a", "b", "c"], 12, 7, 4, seed=3, difficulties=(0, -1, 2), pts=(1, 20))
    s = OS.DataBaseSampler(info_path, root, 1.0, dict(filter_by_difficulty=[-1], filter_by_min_points=dict(a=5, b=0, c=10)),
                           dict(a=1), classes=["a", "b", "c"])
    raw = R.RefSampler(info_path, root, 1.0, {}, dict(a=1), ["a", "b", "c"]).db
    for name, mn in (("a", 5), ("b", 0), ("c", 10)):
        want = [i["path"] for i in raw[name] if i["difficulty"] != -1 and i["num_points_in_gt"] >= mn]
        assert [i["path"] for i in s.db_infos[name]] == want
        assert len(want) < len(raw[name])
    # min points first, then difficulty: the same survivors
    t = OS.DataBaseSampler(info_path, root, 1.0, dict(filter_by_min_points=dict(a=5), filter_by_difficulty=[-1, 2]), dict(a=1),
                           classes=["a", "b", "c"])
    assert [i["path"] for i in t.db_infos["a"]] == [i["path"] for i in raw["a"] if i["difficulty"] not in (-1, 2)
                                                    and i["num_points_in_gt"] >= 5]


@pytest.mark.parametrize("seed", [0, 5, 99])
def test_batch_sampler_order_and_remainder_quirk(seed):
    items = list(range(10))
    np.random.seed(seed)
    bs = OS.BatchSampler(items, "x")
    got = [bs.sample(n) for n in (3, 4, 5, 2, 8, 1, 10)]
    after = np.random.rand()
    np.random.seed(seed)
    idx = np.arange(10)
    np.random.shuffle(idx)
    want, pos = [], 0
    for n in (3, 4, 5, 2, 8, 1, 10):
        if pos + n >= 10:
            want.append(list(idx[pos:]))
            np.random.shuffle(idx)
            pos = 0
        else:
            want.append(list(idx[pos:pos + n]))
            pos += n
    assert got == want
    assert [len(g) for g in got] == [3, 4, 3, 2, 8, 1, 9]  # 7 + 5, 2 + 8 and 1 + 10 reach the end: the remainder only
    assert after == np.random.rand()  # one shuffle at construction, one per reset, nothing else
    np.random.seed(seed)
    OS.BatchSampler(items, "x")
    assert np.array_equal(np.random.get_state()[1], _state_after_shuffles(seed, 1))


def _state_after_shuffles(seed, k):
    np.random.seed(seed)
    for _ in range(k):
        np.random.shuffle(np.arange(10))
    return np.random.get_state()[1].copy()


def test_candidate_draws_follow_sample_groups(tmp_path):
    info_path, root = R.write_db(str(tmp_path), R.NUSC_CLASSES, 9, 9, 5, seed=1)
    prep = dict(filter_by_difficulty=[-1], filter_by_min_points={n: 5 for n in R.NUSC_CLASSES})
    gt_labels = np.array([0, 0, 1, 3, 3, 3, 3, 3, 8, 9, 9, 9], np.int64)
    for seed in range(4):
        np.random.seed(seed)
        s = OS.DataBaseSampler(info_path, root, 1.0, prep, R.NUSC_GROUPS, classes=R.NUSC_CLASSES,
                               points_loader=dict(type="LoadPointsFromFile", load_dim=5, use_dim=[0, 1, 2, 3, 4]))
        got = [s.sample_candidates(gt_labels) for _ in range(3)]
        st = np.random.get_state()[1].copy()
        np.random.seed(seed)
        ref = R.RefSampler(info_path, root, 1.0, prep, R.NUSC_GROUPS, R.NUSC_CLASSES, 5, [0, 1, 2, 3, 4])
        want = [ref.candidates(gt_labels) for _ in range(3)]
        assert np.array_equal(st, np.random.get_state()[1])
        for g, w in zip(got, want):
            assert [n for n, _ in g] == list(R.NUSC_GROUPS)
            assert [[i["path"] for i in lst] for _, lst in g] == [[i["path"] for i in lst] for _, lst in w]
        # car: 2 - 2 GT = 0 drawn; bus: 4 - 5 < 0; traffic_cone: 2 - 3 < 0; truck 3 - 1 = 2
        counts = dict((n, len(lst)) for n, lst in got[0])
        assert counts["car"] == 0 and counts["bus"] == 0 and counts["traffic_cone"] == 0 and counts["truck"] == 2


def test_object_loader_joins_data_root_and_slices(tmp_path):
    info_path, root = R.write_db(str(tmp_path), ["Car"], 3, 7, 6, seed=2)
    s = OS.DataBaseSampler(info_path, root, 1.0, {}, dict(Car=1), classes=["Car"],
                           points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=6, use_dim=[0, 1, 2, 4]))
    info = s.db_infos["Car"][1]
    raw = np.fromfile(os.path.join(root, info["path"]), np.float32).reshape(-1, 6)
    got = s.load_points(info)
    assert got.dtype == np.float32 and np.array_equal(got, raw[:, [0, 1, 2, 4]])
    s3 = OS.DataBaseSampler(info_path, root, 1.0, {}, dict(Car=1), classes=["Car"],
                            points_loader=dict(type="LoadPointsFromFile", load_dim=6, use_dim=3))
    assert np.array_equal(s3.load_points(info), raw[:, :3])
    # a data_root of '' / None leaves the info's path alone
    s0 = OS.DataBaseSampler(info_path, "", 1.0, {}, dict(Car=1), classes=["Car"],
                            points_loader=dict(type="LoadPointsFromFile", load_dim=6, use_dim=3))
    with pytest.raises(FileNotFoundError):
        s0.load_points(info)


def test_refused_options(tmp_path):
    info_path, root = R.write_db(str(tmp_path), ["Car"], 2, 7, 4)
    db = dict(info_path=info_path, data_root=root, rate=1.0, prepare={}, sample_groups=dict(Car=2), classes=["Car"])
    with pytest.raises(NotImplementedError):
        OS.ObjectSample(db, sample_2d=True)
    with pytest.raises(NotImplementedError):
        OS.ObjectSample(db, use_ground_plane=True)
    with pytest.raises(NotImplementedError):
        OS.ObjectSample(dict(db, file_client_args=dict(backend="petrel")))
    for extra in (dict(shift_height=True), dict(use_color=True), dict(file_client_args=dict(backend="memcached"))):
        with pytest.raises(NotImplementedError):
            OS.ObjectSample(dict(db, points_loader=dict(type="LoadPointsFromFile", load_dim=4, use_dim=4, **extra)))
    with pytest.raises(NotImplementedError):
        OS.ObjectNoise(global_rot_range=[-0.1, 0.1])
    OS.ObjectNoise(global_rot_range=[0.0, 0.0009])  # narrower than 1e-3: the noise_per_box path


@pytest.mark.parametrize("n", [0, 1, 17])
def test_object_noise_draw_order(n):
    t = OS.ObjectNoise(translation_std=[1.0, 1.0, 0.5], global_rot_range=[0.0, 0.0], rot_range=[-0.78539816, 0.78539816],
                       num_try=100)
    np.random.seed(n)
    loc, rot = t.draw(n)
    after = np.random.rand()
    np.random.seed(n)
    want_loc = np.random.normal(scale=np.array([1.0, 1.0, 0.5], np.float32), size=[n, 100, 3])
    want_rot = np.random.uniform(-0.78539816, 0.78539816, size=[n, 100])
    np.random.uniform(0.0 - np.zeros((n, 1)), 0.0 - np.zeros((n, 1)), size=[n, 100])
    assert np.array_equal(loc, want_loc) and np.array_equal(rot, want_rot) and loc.dtype == np.float64
    assert after == np.random.rand()


def test_host_geometry_convention():
    """the host planes / corners put a box's corners counter-clockwise by its yaw, bottom-centred"""
    box = np.array([[10.0, -4.0, -1.0, 4.0, 2.0, 1.5, 0.5]], F32)
    c2 = OS.bev_corners(box)[0].astype(np.float64)
    np.testing.assert_allclose(c2, R.corners64(box)[0], atol=1e-5)
    # corner 2 = (+dx/2, +dy/2) turned by +0.5 rad counter-clockwise
    x, y = 2.0 * np.cos(0.5) - 1.0 * np.sin(0.5), 2.0 * np.sin(0.5) + 1.0 * np.cos(0.5)
    np.testing.assert_allclose(c2[2], [10 + x, -4 + y], atol=1e-5)
    rng = np.random.default_rng(0)
    for _ in range(20):
        b = R.random_box(rng, 7)[None]
        q = rng.uniform(-0.7, 0.7, (4000, 3)) * b[0, 3:6]
        q[:, 2] = q[:, 2] + b[0, 5] / 2
        s, c = np.sin(np.float64(b[0, 6])), np.cos(np.float64(b[0, 6]))
        p = np.stack([q[:, 0] * c - q[:, 1] * s + b[0, 0], q[:, 0] * s + q[:, 1] * c + b[0, 1], q[:, 2] + b[0, 2]], -1).astype(F32)
        d = R.face_distance(p, b[0])
        idx = R.np_points_in_boxes(p, OS.box_planes(b))
        assert (idx[d > 1e-3] == 0).all() and (idx[d < -1e-3] == -1).all()
        assert (d > 1e-3).sum() > 500 and (d < -1e-3).sum() > 500


def test_c_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.srf_points_in_boxes(None, -1, 3, None, 0, None, None, None, None) == -1
    assert L.srf_points_in_boxes(None, 10, 3, None, 0, None, None, None, None) == -1   # null points / out
    assert L.srf_points_in_boxes(buf, 10, 2, buf, 1, None, buf, None, None) == -1      # nf < 3
    assert L.srf_points_in_boxes(buf, 10, 3, None, 4, None, buf, None, None) == -1     # null planes
    assert L.srf_points_in_boxes(buf, 10, 3, buf, -1, None, buf, None, None) == -1
    assert L.srf_points_in_boxes(buf, 10, 3, buf, 513, None, buf, None, None) == -3    # above the LDS limit
    assert L.srf_box_collision_matrix(None, -1, None, 3, None, None) == -1
    assert L.srf_box_collision_matrix(None, 2, None, 3, None, None) == -1
    assert L.srf_box_collision_accept(None, -1, None, 2, None, 1, None, None) == -1
    assert L.srf_box_collision_accept(None, 0, None, 2, None, 1, None, None) == -1
    assert L.srf_box_collision_accept(buf, 2, buf, 3, buf, -1, buf, None) == -1
    assert L.srf_box_collision_accept(buf, 2000, buf, 49, buf, 1, buf, None) == -3
    assert L.srf_object_sample_merge_workspace_bytes(-1, 0) == 0 and L.srf_object_sample_merge_workspace_bytes(300000, 900) > 0
    assert L.srf_object_sample_merge(None, -1, 5, None, None, 0, None, None, 0, None, buf, None, None) == -1
    assert L.srf_object_sample_merge(None, 10, 5, None, None, 0, None, None, 0, buf, buf, buf, None) == -1
    assert L.srf_object_sample_merge(buf, 10, 5, buf, None, 4, buf, buf, 1, buf, buf, buf, None) == -1
    assert L.srf_object_sample_merge(buf, 10, 5, buf, buf, 4, buf, buf, 0, buf, buf, buf, None) == -1   # rows, no objects
    assert L.srf_object_sample_merge(buf, 10, 5, buf, buf, 4, buf, buf, 1, buf, None, buf, None) == -1  # no num_out
    assert L.srf_object_noise(None, -1, 4, None, 0, 7, None, None, None, None, None, 1, None, None, None, None) == -1
    assert L.srf_object_noise(buf, 10, 4, buf, 3, 8, buf, buf, buf, buf, buf, 1, buf, buf, buf, None) == -1   # box_dim
    assert L.srf_object_noise(buf, 10, 4, buf, 3, 7, buf, buf, buf, buf, buf, 0, buf, buf, buf, None) == -1   # num_try
    assert L.srf_object_noise(buf, 10, 4, buf, 3, 7, None, buf, buf, buf, buf, 5, buf, buf, buf, None) == -1
    assert L.srf_object_noise(buf, 10, 4, buf, 600, 7, buf, buf, buf, buf, buf, 5, buf, buf, buf, None) == -3
