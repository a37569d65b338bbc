"""tests/dvfe_ref.py (the definition of `srf_dvfe_fwd`) against naive per-voxel loops, a float64 torch restatement of
`DynamicVFECustom.forward` on the float32 decoration, a float32 run of the same network and the reference's recorded voxel features.  No GPU."""
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import detgen
import dvfe_ref as R
import make_fixtures_r2 as mf2
from srfdet3d_amd.plugin import voxel_encoders

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "extra_r2.npz"))
CASES = [("vfe_kitti", dict(in_channels=4, feat_channels=[4], voxel_size=mf2.KITTI_VOXEL, point_cloud_range=mf2.KITTI_RANGE), 4),
         ("vfe_waymo", dict(in_channels=5, feat_channels=[5, 5], voxel_size=mf2.WAYMO_VOXEL, point_cloud_range=mf2.WAYMO_RANGE), 5)]


def encoder(tag, kw, voxel_center=True):
    enc = voxel_encoders.DynamicVFECustom(with_cluster_center=True, with_voxel_center=voxel_center, with_distance=False,
                                          norm_cfg=dict(type="naiveSyncBN1dCustom", eps=1e-3, momentum=0.01), **kw).eval()
    return detgen.load_det_params(enc, tag + ".")


def case(tag, kw, nf, voxel_center=True, drop=True):
    enc = encoder(tag, kw, voxel_center)
    pts, coors = mf2.vfe_points(tag, kw["point_cloud_range"], kw["voxel_size"], nf)
    if drop:                                    # dropped points in between, as the voxelizer marks them
        coors = coors.copy()
        coors[::7] = -1
    pos_enc, layers = R.encoder_params(enc)
    return enc, pts, coors, pos_enc, layers, R.offsets_of(kw["voxel_size"], kw["point_cloud_range"])


def naive(pts, coors, voxel_size, offset, voxel_center, pos_enc, layers):
    """voxel by voxel, point by point, scalar float32 arithmetic for the decoration and float64 loops behind it"""
    W1, s1, h1, W2, s2, h2 = [np.asarray(a, np.float64) for a in pos_enc]
    keys = sorted({tuple(int(v) for v in c) for c in coors if (c >= 0).all()})
    vs, off = np.asarray(voxel_size, np.float32), np.asarray(offset, np.float32)
    out = []
    for key in keys:
        lst = [i for i in range(len(pts)) if tuple(int(v) for v in coors[i]) == key]
        s = np.zeros(3, np.float32)
        for i in lst:
            for d in range(3):
                s[d] = np.float32(s[d] + pts[i, d])
        mean = [np.float32(s[d] / np.float32(len(lst))) for d in range(3)]
        centre = [np.float32(np.float32(np.float32(key[3 - d]) * vs[d]) + off[d]) for d in range(3)]
        xs = []
        for i in lst:
            rel = np.array([np.float32(pts[i, d] - mean[d]) for d in range(3)], np.float64)
            h = np.tanh((W1 @ rel) * s1 + h1)
            pos = np.tanh((W2 @ h) * s2 + h2)
            x = list(pts[i].astype(np.float64)) + list(pos)
            if voxel_center:
                x += [float(np.float32(pts[i, d] - centre[d])) for d in range(3)]
            xs.append(np.array(x))
        v = None
        for li, (W, sc, sh) in enumerate(layers):
            ps = []
            for x in xs:
                z = (np.asarray(W, np.float64) @ x) * np.asarray(sc, np.float64) + np.asarray(sh, np.float64)
                ps.append(np.where(z < 0, 0.0, z))
            v = np.full(len(ps[0]), -np.inf)
            for p in ps:
                v = np.where(p > v, p, v)
            xs = [np.concatenate([p, v]) for p in ps]
        out.append(v)
    return np.array(keys, np.int32).reshape(-1, 4), np.array(out)


@pytest.mark.parametrize("tag,kw,nf", CASES)
@pytest.mark.parametrize("voxel_center", [True, False])
def test_against_naive_loops(tag, kw, nf, voxel_center):
    _, pts, coors, pos_enc, layers, off = case(tag, kw, nf, voxel_center)
    pts, coors = pts[:150], coors[:150]
    got = R.dvfe(pts, coors, kw["voxel_size"], off, voxel_center, pos_enc, layers)
    keys, want = naive(pts, coors, kw["voxel_size"], off, voxel_center, pos_enc, layers)
    assert np.array_equal(got["coors"], keys) and (got["point2voxel"][::7] == -1).all()
    np.testing.assert_allclose(got["out"], want, rtol=1e-12, atol=1e-13)      # the same float64 sums in another order
    assert (got["bound"] > 0).all() and (got["bound"] < 1e-3).all()      # gamma_41 on coordinates of up to 77 m: some 1e-4


def torch_restatement(enc, pts, coors):
    """`DynamicVFECustom.forward` line by line: the decoration in float32 as the module computes it, the layers in float64, the
    DynamicScatter as tests/golden/make_fixtures_r2.py restates it (`torch.unique` + `scatter_reduce`); the mean is summed point by point."""
    enc = enc.double()
    f, c = torch.from_numpy(pts), torch.from_numpy(coors)
    keep = (c >= 0).all(dim=1)
    f, c = f[keep], c[keep]
    uniq, inv = torch.unique(c.long(), dim=0, sorted=True, return_inverse=True)
    M = uniq.shape[0]
    s, cnt = torch.zeros(M, 3), torch.zeros(M)
    for i in range(f.shape[0]):
        s[inv[i]] += f[i, :3]
        cnt[inv[i]] += 1
    mean = s / cnt[:, None]
    parts = [f.double(), enc.cen2point_pos_enc((f[:, :3] - mean[inv]).double())]
    if enc._with_voxel_center:
        cf = c.type_as(f)
        parts.append(torch.stack([f[:, 0] - (cf[:, 3] * enc.vx + enc.x_offset), f[:, 1] - (cf[:, 2] * enc.vy + enc.y_offset),
                                  f[:, 2] - (cf[:, 1] * enc.vz + enc.z_offset)], dim=1).double())
    x = torch.cat(parts, dim=-1)
    for i, vfe in enumerate(enc.vfe_layers):
        bn = vfe.norm          # DynamicVFELayer; the config's naiveSyncBN1dCustom takes float32 only, in eval mode it is this
        p = F.relu(F.batch_norm(vfe.linear(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
        v = torch.full((M, p.shape[1]), -float("inf"), dtype=p.dtype).scatter_reduce(0, inv[:, None].expand(-1, p.shape[1]), p, "amax")
        if i != enc.num_vfe - 1:
            x = torch.cat([p, v[inv]], dim=1)
    return v.numpy(), uniq.int().numpy()


@pytest.mark.parametrize("tag,kw,nf", CASES)
@pytest.mark.parametrize("voxel_center", [True, False])
def test_against_the_module_restated_in_float64(tag, kw, nf, voxel_center):
    """What differs is the BatchNorm, folded to float32 scale and shift here and applied unfolded in float64 there: two roundings of
    2^-24 on scale and shift, through at most four layers whose weights have rows of absolute sum below 4 -- 1e-5 covers it many times."""
    enc, pts, coors, pos_enc, layers, off = case(tag, kw, nf, voxel_center)
    got = R.dvfe(pts, coors, kw["voxel_size"], off, voxel_center, pos_enc, layers)
    with torch.no_grad():
        want, keys = torch_restatement(enc, pts, coors)
    assert np.array_equal(got["coors"], keys)
    np.testing.assert_allclose(got["out"], want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("tag,kw,nf", CASES)
def test_reference_fixture(tag, kw, nf):
    """The reference's own run of these weights and points (tests/golden/extra_r2.npz), at the tolerance tests/test_gpu_fixtures_r2.py
    holds the GPU route to."""
    _, pts, coors, pos_enc, layers, off = case(tag, kw, nf, drop=False)
    np.testing.assert_array_equal(coors, GOLD[tag + ".coors_in"])
    got = R.dvfe(pts, coors, kw["voxel_size"], off, True, pos_enc, layers)
    np.testing.assert_array_equal(got["coors"], GOLD[tag + ".voxel_coors"])
    np.testing.assert_allclose(got["out"], GOLD[tag + ".voxel_feats"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("tag,kw,nf", CASES)
def test_a_float32_run_stays_inside_the_bound(tag, kw, nf):
    """The same network in float32 numpy (matrix products in whatever order the library takes; scale and shift as one fma: the product
    is exact in float64 and the sum is rounded to float32; tanh taken in float64 and rounded: half an ulp, so T = 1 holds it) must lie
    inside the running bound of the definition."""
    _, pts, coors, pos_enc, layers, off = case(tag, kw, nf)
    ref = R.dvfe(pts, coors, kw["voxel_size"], off, True, pos_enc, layers, T=1.0)
    _, idx, rel, cen = R.decorate(pts, coors, kw["voxel_size"], off)
    pv = ref["point2voxel"][idx]
    f32 = np.float32
    W1, s1, h1, W2, s2, h2 = [np.asarray(a, f32) for a in pos_enc]
    tanh = lambda z: np.tanh(z.astype(np.float64)).astype(f32)
    fma = lambda y, sc, sh: (y.astype(np.float64) * np.asarray(sc, np.float64) + np.asarray(sh, np.float64)).astype(f32)
    h = tanh(fma(rel @ W1.T, s1, h1))
    pos = tanh(fma(h @ W2.T, s2, h2))
    x = np.concatenate([pts[idx], pos, cen], 1).astype(f32)
    for li, (W, sc, sh) in enumerate(layers):
        p = np.maximum(fma(x @ np.asarray(W, f32).T, sc, sh), f32(0))
        v = np.full((len(ref["out"]), p.shape[1]), -np.inf, f32)
        np.maximum.at(v, pv, p)
        x = np.concatenate([p, v[pv]], 1)
    assert v.dtype == f32
    err = np.abs(v.astype(np.float64) - ref["out"])
    assert (err <= ref["bound"]).all()
    assert err.max() > 0                          # and it is a float32 run


def test_sequential_mean_and_two_rounding_centre():
    """The two places where the decoration is pinned: the float32 sum runs in point order, the centre is a product and a sum."""
    rng = np.random.default_rng(3)
    n = 400
    coors = np.stack([np.zeros(n), np.zeros(n), rng.integers(0, 4, n), rng.integers(0, 4, n)], 1).astype(np.int32)
    pts = (70.0 + rng.uniform(0, 0.2, (n, 4))).astype(np.float32)
    (vox, p2v, order, offsets, counts), idx, rel, cen = R.decorate(pts, coors, [0.05, 0.05, 0.1], [0.025, -39.975, -2.95])
    for m in range(len(vox)):
        lst = np.nonzero(p2v == m)[0]
        assert np.array_equal(order[offsets[m]:offsets[m] + counts[m]], lst)
        s = np.float32(0)
        for i in lst:
            s = np.float32(s + pts[i, 0])
        assert rel[idx == lst[0], 0] == np.float32(pts[lst[0], 0] - np.float32(s / np.float32(len(lst))))
    i = np.arange(1408)
    two = R.centres(np.stack([i * 0, i * 0, i * 0, i], 1), [0.05] * 3, [0.025] * 3)[:, 0]
    fused = (i.astype(np.float64) * np.float64(np.float32(0.05)) + np.float64(np.float32(0.025))).astype(np.float32)
    assert (two != fused).any() and np.array_equal(two, (i.astype(np.float32) * np.float32(0.05)).astype(np.float32) + np.float32(0.025))
