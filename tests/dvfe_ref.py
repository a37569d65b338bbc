"""The definition of `srf_dvfe_fwd` (csrc/dvfe.hip, file header) in numpy: DynamicVFECustom.forward in eval mode with the cluster centre through
the centroid-aware position encoder, an optional voxel centre, one or two VFE layers and mode="max".

fl = one rounding to float32.  A point with a negative coordinate belongs to no voxel and touches nothing.  The voxels are the distinct
(b, z, y, x) rows in lexicographic order, L(m) the points of voxel m in ascending order (`srf_voxel_unique`).
  cluster mean      mean_d(m) = fl(s_d / fl(|L|)), s_d the float32 sum of coordinate d over L(m) in that order, starting from 0
  voxel centre      c_x(m) = fl(fl(fl(x_idx) * vx) + off_x), likewise y and z (a product and a sum: two roundings, no fma)
  decoration        rel = fl(xyz - mean), cen = fl(xyz - c)
  position encoder  h = tanh((W1 . rel) * scale1 + shift1),  pos = tanh((W2 . h) * scale2 + shift2)
  layer 0           x = [raw features | pos | cen (with voxel_center)],  p0 = relu((Wa . x) * scale_a + shift_a),  v0(m) = max p0 over L(m)
  layer 1           p1 = relu((Wb . [p0 | v0(m)]) * scale_b + shift_b),  out(m) = max p1 over L(m);  one layer: out = v0
  relu              v < 0 ? 0 : v (a NaN stays);   max: start at -inf, take v only if v > acc (a NaN is never taken)
The decoration is float32 with exactly these roundings; everything behind it is float64 on those float32 values.

Beside every value runs a bound e on |float32 kernel - this float64 value| (u = 2^-24, gamma_n = n u / (1 - n u)):
  linear map of K inputs   gamma_{K+1} sum_k |w_k| |x_k|  +  sum_k |w_k| e_k        (K chained fmas in any order; the inputs' own error)
  scale / shift            |scale| e + u |z|                                        (one fma, one rounding)
  tanh                     e + T ulp(tanh z)                                        (1-Lipschitz; T float32 ulps of its value per evaluation)
  relu, max                e, and the largest e of the voxel's points               (1-Lipschitz)
T is the caller's: the accuracy of the tanh the kernel is compared with (tests/test_gpu_dvfe.py measures it)."""
import numpy as np

U32 = 2.0 ** -24   # unit roundoff of float32


def gamma(n, u=U32):
    """n u / (1 - n u): the bound on the relative error of n chained roundings (Higham, Accuracy and Stability, Lemma 3.1)."""
    return n * u / (1.0 - n * u)


def ulp32(v):
    """the float32 spacing at |v|, as float64"""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def voxel_map(coors):
    """(n, 4) int (b, z, y, x) -> voxel_coors (M, 4) sorted, point2voxel (n) with -1 for dropped points, order (points grouped by voxel,
    ascending inside a voxel), offsets (M), counts (M)."""
    coors = np.asarray(coors).astype(np.int64).reshape(-1, 4)
    valid = (coors >= 0).all(axis=1)
    p2v = np.full(len(coors), -1, np.int64)
    if not valid.any():
        z = np.zeros(0, np.int64)
        return np.zeros((0, 4), np.int32), p2v, z, z, z
    vox, inv = np.unique(coors[valid], axis=0, return_inverse=True)
    p2v[valid] = inv.reshape(-1)
    idx = np.nonzero(valid)[0]
    order = idx[np.argsort(p2v[idx], kind="stable")]
    counts = np.bincount(p2v[idx], minlength=len(vox))
    offsets = np.cumsum(counts) - counts
    return vox.astype(np.int32), p2v, order, offsets, counts


def cluster_means(xyz, order, offsets, counts):
    """(M, 3) float32: the sequential float32 sum over each voxel's list, divided by float32(count)."""
    s = np.zeros((len(counts), 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(int(counts.max()) if len(counts) else 0):
            sel = np.nonzero(counts > r)[0]
            s[sel] = (s[sel] + xyz[order[offsets[sel] + r]]).astype(np.float32)
        return (s / counts.astype(np.float32)[:, None]).astype(np.float32)


def centres(voxel_coors, voxel_size, offset):
    """(M, 3) float32 (x, y, z) voxel centres with the two roundings of the definition."""
    v = np.asarray(voxel_size, np.float32)
    o = np.asarray(offset, np.float32)
    idx = np.asarray(voxel_coors)[:, [3, 2, 1]].astype(np.float32)
    prod = (idx * v[None, :]).astype(np.float32)
    return (prod + o[None, :]).astype(np.float32)


def decorate(points, coors, voxel_size, offset):
    """-> the voxel map, rel (k, 3) and cen (k, 3) float32 of the k points that lie in a voxel, and their indices."""
    points = np.asarray(points, np.float32)
    vox, p2v, order, offsets, counts = voxel_map(coors)
    idx = np.nonzero(p2v >= 0)[0]
    xyz = points[:, :3]
    with np.errstate(all="ignore"):
        mean = cluster_means(xyz, order, offsets, counts)
        rel = (xyz[idx] - mean[p2v[idx]]).astype(np.float32)
        cen = (xyz[idx] - centres(vox, voxel_size, offset)[p2v[idx]]).astype(np.float32)
    return (vox, p2v, order, offsets, counts), idx, rel, cen


def _linear(x, e, W):
    W = np.asarray(W, np.float64)
    K = W.shape[1]
    return x @ W.T, gamma(K + 1) * (np.abs(x) @ np.abs(W).T) + e @ np.abs(W).T


def _affine(y, e, scale, shift):
    z = y * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    return z, e * np.abs(np.asarray(scale, np.float64)) + U32 * np.abs(z)


def _tanh(z, e, T):
    v = np.tanh(z)
    return v, e + T * ulp32(v)


def _relu(z):
    return np.where(z < 0, 0.0, z)          # NaN < 0 is False: a NaN stays


def _voxel_max(v, e, p2v, M):
    """max with the kernel's rule (a NaN is never taken, an empty or all-NaN list gives -inf) and the largest bound of the list"""
    out = np.full((M, v.shape[1]), -np.inf)
    np.maximum.at(out, p2v, np.where(np.isnan(v), -np.inf, v))
    eb = np.zeros((M, v.shape[1]))
    np.maximum.at(eb, p2v, np.where(np.isfinite(e), e, 0.0))
    return out, eb


def dvfe(points, coors, voxel_size, offset, voxel_center, pos_enc, layers, T=1.0):
    """-> dict(out (M, C) float64, bound (M, C) float64, coors (M, 4) int32, point2voxel (n), tanh_args float32 (every argument a tanh
    of the position encoder was taken at, rounded to float32))."""
    points = np.asarray(points, np.float32)
    (vox, p2v, order, offsets, counts), idx, rel, cen = decorate(points, coors, voxel_size, offset)
    M, pv = len(vox), p2v[idx]
    W1, s1, h1, W2, s2, h2 = pos_enc
    with np.errstate(all="ignore"):
        y, e = _linear(rel.astype(np.float64), np.zeros(rel.shape), W1)
        z1, e = _affine(y, e, s1, h1)
        h, e = _tanh(z1, e, T)
        y, e = _linear(h, e, W2)
        z2, e = _affine(y, e, s2, h2)
        pos, e = _tanh(z2, e, T)
        parts, errs = [points[idx].astype(np.float64), pos], [np.zeros(points[idx].shape), e]
        if voxel_center:
            parts.append(cen.astype(np.float64))
            errs.append(np.zeros(cen.shape))
        x, e = np.concatenate(parts, 1), np.concatenate(errs, 1)
        for li, (W, scale, shift) in enumerate(layers):
            y, e = _linear(x, e, W)
            z, e = _affine(y, e, scale, shift)
            p = _relu(z)
            out, eb = _voxel_max(p, e, pv, M)
            if li + 1 < len(layers):
                x, e = np.concatenate([p, out[pv]], 1), np.concatenate([e, eb[pv]], 1)
    args = np.concatenate([z1.ravel(), z2.ravel()]).astype(np.float32)
    return dict(out=out, bound=eb, coors=vox, point2voxel=p2v, tanh_args=args)


def encoder_params(enc):
    """(pos_enc, layers) of a `DynamicVFECustom` in eval mode as float32 numpy arrays: the weights, and the BatchNorms folded by
    `derived.fold_bn` -- the very arrays the module hands to `ops.dvfe`."""
    from srfdet3d_amd import derived
    a = lambda t: t.detach().float().cpu().numpy()
    pe = enc.cen2point_pos_enc
    pos_enc = (a(pe[0].weight), *map(a, derived.fold_bn(pe[1])), a(pe[3].weight), *map(a, derived.fold_bn(pe[4])))
    layers = [(a(v.linear.weight), *map(a, derived.fold_bn(v.norm))) for v in enc.vfe_layers]
    return pos_enc, layers


def offsets_of(voxel_size, pc_range):
    """the three offsets as `DynamicVFECustom.__init__` computes them (in double; the kernel gets them rounded to float32)"""
    return [voxel_size[d] / 2 + pc_range[d] for d in range(3)]
