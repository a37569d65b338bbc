"""The definition of `srf_pillar_vfe` (csrc/pillar.hip, file header) in numpy: the single-layer, mode="max" pillar feature net.

For pillar r with n = num[r] points (fl = one rounding to float32):
  cluster mean     mean_d = fl(s_d / fl(n)), s_d the float32 sum of coordinate d over the points 0..n-1 in ascending order
  voxel centre     c_x = fl(fl(fl(x_idx) * vx) + off_x), likewise y and z (a product and a sum: two roundings, no fma)
  decorated point  [the nf raw features, xyz replaced by xyz - c when legacy], then xyz - mean, then xyz - c; every difference is one
                   float32 subtraction of the raw coordinate
  point p < n, channel c:  acc = sum_k x_k W[c][k];  v = acc * scale_c + shift_c;  v = v < 0 ? 0 : v  (a NaN stays a NaN)
  out[r][c]        = max over p < n of v and, when n < P, also over relu(shift_c) (the reference zeroes the padded slots BEFORE the linear
                   layer, so they contribute relu(bn(0))); the max propagates NaN
  padding rows     (r >= rows_live, b < 0 or n <= 0) are zeros
The decoration is float32 with exactly these roundings; the linear layer and the epilogue are float64 on those float32 values, so the
kernel's float32 fma chain is held to this within gamma_{K+2} times `magnitude`, the |scale_c| sum_k |x_k w_ck| + |shift_c| of the point
that attains the max."""
import numpy as np

U32 = 2.0 ** -24   # unit roundoff of float32


def gamma(n, u=U32):
    """n u / (1 - n u): the bound on the relative error of n chained roundings (Higham, Accuracy and Stability, Lemma 3.1)."""
    return n * u / (1.0 - n * u)


def centres(coors4, voxel_size, offset):
    """(rows, 3) float32 (x, y, z) voxel centres with the two roundings of the definition."""
    v = np.asarray(voxel_size, np.float32)
    o = np.asarray(offset, np.float32)
    idx = np.asarray(coors4)[:, [3, 2, 1]].astype(np.float32)
    prod = (idx * v[None, :]).astype(np.float32)
    return (prod + o[None, :]).astype(np.float32)


def cluster_means(vox, num):
    """(rows, 3) float32: the sequential float32 sum over the points 0..n-1, divided by float32(n) (rows with n <= 0: zeros)."""
    vox = np.asarray(vox, np.float32)
    num = np.asarray(num)
    rows, P, _ = vox.shape
    s = np.zeros((rows, 3), np.float32)
    for p in range(P):
        s = np.where((p < num)[:, None], (s + vox[:, p, :3]).astype(np.float32), s)
    with np.errstate(all="ignore"):
        mean = (s / np.maximum(num, 1).astype(np.float32)[:, None]).astype(np.float32)
    return mean


def decorate(vox, num, coors4, voxel_size, offset, cluster=True, centre=True, legacy=True):
    """(rows, P, K) float32 decorated points, slots p >= n zeroed (as the reference's mask leaves them)."""
    vox = np.asarray(vox, np.float32)
    num = np.asarray(num)
    parts = [vox.copy()]
    with np.errstate(all="ignore"):
        if cluster:
            parts.append((vox[:, :, :3] - cluster_means(vox, num)[:, None, :]).astype(np.float32))
        if centre:
            fc = (vox[:, :, :3] - centres(coors4, voxel_size, offset)[:, None, :]).astype(np.float32)
            if legacy:
                parts[0][:, :, :3] = fc
            parts.append(fc)
    x = np.concatenate(parts, axis=2)
    live = np.arange(vox.shape[1])[None, :] < num[:, None]
    return np.where(live[:, :, None], x, np.float32(0)).astype(np.float32)


def pillar_vfe(vox, num, coors4, voxel_size, offset, W, scale, shift, cluster=True, centre=True, legacy=True, rows_live=None):
    """-> out (rows, Cout) float64, magnitude (rows, Cout) float64."""
    vox = np.asarray(vox, np.float32)
    num = np.asarray(num).astype(np.int64)
    coors4 = np.asarray(coors4)
    rows, P, _ = vox.shape
    W = np.asarray(W, np.float64)
    scale = np.asarray(scale, np.float64)
    shift = np.asarray(shift, np.float64)
    x = decorate(vox, num, coors4, voxel_size, offset, cluster, centre, legacy).astype(np.float64)
    with np.errstate(all="ignore"):
        acc = np.einsum("rpk,ck->rpc", x, W)
        mag = np.einsum("rpk,ck->rpc", np.abs(x), np.abs(W)) * np.abs(scale) + np.abs(shift)
        v = acc * scale + shift
        v = np.where(v < 0, 0.0, v)                                 # NaN < 0 is False: a NaN stays
        # slot P: the padded slots' relu(bn(0)), present when n < P
        pad = np.broadcast_to(np.where(shift < 0, 0.0, shift), (rows, 1, len(shift)))
        v = np.concatenate([v, pad], axis=1)
        mag = np.concatenate([mag, np.broadcast_to(np.abs(shift), (rows, 1, len(shift)))], axis=1)
        slot = np.arange(P + 1)[None, :]
        use = (slot < num[:, None]) | ((slot == P) & (num[:, None] < P))
        v = np.where(use[:, :, None], v, -np.inf)
        isnan = np.isnan(v)                                          # the first NaN if there is one: the max propagates it
        best = np.where(isnan.any(axis=1), np.argmax(isnan, axis=1), np.argmax(np.where(isnan, -np.inf, v), axis=1))
        out = np.take_along_axis(v, best[:, None, :], axis=1)[:, 0]
        mg = np.take_along_axis(mag, best[:, None, :], axis=1)[:, 0]
    pad_row = (num <= 0) | (coors4[:, 0] < 0)
    if rows_live is not None:
        pad_row |= np.arange(rows) >= int(rows_live)
    out = np.where(pad_row[:, None], 0.0, out)
    mg = np.where(pad_row[:, None], 0.0, mg)
    return out, mg
