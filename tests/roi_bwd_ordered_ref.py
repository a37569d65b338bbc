"""numpy float32 definition of `srf_roi_extract_bwd_ordered` (csrc/roi_bwd_ordered.hip), operation by operation: the gradient of the
multi-level RoIAlign gather w.r.t. its maps with the adds of every map element in a fixed order.  No project kernel, no C oracle.

A record is (RoI r, output row ph, column pw, sample iy, ix, tap t); the taps are ordered (y_low, x_low), (y_low, x_high),
(y_high, x_low), (y_high, x_high); a record's slot is its index in C order over (r, ph, pw, iy, ix, t).  Level (`roi_ref.levels`),
sample point, validity and weights are float32 as `srf_roi_extract_bwd_k` forms them.  A record with weight 0, a sample that is NaN or
outside [-1, H] x [-1, W], or a batch id outside [0, N) contributes nothing.  Every element touched by a record is

    acc = +0;  for its records in ascending slot:  acc = acc + w * (gout[r][bin][c] * (1 / (sr sr)))        (each op rounded to float32)

and elements without a record keep what the caller passed.  `rank` replaces the slot as the order inside an element: the tests plant a
wrong order with it to show that they can see order at all.

The batch id is truncated as C's (int) does; NaN and out-of-int-range ids are outside this definition (the kernel's conversion
saturates, numpy's does not) and no case uses them."""
import numpy as np
import torch

import roi_ref as RR

F = np.float32
ROI_BWD_TOL = 1e-5            # tests/test_gpu_train_grads.py:299, the bar test_gpu_roi_domain.py::test_backward_against_float64 applies
STRIDES, FINEST = [4, 8, 16, 32], 56.0
SHAPES = [(4, 48 >> l, 80 >> l) for l in range(4)]          # level 0 covers 192 x 320 image pixels


def records(rois, shapes, strides, pooled, sr, finest_scale=FINEST):
    """-> (lvl, pix, w, live, src) per record in slot order: level, flat pixel (n H + y) W + x inside the level, float32 weight, whether
    the record contributes, and the row r pooled^2 + ph pooled + pw of the output gradient it reads."""
    rois = np.asarray(rois, F)
    R = rois.shape[0]
    lv = RR.levels(torch.from_numpy(rois), len(strides), finest_scale).numpy()
    N, H, W = (np.array([s[i] for s in shapes], np.int64)[lv] for i in range(3))
    sc = np.array([1.0 / s for s in strides], F)[lv]                        # spatial_scale as the float the ABI carries
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = (rois[:, j] * sc - F(0.5) for j in (1, 2, 3, 4))
        bin_h, bin_w = (y2 - y1) / F(pooled), (x2 - x1) / F(pooled)
        pp = np.arange(pooled, dtype=F)[None, :, None]
        ii = np.arange(sr, dtype=F)[None, None, :] + F(0.5)
        ys = (y1[:, None, None] + pp * bin_h[:, None, None]) + (ii * bin_h[:, None, None]) / F(sr)       # (R, ph, iy)
        xs = (x1[:, None, None] + pp * bin_w[:, None, None]) + (ii * bin_w[:, None, None]) / F(sr)       # (R, pw, ix)
        nb = np.trunc(rois[:, 0]).astype(np.int64)
        ok_n = (nb >= 0) & (nb < N)

        def axis(v, size):
            size = size[:, None, None]
            ok = ~((v < F(-1.0)) | (v > size.astype(F))) & (v == v)
            v = np.where(ok, v, F(0))
            v = np.where(v <= F(0), F(0), v)
            lo = v.astype(np.int64)                                         # v >= 0: truncation
            top = lo >= size - 1
            lo = np.where(top, size - 1, lo)
            hi = np.where(top, lo, lo + 1)
            v = np.where(top, lo.astype(F), v)
            l = (v - lo.astype(F)).astype(F)
            return ok, lo, hi, l, (F(1.0) - l).astype(F)

        oky, yl, yh, ly, hy = axis(ys, H)
        okx, xl, xh, lx, hx = axis(xs, W)
        e = lambda a: a[:, :, None, :, None]                                # y terms: (R, ph, 1, iy, 1)
        f = lambda a: a[:, None, :, None, :]                                # x terms: (R, 1, pw, 1, ix)
        w = np.stack([e(hy) * f(hx), e(hy) * f(lx), e(ly) * f(hx), e(ly) * f(lx)], -1).astype(F)
    ok = (e(oky) & f(okx) & ok_n[:, None, None, None, None])[..., None]
    n5, H5, W5 = (a[:, None, None, None, None] for a in (np.clip(nb, 0, N - 1), H, W))
    row = lambda yy, xx: (n5 * H5 + e(yy)) * W5 + f(xx)
    pix = np.stack([row(yl, xl), row(yl, xh), row(yh, xl), row(yh, xh)], -1)
    live = ok & (w != 0)
    shape = w.shape
    lvl = np.broadcast_to(lv[:, None, None, None, None, None], shape)
    src = np.broadcast_to((np.arange(R)[:, None, None] * pooled * pooled + np.arange(pooled)[None, :, None] * pooled +
                           np.arange(pooled)[None, None, :])[:, :, :, None, None, None], shape)
    return tuple(a.reshape(-1) for a in (lvl, np.where(live, pix, 0), np.where(live, w, F(0)), np.broadcast_to(live, shape), src))


def grad_ordered(shapes, strides, rois, g_bm, pooled, sr, finest_scale=FINEST, fill=0.0, rank=None):
    """The definition.  g_bm: (R, pooled^2, C) float32 output gradient, bin-major.  -> [(N, H, W, C) float32 per level], elements
    without a record hold `fill`.  rank (records,): the order inside an element, the slot when None."""
    g_bm = np.asarray(g_bm, F)
    R, PP, C = g_bm.shape
    lvl, pix, w, live, src = records(rois, shapes, strides, pooled, sr, finest_scale)
    base = np.concatenate([[0], np.cumsum([n * h * wd for n, h, wd in shapes])])
    out = [np.full((n * h * wd, C), fill, F) for n, h, wd in shapes]
    sel = np.nonzero(live)[0]                                               # ascending slot
    if len(sel) == 0:
        return [o.reshape(n, h, wd, C) for o, (n, h, wd) in zip(out, shapes)]
    key = base[lvl[sel]] + pix[sel]
    order = np.lexsort((sel if rank is None else np.asarray(rank)[sel], key))
    ks, ws, rows = key[order], w[sel][order], src[sel][order]
    gs = (g_bm.reshape(R * PP, C) * (F(1.0) / F(sr * sr))).astype(F)        # gout * (1 / (sr sr))
    heads = np.nonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))[0]
    lens = np.diff(np.concatenate([heads, [len(ks)]]))
    by_len = np.argsort(-lens, kind="stable")
    acc = np.zeros((len(heads), C), F)
    for k in range(int(lens.max())):                                        # the k-th record of every element that has one
        segs = by_len[:int((lens > k).sum())]
        at = heads[segs] + k
        acc[segs] = acc[segs] + ws[at, None] * gs[rows[at]]
    hk = ks[heads]
    hl = np.searchsorted(base, hk, side="right") - 1
    for l in range(len(shapes)):
        m = hl == l
        out[l][hk[m] - base[l]] = acc[m]
    return [o.reshape(n, h, wd, C) for o, (n, h, wd) in zip(out, shapes)]


def touched(shapes, strides, rois, pooled, sr, finest_scale=FINEST):
    """-> [(N, H, W) bool per level]: the pixels that at least one record lands on."""
    lvl, pix, _, live, _ = records(rois, shapes, strides, pooled, sr, finest_scale)
    out = []
    for l, (n, h, wd) in enumerate(shapes):
        t = np.zeros(n * h * wd, bool)
        t[pix[live & (lvl == l)]] = True
        out.append(t.reshape(n, h, wd))
    return out


def rank_r_descending(R, pooled, sr):
    """A planted WRONG order: RoIs descending, the slot order inside a RoI."""
    per = pooled * pooled * sr * sr * 4
    slot = np.arange(R * per)
    return (R - 1 - slot // per) * per + slot % per


# ------------------------------------------------------------------------------------------------------------------ the case table
def case_table():
    """name -> RoIs (n, 5) float32 on SHAPES / STRIDES (N = 4 images of 192 x 320 px)."""
    rng = np.random.default_rng(7)
    one = [1, 40.3, 30.7, 90.9, 85.2]                                        # sqrt(50.6 x 54.5) < 56: level 0
    dup64 = np.tile(np.asarray(one, F), (64, 1))
    # level 0 is 48 x 80 pixels: samples of these reach the last row / column, where x_low = x_high (y_low = y_high) and the clamped
    # coordinate makes the second tap's weight 0; each RoI three times, so that the border pixels collect several records
    clamp = np.asarray([[0, 296.0, 150.0, 323.9, 191.9], [3, 280.5, 168.2, 330.0, 200.0], [2, 300.0, 20.0, 319.0, 70.0],
                        [1, 100.0, 170.0, 150.0, 191.0]] * 3, F)
    invalid = np.asarray([[-1, 10, 10, 90, 80], [4, 10, 10, 90, 80], [7, 5, 5, 300, 280],              # batch id outside [0, 4)
                          [0, np.nan, 20, 90, 80], [1, 10, np.nan, 90, 80], [2, 10, 20, np.nan, 80], [3, 10, 20, 90, np.nan],
                          [0, 0.7 * 192, 0.2 * 192, 0.3 * 192, 0.6 * 192], [3, 0.9 * 192, 0.8 * 192, 0.2 * 192, 0.1 * 192],   # inverted
                          [0, 500, 400, 560, 470], [1, -300, -250, -100, -90]], F)                                         # outside
    # levels 0, 1 and 3 only (level 2 wants sqrt(area) in [224, 448))
    sizes = np.concatenate([rng.uniform(10, 50, 8), rng.uniform(120, 200, 8), rng.uniform(460, 700, 8)])
    c = np.stack([rng.uniform(20, 300, 24), rng.uniform(20, 170, 24)], 1)
    empty_level = np.concatenate([rng.integers(0, 4, 24)[:, None], c - sizes[:, None] / 2, c + sizes[:, None] / 2], 1).astype(F)
    return {"dup64": dup64, "clamp": clamp, "invalid": invalid, "empty_level": empty_level}
