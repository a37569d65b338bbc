"""float64 definition of the RoI path of csrc/roi.hip: the multi-level RoIAlign gather (mmdet SingleRoIExtractor over mmcv
RoIAlign, avg pooling, aligned=True, fixed sampling ratio), its gradient w.r.t. the maps, and the proposal-box -> RoI
geometry.  Plain torch / numpy, no project kernel and no C oracle; every function runs on the CPU (the gathers also on
whatever device the maps live on, in float64).

What is float32 here is float32 in the operator itself: mmdet maps a RoI to its level in float32 and mmcv forms the sample
coordinates in float32, so the level and the sample points are computed in float32, operation by operation as
`srf_roi_level` / `srf_roi_extract_k` and mmcv do.  From the sample point on everything is float64: the bilinear weights
are the exact weights at that point and the sums carry no rounding that matters.

Error bound of a float32 implementation (`gamma`): one output is sum_taps(w * v) / sr^2 with w = (1 - ly | ly) * (1 - lx | lx).
A tap term passes through two subtractions (ly = y - y_low is exact, 1 - ly is not, per axis), the product of the two axis
weights and the product with the map value: 4 roundings.  The four taps of a sample and the sr^2 samples of a bin are then
added: fewer than 4 sr^2 additions, and one division by sr^2.  With u = 2^-24 every |w v| term is therefore off by at most
(1 + u)^c - 1 with c = 4 + 4 sr^2 + 1, and |out - out64| <= c u D to first order, where D is the same operator applied to
|map| (`gather_abs64`).  The count is an upper bound on the depth of the chain (no term passes through more than
8 + sr^2 roundings), which covers the second-order terms many times over.  Each further float32 addition of whole outputs
(the camera sum, `accumulate`) adds one rounding of the sum of the magnitudes: `gamma(sr, extra_adds)`."""
import numpy as np
import torch

U32 = 2.0 ** -24


def gamma(sr, extra_adds=0):
    """c * 2^-24 with c = 4 (tap) + 4 sr^2 (additions) + 1 (division) + extra_adds, see the module docstring."""
    return (4 + 4 * sr * sr + 1 + extra_adds) * U32


def _level_expr32(rois):
    r = torch.as_tensor(rois, dtype=torch.float32).cpu()
    area = (r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])
    return torch.sqrt(area)


def levels(rois, num_levels, finest_scale=56.0):
    """mmdet SingleRoIExtractor.map_roi_levels in float32, op by op: floor(log2(sqrt(area) / finest + 1e-6)) clamped to
    [0, num_levels - 1]; a NaN (negative or NaN area) goes to level 0.  -> (R,) int64."""
    s = _level_expr32(rois)
    t = torch.floor(torch.log2(s / torch.full_like(s, float(finest_scale)) + torch.full_like(s, 1e-6)))
    nan = t != t
    t = torch.where(nan, torch.zeros_like(t), t).clamp(0, num_levels - 1)
    return t.long()


def level_expr(rois, finest_scale=56.0):
    """sqrt(area) / finest + 1e-6 -> (float32 value op by op, float64 value from the same float32 RoIs)."""
    s = _level_expr32(rois)
    e32 = s / torch.full_like(s, float(finest_scale)) + torch.full_like(s, 1e-6)
    r = torch.as_tensor(rois, dtype=torch.float32).cpu().double()
    e64 = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / float(np.float32(finest_scale)) + float(np.float32(1e-6))
    return e32, e64


def taps(rois, shapes, strides, pooled, sr, finest_scale=56.0, lv=None, coord64=False):
    """Bilinear taps of every sample point of every RoI.

    rois (R, 5) float32 [batch id, x1, y1, x2, y2]; shapes [(N, H, W)] and strides per level.  The level is `levels(...)`
    unless `lv` (R,) is given.  Sample coordinates in float32 op by op (coord64: the scaled corner in float32 and the rest
    in float64, the form of the scalar definition in test_oracle_bruteforce.py), mmcv's rules on top: a sample that is NaN
    or outside [-1, H] x [-1, W], or whose RoI names a batch id outside [0, N), contributes nothing (weights 0, taps 0);
    coordinates below 0 clamp to 0; the low tap is the truncation, clamped to the last row / column together with the
    coordinate.
    -> per level: (RoI ids (r,), flat tap rows (r, pooled sr, pooled sr, 4) into (N H W), float64 weights, same shape);
    axis 1 is y (bin-major, sample-minor), axis 2 is x."""
    rois = torch.as_tensor(rois, dtype=torch.float32).cpu()
    if lv is None:
        lv = levels(rois, len(strides), finest_scale)
    lv = torch.as_tensor(lv).cpu().long()
    dt = torch.float64 if coord64 else torch.float32
    K = pooled * sr
    res = []
    for l, ((N, H, W), s) in enumerate(zip(shapes, strides)):
        ids = torch.nonzero(lv == l).squeeze(1)
        b = rois[ids]
        r = b.shape[0]
        sc = torch.tensor(1.0 / s, dtype=torch.float32)
        x1, y1, x2, y2 = ((b[:, j] * sc).to(dt) - 0.5 for j in (1, 2, 3, 4))
        bw, bh = (x2 - x1) / torch.full_like(x1, float(pooled)), (y2 - y1) / torch.full_like(y1, float(pooled))
        j = torch.arange(K)
        pp, ii = (j // sr).to(dt), (j % sr).to(dt) + 0.5
        ys = (y1[:, None] + pp * bh[:, None]) + (ii * bh[:, None]) / torch.full((r, K), float(sr), dtype=dt)
        xs = (x1[:, None] + pp * bw[:, None]) + (ii * bw[:, None]) / torch.full((r, K), float(sr), dtype=dt)
        n = b[:, 0].long()   # (int) truncation, as the kernel
        ok_n = (n >= 0) & (n < N)

        def axis(v, size):
            ok = ~((v < -1.0) | (v > size)) & (v == v)
            v = torch.where(ok, v, torch.zeros_like(v)).clamp(min=0.0)
            lo = v.long()
            top = lo >= size - 1
            lo = torch.where(top, torch.full_like(lo, size - 1), lo)
            hi = torch.where(top, lo, lo + 1)
            v = torch.where(top, lo.to(dt), v)
            frac = v.double() - lo.double()
            return ok, lo, hi, frac, 1.0 - frac

        oky, yl, yh, ly, hy = axis(ys, H)
        okx, xl, xh, lx, hx = axis(xs, W)
        ok = (oky[:, :, None] & okx[:, None, :] & ok_n[:, None, None]).unsqueeze(-1)
        w = torch.stack([hy[:, :, None] * hx[:, None, :], hy[:, :, None] * lx[:, None, :], ly[:, :, None] * hx[:, None, :],
                         ly[:, :, None] * lx[:, None, :]], -1) * ok
        nn_ = n.clamp(0, N - 1)[:, None, None]
        row = lambda yy, xx: (nn_ * H + yy[:, :, None]) * W + xx[:, None, :]
        t = torch.stack([row(yl, xl), row(yl, xh), row(yh, xl), row(yh, xh)], -1) * ok
        res.append((ids, t, w))
    return res


def _shapes(maps):
    return [(m.shape[0], m.shape[2], m.shape[3]) for m in maps]


def gather64(maps, rois, strides, pooled=7, sr=2, finest_scale=56.0, lv=None, coord64=False, absolute=False):
    """The gather in float64: maps [(N, C, H, W)] (any float dtype / layout / device) -> (R, C, pooled, pooled) float64 on
    the maps' device.  absolute: the same operator on |maps| (see gather_abs64)."""
    dev = maps[0].device
    C = maps[0].shape[1]
    R = len(rois)
    out = torch.zeros(R, C, pooled, pooled, dtype=torch.float64, device=dev)
    K = pooled * sr
    chunk = max(1, int(2e7 // (K * K * C)))
    for m, (ids, t, w) in zip(maps, taps(rois, _shapes(maps), strides, pooled, sr, finest_scale, lv, coord64)):
        N, _, H, W = m.shape
        flat = m.double().permute(0, 2, 3, 1).reshape(N * H * W, C)
        if absolute:
            flat = flat.abs()
        for c0 in range(0, ids.shape[0], chunk):
            sl = slice(c0, c0 + chunk)
            tt, ww = t[sl].to(dev), w[sl].to(dev)
            acc = torch.zeros(tt.shape[0], K, K, C, dtype=torch.float64, device=dev)
            for q in range(4):
                acc += ww[..., q, None] * flat[tt[..., q].reshape(-1)].view(-1, K, K, C)
            acc = acc.view(-1, pooled, sr, pooled, sr, C).sum((2, 4)) / float(sr * sr)
            out[ids[sl].to(dev)] = acc.permute(0, 3, 1, 2)
    return out


def gather_abs64(maps, rois, strides, pooled=7, sr=2, finest_scale=56.0, lv=None):
    """D: the gather of |maps|, the scale of the rounding error of one output (every weight is >= 0)."""
    return gather64(maps, rois, strides, pooled, sr, finest_scale, lv, absolute=True)


def grad64(shapes, strides, rois, g_bm, pooled=7, sr=2, finest_scale=56.0, lv=None, dev="cpu", chunk=64):
    """float64 gradient of the gather w.r.t. each map, channels-last (N, H, W, C), and its magnitude sums (the same sum over
    |weight * gradient|).  g_bm: (R, pooled^2, C) output gradient in bin-major form."""
    C = g_bm.shape[2]
    grads, mags = [], []
    for (N, H, W), (ids, t_all, w_all) in zip(shapes, taps(rois, shapes, strides, pooled, sr, finest_scale, lv)):
        gr = torch.zeros(N * H * W, C, dtype=torch.float64, device=dev)
        mg = torch.zeros_like(gr)
        for c0 in range(0, ids.shape[0], chunk):
            sl = slice(c0, c0 + chunk)
            g = g_bm[ids[sl].to(dev)].double().view(-1, pooled, pooled, C) / float(sr * sr)
            g = g.repeat_interleave(sr, 1).repeat_interleave(sr, 2)            # (r, K, K, C): each bin's sr^2 samples
            t, ww = t_all[sl].to(dev), w_all[sl].to(dev)
            for q in range(4):
                src = ww[..., q:q + 1] * g
                gr.index_add_(0, t[..., q].reshape(-1), src.reshape(-1, C))
                mg.index_add_(0, t[..., q].reshape(-1), src.abs().reshape(-1, C))
        grads.append(gr.view(N, H, W, C))
        mags.append(mg.view(N, H, W, C))
    return grads, mags


# ---------------------------------------------------------------------------------------------- box -> RoI geometry
_SX = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)
_SY = np.array([-1, -1, 1, 1, -1, -1, 1, 1], np.float64)
_SZ = np.array([-1, -1, -1, -1, 1, 1, 1, 1], np.float64)


def box_rois64(boxes, pc_range, voxel_size, lidar2img=None):
    """srf_box_rois in float64 from the float32 inputs cast up.

    boxes (B, P, >= 8) float32 [normalised centre, log w l h, sin, cos, ...]; `lo`, `ext = hi - lo` and the voxel size are
    rounded to float32 first, as the kernel receives them (the range arrives as float32 and is subtracted in float32);
    lidar2img (B, n_cam, 4, 4) float32 or None.
    -> dict: centres (B, P, 3) metres and centres_tol, the rounding of their float32 product and sum; bev (B P, 5) and s_bev (B P, 4); with lidar2img also img (n_cam B P, 5), s_img
    (n_cam B P, 4) and pz (n_cam, B, P, 8).  Rows and batch ids as the kernel writes them (image rows cam-major, batch id
    b + cam B).  s is the first-order sensitivity of a coordinate to a relative perturbation of its inputs, maximised over
    the eight corners (the float32 and float64 min / max may pick different corners): image u = pu / d has
    s = (sum_j |M0j| |Xj| + |u| sum_j |M2j| |Xj|) / d with X = (x, y, z, 1); BEV (X - lo) / vs has (|X| + |lo|) / vs."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    B, P = b.shape[:2]
    r32 = np.asarray(pc_range, np.float32)
    lo = r32[:3].astype(np.float64)
    ext = (r32[3:] - r32[:3]).astype(np.float32).astype(np.float64)
    vs = np.asarray(voxel_size, np.float32).astype(np.float64)
    ctr = b[..., :3] * ext + lo
    w, l, h = (np.exp(b[..., i]) for i in (3, 4, 5))
    ry = np.arctan2(b[..., 6], b[..., 7])
    cs, sn = np.cos(ry)[..., None], np.sin(ry)[..., None]
    x0, y0, z0 = (w / 2)[..., None] * _SX, (l / 2)[..., None] * _SY, (h / 2)[..., None] * _SZ
    X = ctr[..., 0:1] + (x0 * cs + y0 * sn)          # (B, P, 8)
    Y = ctr[..., 1:2] + (x0 * (-sn) + y0 * cs)
    Z = ctr[..., 2:3] + z0
    px, py = (X - lo[0]) / vs[0], (Y - lo[1]) / vs[1]
    bid = np.repeat(np.arange(B, dtype=np.float64), P)
    flat = lambda a: a.reshape(B * P)
    # centres: one product and one sum in float32, each within u = 2^-24 of its own magnitude
    out = dict(centres=ctr, centres_tol=2 * U32 * (np.abs(b[..., :3]) * ext + np.abs(lo) + np.abs(ctr)))
    out["bev"] = np.stack([bid, flat(px.min(-1)), flat(py.min(-1)), flat(px.max(-1)), flat(py.max(-1))], 1)
    sx = flat(((np.abs(X) + abs(lo[0])) / vs[0]).max(-1))
    sy = flat(((np.abs(Y) + abs(lo[1])) / vs[1]).max(-1))
    out["s_bev"] = np.stack([sx, sy, sx, sy], 1)
    if lidar2img is None:
        return out
    M = np.asarray(lidar2img, np.float32).astype(np.float64)
    n_cam = M.shape[1]
    hom = np.stack([X, Y, Z, np.ones_like(X)], -1)   # (B, P, 8, 4)
    rows, sens, pzs = [], [], []
    for cam in range(n_cam):
        m = M[:, cam][:, None, None]                 # (B, 1, 1, 4, 4)
        p = (m * hom[..., None, :]).sum(-1)          # (B, P, 8, 4)
        mag = (np.abs(m) * np.abs(hom[..., None, :])).sum(-1)
        pz = p[..., 2]
        d = np.maximum(pz, float(np.float32(1e-5)))
        u, v = p[..., 0] / d, p[..., 1] / d
        su = ((mag[..., 0] + np.abs(u) * mag[..., 2]) / d).max(-1)
        sv = ((mag[..., 1] + np.abs(v) * mag[..., 2]) / d).max(-1)
        rows.append(np.stack([bid + cam * B, flat(u.min(-1)), flat(v.min(-1)), flat(u.max(-1)), flat(v.max(-1))], 1))
        sens.append(np.stack([flat(su), flat(sv), flat(su), flat(sv)], 1))
        pzs.append(pz)
    out["img"], out["s_img"], out["pz"] = np.concatenate(rows, 0), np.concatenate(sens, 0), np.stack(pzs, 0)
    return out


def box_strata(pz):
    """pz (n_cam, B, P, 8) -> boolean masks over the n_cam B P image rows: (a) all eight corners >= 1 m in front of the camera
    plane; (b) the other pairs whose every corner is >= 0.1 m in front or >= 0.1 m behind (a corner behind is clamped to
    d = 1e-5 by both sides alike); left out: a corner within 0.1 m of the plane, where d itself is decided by rounding."""
    a = (pz >= 1.0).all(-1).reshape(-1)
    clear = (np.abs(pz) >= 0.1).all(-1).reshape(-1)
    return a, clear & ~a, ~clear


def random_boxes(rng, B, P, box_dim):
    """centres U(0, 1), sizes log U(0.4, 6) m, yaw U(-pi, pi), the columns past 8 filled with noise."""
    yaw = rng.uniform(-np.pi, np.pi, (B, P))
    cols = [rng.uniform(0, 1, (B, P, 3)), rng.uniform(np.log(0.4), np.log(6.0), (B, P, 3)), np.sin(yaw)[..., None],
            np.cos(yaw)[..., None], rng.standard_normal((B, P, box_dim - 8))]
    return np.concatenate(cols, -1).astype(np.float32)


def perturbed_rigs(rig, B, rng):
    """(n_cam, 4, 4) -> (B, n_cam, 4, 4) float32: sample 0 keeps the rig, every further sample gets the cameras in another order
    and its own small change of the extrinsics (a rotation about z and a shift), so that no two samples share a matrix."""
    rig = np.asarray(rig, np.float64)
    out = [rig]
    for b in range(1, B):
        a = rng.uniform(-0.05, 0.05)
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = rng.uniform(-0.3, 0.3, 3)
        out.append(np.roll(rig, b, 0) @ T)
    return np.stack(out, 0).astype(np.float32)


# ---------------------------------------------------------------------------------------------- RoIs of the ABI domain
def boundary_rois(rng, N, extent, finest_scale=56.0, per_side=3):
    """RoIs whose float32 sqrt(area) / finest + 1e-6 sits 6 .. 12 ulp either side of T = 1, 2, 4 and 8 (ulp = T 2^-23 on
    both sides, so that log2 of the value is as far from the integer below as above it), chosen on the float32 value alone (y2 is stepped through neighbouring float32 values until the expression lands there).
    -> (rois (n, 5) float32, keep (n,) bool): keep is False where the float64 value of the expression is within 4 of those ulp
    of the power of two, where an implementation whose log2f is a few ulp off may legitimately pick either level."""
    out = []
    for k in range(4):
        T = 2.0 ** k
        for side in (-1, 1):
            found = 0
            while found < per_side:
                w = float(np.exp(rng.uniform(np.log(0.4), np.log(2.5)))) * 56.0 * T
                h = (56.0 * (T - 1e-6)) ** 2 / w
                x1, y1 = rng.uniform(-0.3 * extent, 0.9 * extent, 2)
                y2s = np.float32(y1 + h) + np.arange(-300, 301).astype(np.float32) * np.spacing(np.float32(y1 + h))
                c = np.zeros((len(y2s), 5), np.float32)
                c[:, 0], c[:, 1], c[:, 2], c[:, 3], c[:, 4] = rng.integers(0, N), x1, y1, x1 + w, y2s
                e32 = level_expr(c, finest_scale)[0].numpy().astype(np.float64)
                ulps = (e32 - T) / (T * 2.0 ** -23)
                hit = np.nonzero((ulps * side >= 6) & (ulps * side <= 12))[0]
                if len(hit):
                    out.append(c[hit[rng.integers(0, len(hit))]])
                    found += 1
    rois = np.stack(out, 0)
    e64 = level_expr(rois, finest_scale)[1].numpy()
    T = 2.0 ** np.round(np.log2(e64))
    return rois, np.abs(e64 - T) > 4 * T * 2.0 ** -23


def domain_rois(rng, base, N, extent, finest_scale=56.0):
    """The RoIs of one case of the domain tests: `base` (random boxes over the map, some fully outside, some of zero area)
    and the edges of the ABI: inverted RoIs (x2 < x1, y2 < y1, both), batch ids -1 and N, RoIs of 1e7 px, RoIs with one NaN
    coordinate, (-inf, +inf) spans, and RoIs at the level boundaries (`boundary_rois`, the undecidable ones dropped).
    -> (rois (n, 5) float32 in random order, fraction of the boundary RoIs dropped)."""
    e = float(extent)
    edge = [[0, 0.7 * e, 0.2 * e, 0.3 * e, 0.6 * e], [N - 1, 0.1 * e, 0.8 * e, 0.5 * e, 0.3 * e],      # one axis inverted: NaN level
            [0, 0.9 * e, 0.8 * e, 0.2 * e, 0.1 * e], [N - 1, 0.4 * e, 0.5 * e, 0.3 * e, 0.35 * e],     # both: a real level
            [0, 1.2 * e, 0.6 * e, -0.2 * e, -0.1 * e],
            [-1, 10, 10, 0.5 * e, 0.4 * e], [N, 10, 10, 0.5 * e, 0.4 * e], [N + 3, 5, 5, 0.9 * e, 0.8 * e],
            [0, -5e6, -5e6 + 3, 5e6 + 11, 5e6], [N - 1, 0.3 * e, 0.2 * e, 1e7, 0.6 * e],
            [0, np.nan, 20, 90, 80], [N - 1, 10, np.nan, 90, 80], [0, 10, 20, np.nan, 80], [N - 1, 10, 20, 90, np.nan],
            [0, -np.inf, 20, np.inf, 80], [N - 1, 10, -np.inf, 90, np.inf], [0, -np.inf, -np.inf, np.inf, np.inf],
            [N - 1, 30, 20, np.inf, 80]]
    br, keep = boundary_rois(rng, N, extent, finest_scale)
    allr = np.concatenate([np.asarray(base, np.float32), np.asarray(edge, np.float32), br[keep]], 0)
    return allr[rng.permutation(len(allr))], 1.0 - keep.mean()


# ---------------------------------------------------------------------------------------------- the case matrix
C_LO, C_HI = (1, 3, 96, 128, 130, 256, 384, 512), (516, 640)      # <= 512: running sums in registers; above: in the output element
POOL_SR = ((7, 2), (1, 1), (2, 3), (3, 3), (8, 4), (8, 1), (5, 4))
MODES = ("plain", "slice", "acc", "sum1", "sum2", "sum6")
STRIDES = (4, 8, 16, 32)
SIZES = ((40, 48), (20, 24), (10, 12), (5, 6))                     # level 0 covers 160 x 192 px
EXTENT = 192


def domain_cases():
    """About 60 points of C x (pooled, sr) x levels x map layout x output layout x call form x thin map, pruned so that every
    value of every axis appears on both sides of C = 512 (tests/test_roi_ref.py checks that it does)."""
    cases = []
    for Cs, n in ((C_LO, 32), (C_HI, 28)):
        for i in range(n):
            pooled, sr = POOL_SR[i % 7]
            nl = (4, 1, 3, 2)[(i + i // 4) % 4]
            thin = ("", "h1", "", "w1")[(i // 2) % 4] if nl > 1 else ""
            cases.append(dict(C=Cs[i % len(Cs)], pooled=pooled, sr=sr, nl=nl, cl=bool((i // 3) % 2), bin_major=bool((i + i // 6) % 2),
                              mode=MODES[(i + i // 7) % 6], thin=thin))
    return cases


def case_id(c):
    return (f"C{c['C']}-p{c['pooled']}s{c['sr']}-L{c['nl']}{c['thin']}-{'nhwc' if c['cl'] else 'nchw'}-"
            f"{'bin' if c['bin_major'] else 'chan'}-{c['mode']}")


def make_case(c, seed, R=40, N=2):
    """-> (maps [(N, C, H, W) float32 numpy], rois (n, 5) float32, strides, finest_scale, boundary RoIs dropped / made).
    A single level is the form behind roi.RoIAlign: finest_scale 1e30.  thin: the last level is one row (h1) or one column
    (w1) high / wide.  The number of RoIs is a multiple of the case's n_sum (padded with copies of the first ones)."""
    rng = np.random.default_rng(seed)
    nl = c["nl"]
    sizes = [list(s) for s in SIZES[:nl]]
    if c["thin"] == "h1":
        sizes[-1][0] = 1
    if c["thin"] == "w1":
        sizes[-1][1] = 1
    maps = [rng.standard_normal((N, c["C"], h, w)).astype(np.float32) for h, w in sizes]
    finest = 56.0 if nl > 1 else 1e30
    from test_gpu_roi import _rois                     # the RoIs of the single-shape tests are the base
    rois, dropped = domain_rois(rng, _rois(rng, R, size=EXTENT, N=N), N, EXTENT)
    n_sum = int(c["mode"][3:]) if c["mode"].startswith("sum") else 1
    pad = -len(rois) % n_sum
    if pad:
        rois = np.concatenate([rois, rois[:pad]], 0)
    return maps, rois, list(STRIDES[:nl]), finest, dropped


# ---------------------------------------------------------------------------------------------- box geometry cases
def box_configs():
    """name -> (pc_range, voxel_size, rig (n_cam, 4, 4)): nuScenes (nusc_LC, six cameras), KITTI (one camera) and Waymo (five
    cameras at 960 x 640) with the rigs of srfdet3d_amd.synthetic."""
    from srfdet3d_amd import synthetic as S
    return {"nusc": (list(S.NUSC_RANGE), [0.075, 0.075, 0.2], S.camera_rig()),
            "kitti": (list(S.KITTI_RANGE), [0.05, 0.05, 0.1], S.camera_rig(n_cam=1)),
            "waymo": (list(S.WAYMO_RANGE), [0.1, 0.1, 0.15], S.camera_rig(n_cam=5, f=1266.0 * 960 / 1600, cx=480.0, cy=320.0))}


BOX_SHAPES = ((1, 200), (2, 900), (3, 129))


def box_inputs(name, B, P, box_dim):
    """-> (boxes (B, P, box_dim) float32, lidar2img (B, n_cam, 4, 4) float32, pc_range, voxel_size) of one geometry case."""
    pc_range, vs, rig = box_configs()[name]
    rng = np.random.default_rng(100 * B + box_dim)
    return random_boxes(rng, B, P, box_dim), perturbed_rigs(rig, B, rng), pc_range, vs


def pool_errors(errs):
    """box_errors of several cases -> the strata pooled: the largest figure and the summed populations."""
    return dict(a=max(e["a"] for e in errs), b=max(e["b"] for e in errs), bev=max(e["bev"] for e in errs),
                left_out=max(e["left_out"] for e in errs), n_a=sum(e["n_a"] for e in errs), n_b=sum(e["n_b"] for e in errs))


def box_errors(bev, img, ref):
    """max |delta| / s per stratum of `box_strata` -> dict(a, b, bev, left_out (fraction of the (camera, box) pairs)).
    bev / img: the float32 RoIs under test ((B P, 5) / (n_cam B P, 5)); ref: box_rois64's dict."""
    a, b, out = box_strata(ref["pz"])
    e = np.abs(np.asarray(img, np.float64)[:, 1:] - ref["img"][:, 1:]) / ref["s_img"]
    eb = np.abs(np.asarray(bev, np.float64)[:, 1:] - ref["bev"][:, 1:]) / ref["s_bev"]
    return dict(a=float(e[a].max()), b=float(e[b].max()), bev=float(eb.max()), left_out=float(out.mean()),
                n_a=int(a.sum()), n_b=int(b.sum()))
