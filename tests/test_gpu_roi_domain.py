"""csrc/roi.hip over the shapes of every config and the whole domain its C ABI admits, against float64 (tests/roi_ref.py).

Forward gather (`srf_roi_extract`, `srf_roi_extract_sum`): about 60 points of channels (1 .. 640: one to four channels per
thread in registers, and the form above 512 channels that keeps its sums in the output) x (pooled, sampling ratio) x 1 - 4
levels x map layout x output layout x call form (plain, into a strided slice, accumulate, camera sums of 1 / 2 / 6), on
RoIs that include inverted, NaN, infinite, 1e7-px and level-boundary ones and batch ids outside [0, N).  Two checks per
point: bit-equal to the C oracle (the existing contract; tests/test_roi_ref.py holds the oracle to float64 on the same
inputs), and within gamma D of the float64 gather, gamma derived in roi_ref.  Then the load-and-select of out-of-map taps
against NaN / Inf at element 0 of every plane, the backward at 128 / 256 / 516 channels, and `srf_box_rois` against
float64 with the float32 numpy chain as yardstick, composed with the camera-sum gather."""
import numpy as np
import pytest
import torch

import roi_ref as RR
from oracle import decoder_oracle as DO
from oracle import oracle as O
from srfdet3d_amd import _lib, ops, roi, synthetic as S
from test_gpu_train_grads import ROI_BWD_TOL, _edge_rois, _random_rois

pytestmark = pytest.mark.gpu
CASES = RR.domain_cases()


def _maps(maps, cl, dev):
    ts = [torch.from_numpy(m).to(dev) for m in maps]
    return [t.contiguous(memory_format=torch.channels_last) for t in ts] if cl else ts


def _sum_raw(maps, rois, strides, pooled, sr, finest, n_sum, bin_major):
    """srf_roi_extract_sum itself (ops.roi_extract routes n_sum = 1 to srf_roi_extract)."""
    nl, C, R, bins = len(strides), maps[0].shape[1], rois.shape[0] // n_sum, pooled * pooled
    fm = (_lib.FeatMap * nl)(*[ops._featmap(f, 1.0 / s) for f, s in zip(maps, strides)])
    out = torch.empty((R, bins, C) if bin_major else (R, C, pooled, pooled), dtype=torch.float32, device=rois.device)
    so_r, so_c, so_b = (bins * C, 1, C) if bin_major else (C * bins, bins, 1)
    _lib.check(_lib.lib().srf_roi_extract_sum(fm, nl, C, rois.data_ptr(), R, n_sum, pooled, sr, float(finest), out.data_ptr(),
                                              so_r, so_c, so_b, ops._stream()), "roi_extract_sum")
    return out


def _chan_major(t, bin_major, pooled):
    """-> (R, C, pooled, pooled) whatever the output layout."""
    return t.permute(0, 2, 1).reshape(t.shape[0], t.shape[2], pooled, pooled) if bin_major else t


@pytest.mark.parametrize("i", range(len(CASES)), ids=[RR.case_id(c) for c in CASES])
def test_gather_over_the_domain(dev, i):
    c = CASES[i]
    maps, rois, strides, finest, dropped = RR.make_case(c, 1000 + i, R=60)
    C, pooled, sr, nl, mode = c["C"], c["pooled"], c["sr"], c["nl"], c["mode"]
    n_sum = int(mode[3:]) if mode.startswith("sum") else 1
    R = len(rois) // n_sum
    tm, tr = _maps(maps, c["cl"], dev), torch.from_numpy(rois).to(dev)
    through_module = nl == 1 and mode == "plain"           # roi.RoIAlign: the single-level form, channel-major output only
    bm = c["bin_major"] and not through_module
    shape = (R, pooled * pooled, C) if bm else (R, C, pooled, pooled)
    prior = None
    if through_module:
        got = roi.RoIAlign(pooled, 1.0 / strides[0], sr)(tm[0], tr)
    elif mode == "plain":
        got, glv = ops.roi_extract(tm, tr, strides, pooled, sr, finest, bin_major=bm, return_levels=True)
        np.testing.assert_array_equal(glv.cpu().numpy(), RR.levels(rois, nl, finest).numpy())
    elif mode == "slice":                                  # a channel slice of a wider buffer; the rest stays as it was
        wide = (R, pooled * pooled, C + 5) if bm else (R, C + 5, pooled, pooled)
        buf = torch.full(wide, 7.0, device=dev)
        view = buf[..., 3:3 + C] if bm else buf[:, 3:3 + C]
        out = ops.roi_extract(tm, tr, strides, pooled, sr, finest, out=view, bin_major=bm)
        assert out.data_ptr() == view.data_ptr()
        rest = torch.cat([buf[..., :3], buf[..., 3 + C:]], -1) if bm else torch.cat([buf[:, :3], buf[:, 3 + C:]], 1)
        assert torch.all(rest == 7.0)
        got = view
    elif mode == "acc":
        prior = torch.randn(shape, generator=torch.Generator().manual_seed(i)).to(dev)
        got = ops.roi_extract(tm, tr, strides, pooled, sr, finest, out=prior.clone(), accumulate=True, bin_major=bm)
    elif mode == "sum1":
        got = _sum_raw(tm, tr, strides, pooled, sr, finest, 1, bm)
    else:
        got = ops.roi_extract(tm, tr, strides, pooled, sr, finest, bin_major=bm, n_sum=n_sum)
    assert tuple(got.shape) == shape
    got = _chan_major(got, bm, pooled).cpu().numpy()
    assert np.isfinite(got).all()

    # 1. the oracle, bit for bit: per-RoI gathers added in float32 in the order of the call form
    ref, lvl = O.roi_extract(maps, rois, strides, pooled, sr, finest)
    assert set(np.unique(lvl)) == set(range(nl))
    want = ref[:R].copy()
    for s in range(1, n_sum):
        want = want + ref[s * R:(s + 1) * R]
    extra = n_sum - 1
    if prior is not None:
        p = _chan_major(prior, bm, pooled).cpu().numpy()
        want, extra = p + want, 1
    np.testing.assert_array_equal(got, want)

    # 2. float64, within gamma D
    out64 = RR.gather64(tm, rois, strides, pooled, sr, finest).view(n_sum, R, C, pooled, pooled).sum(0).cpu().numpy()
    D = RR.gather_abs64(tm, rois, strides, pooled, sr, finest).view(n_sum, R, C, pooled, pooled).sum(0).cpu().numpy()
    if prior is not None:
        out64, D = out64 + p.astype(np.float64), D + np.abs(p).astype(np.float64)
    err = np.abs(got.astype(np.float64) - out64)
    g = RR.gamma(sr, extra)
    assert (D > 0).mean() > 0.2 and (got[D == 0] == 0).all()
    ratio = float((err[D > 0] / (g * D[D > 0])).max())
    print(f"\n{RR.case_id(c)}: {len(rois)} RoIs ({100 * dropped:.0f} % of the boundary RoIs dropped), max err / (gamma D) = "
          f"{ratio:.3f}, gamma {g:.2e}")
    assert (err <= g * D).all(), ratio


# ------------------------------------------------------------------------------------------------ load-and-select
def _poison_rois(rng, N, n_groups):
    """RoIs whose every tap with a non-zero weight stays at least 2 px from pixel (0, 0) of its level (x1, y1 >= 3 strides) and
    which run out of the 160 x 192 px map on the far sides, plus RoIs wholly outside; a multiple of n_groups."""
    out = []
    for l, s in enumerate(RR.STRIDES):
        side = 56.0 * 2 ** l * 1.4
        for _ in range(9):
            x1, y1 = rng.uniform(3 * s, 3 * s + 60), rng.uniform(3 * s, 3 * s + 50)
            out.append([rng.integers(0, N), x1, y1, x1 + side * rng.uniform(0.8, 1.2), y1 + side * rng.uniform(0.8, 1.2)])
    for _ in range(6):
        x1, y1 = rng.uniform(400, 900, 2)
        out.append([rng.integers(0, N), x1, y1, x1 + rng.uniform(10, 300), y1 + rng.uniform(10, 300)])
    out.append([0, -400, -300, -150, -100])
    out.append([N - 1, 30, 700, 120, 900])
    r = np.asarray(out, np.float32)
    r = r[rng.permutation(len(r))]
    return r[:len(r) - len(r) % n_groups]


@pytest.mark.parametrize("C", [128, 516])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_value_at_element_zero_of_a_plane_stays_out(dev, C, cl, bad):
    """A sample outside its map loads `plane[0]` and drops it by a select: with NaN (or +inf) at [n, c, 0, 0] of every plane
    the output must be finite and bit-equal to the clean run, for the plain gather and the sum over six groups."""
    rng = np.random.default_rng(5)
    N = 2
    maps = [rng.standard_normal((N, C, h, w)).astype(np.float32) for h, w in RR.SIZES]
    rois = _poison_rois(rng, N, 6)
    shapes = [(N, h, w) for h, w in RR.SIZES]
    for pooled, sr in ((7, 2), (2, 3)):
        n_out = n_in = 0
        for (_, h, w), (ids, t, wt) in zip(shapes, RR.taps(rois, shapes, list(RR.STRIDES), pooled, sr)):
            assert ids.numel() > 0
            assert not ((t % (h * w) == 0) & (wt > 0)).any()       # no live tap on pixel (0, 0)
            live = (wt > 0).any(-1)
            n_out, n_in = n_out + int((~live).sum()), n_in + int(live.sum())
        assert n_out > 200 and n_in > 200
        tr = torch.from_numpy(rois).to(dev)
        clean = _maps(maps, cl, dev)
        dirty = [m.clone(memory_format=torch.preserve_format) for m in clean]
        for m in dirty:
            m[:, :, 0, 0] = bad
        for n_sum in (1, 6):
            a = ops.roi_extract(clean, tr, list(RR.STRIDES), pooled, sr, bin_major=cl, n_sum=n_sum)
            b = ops.roi_extract(dirty, tr, list(RR.STRIDES), pooled, sr, bin_major=cl, n_sum=n_sum)
            assert torch.isfinite(b).all() and a.abs().sum() > 0
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (pooled, sr, n_sum)


# ------------------------------------------------------------------------------------------------ backward
IMG_STRIDES, FINEST = [4, 8, 16, 32], 56.0


def _bwd(maps, rois, pooled, sr, g_bm, cl, bin_major, dev):
    fs = [m.to(dev).contiguous(memory_format=torch.channels_last) if cl else m.to(dev).contiguous() for m in maps]
    fs = [f.detach().requires_grad_(True) for f in fs]
    y = ops.roi_extract_autograd(fs, rois.to(dev), IMG_STRIDES, pooled, sr, FINEST, bin_major=bin_major)
    R, C = rois.shape[0], maps[0].shape[1]
    g = g_bm if bin_major else g_bm.view(R, pooled, pooled, C).permute(0, 3, 1, 2)
    y.backward(g.contiguous())
    return [f.grad.permute(0, 2, 3, 1) for f in fs]


@pytest.mark.parametrize("C", [128, 256, 516])
@pytest.mark.parametrize("pooled,sr", [(7, 2), (2, 3), (8, 4)])
def test_backward_against_float64(dev, C, pooled, sr):
    """srf_roi_extract_bwd at the widths the configs train through (256: the L-only extractors) and past 512, at three
    (pooled, sr), both map layouts: the rule of test_roi_extract_backward_training_form, its normalisation (the sum of
    |weight * output gradient| of the element) and its factor."""
    g = torch.Generator().manual_seed(100 * C + pooled)
    shapes = [(4, 48 >> l, 80 >> l) for l in range(4)]
    rois = torch.cat([_random_rois(g, 240, 4, 256, torch.arange(240) % 4), _edge_rois(4, 256)])
    maps = [torch.randn(N, C, H, W, generator=g) for N, H, W in shapes]
    lv = RR.levels(rois, 4, FINEST)
    assert len(set(lv.tolist())) == 4
    gb = torch.randn(rois.shape[0], pooled * pooled, C, generator=g).to(dev)
    ref, mag = RR.grad64(shapes, IMG_STRIDES, rois, gb, pooled, sr, FINEST, dev=dev, chunk=16)
    worst = 0.0
    for cl, bin_major in ((True, True), (False, False)):
        got = _bwd(maps, rois, pooled, sr, gb, cl, bin_major, dev)
        for l in range(4):
            assert ref[l].abs().sum() > 0
            err = ((got[l].double() - ref[l]).abs() / mag[l].clamp_min(1e-300)).max().item()
            assert err <= ROI_BWD_TOL, f"channels_last {cl} level {l}: {err:.3e}"
            worst = max(worst, err)
    print(f"\nroi bwd C {C} pooled {pooled} sr {sr}: worst normalised error {worst:.2e}")


def test_backward_exact_at_256_channels_and_sr_3(dev):
    """The integer-gradient form of test_roi_extract_backward_exact at C = 256 and sr = 3: bins 1.5 or 3 feature pixels wide
    with corners on the pixel grid put every sample on a multiple of 1/4, so the weights are multiples of 1/16; output
    gradients are 9 x small integers, so that gradient * (1 / 9) rounds to the integer itself (9 k fl(1/9) is within
    k 7.5e-9 of k, far inside half an ulp).  Every product and every atomic add is then exact: bit-equal to float64."""
    g = torch.Generator().manual_seed(2)
    C, pooled, sr = 256, 7, 3
    shapes = [(12, 48 >> l, 80 >> l) for l in range(4)]
    fit = {0: [(3, 3), (3, 6), (6, 3), (6, 6)], 1: [(3, 6), (6, 3), (6, 6)], 2: [(3, 6), (6, 3), (6, 6)], 3: [(3, 6), (6, 3), (6, 6)]}
    rows, want = [], []
    for i in range(360):
        l = i % 4
        _, H, W = shapes[l]
        s = IMG_STRIDES[l]
        bw2, bh2 = fit[l][int(torch.randint(0, len(fit[l]), (1,), generator=g))]     # bin sizes in half pixels
        kx = int(torch.randint(-3, max(W - 7 * bw2 // 2, 0) + 4, (1,), generator=g))
        ky = int(torch.randint(-3, max(H - 7 * bh2 // 2, 0) + 4, (1,), generator=g))
        rows.append([i % 12, kx * s, ky * s, kx * s + 7 * bw2 * s / 2, ky * s + 7 * bh2 * s / 2])
        want.append(l)
    rois = torch.tensor(rows, dtype=torch.float32)
    assert torch.equal(RR.levels(rois, 4, FINEST), torch.tensor(want))
    for (_, H, W), (ids, t, w) in zip(shapes, RR.taps(rois, shapes, IMG_STRIDES, pooled, sr)):
        assert torch.equal(w * 16, (w * 16).round()) and ((w > 0) & (w < 1)).any()
    maps = [torch.randn(N, C, H, W, generator=g) for N, H, W in shapes]
    gb = (9 * torch.randint(-3, 4, (rois.shape[0], pooled * pooled, C), generator=g)).float().to(dev)
    ref, _ = RR.grad64(shapes, IMG_STRIDES, rois, gb, pooled, sr, FINEST, dev=dev, chunk=32)
    for cl, bin_major in ((True, True), (False, False), (True, False)):
        got = _bwd(maps, rois, pooled, sr, gb, cl, bin_major, dev)
        for l in range(4):
            assert ref[l].abs().sum() > 0
            d = (got[l].double() - ref[l]).abs().max().item()
            assert d == 0, f"channels_last {cl} bin_major {bin_major} level {l}: {d}"


# ------------------------------------------------------------------------------------------------ srf_box_rois
@pytest.mark.parametrize("name", ["nusc", "kitti", "waymo"])
def test_box_rois_against_float64(dev, name):
    """srf_box_rois at (B, P) = (1, 200), (2, 900), (3, 129), box_dim 8 and 10, every sample with its own camera matrices,
    with and without either output and with mutate_centres 0 and 1.  Nothing fixed in advance: e = max |delta| / s against
    box_rois64 per stratum (tests/roi_ref.py: box_strata), pooled over the config's cases, must stay within 4 x the figure
    of the float32 numpy chain of oracle/decoder_oracle.py on the same inputs (device expf / sinf / cosf / atan2f are a few
    ulp where numpy's are within one).  Batch ids and row order exact; the columns from 3 on never change and the centres
    become the metres only when asked."""
    hip, orc = [], []
    for B, P in RR.BOX_SHAPES:
        for box_dim in (8, 10):
            boxes, l2i, pc_range, vs = RR.box_inputs(name, B, P, box_dim)
            ref = RR.box_rois64(boxes, pc_range, vs, l2i)
            tb = lambda: torch.from_numpy(boxes.copy()).to(dev)
            tl = torch.from_numpy(l2i).to(dev)
            bx = tb()
            rb, ri = ops.box_rois(bx, pc_range, vs, mutate_centres=False, lidar2img=tl)
            assert torch.equal(bx.cpu(), torch.from_numpy(boxes))                      # untouched
            assert rb.shape == (B * P, 5) and ri.shape == (l2i.shape[1] * B * P, 5)
            bx = tb()
            rb1, ri1 = ops.box_rois(bx, pc_range, vs, mutate_centres=True, lidar2img=tl)
            after = bx.cpu().numpy()
            np.testing.assert_array_equal(after[..., 3:], boxes[..., 3:])
            assert (np.abs(after[..., :3] - ref["centres"]) <= ref["centres_tol"]).all()
            assert torch.equal(rb, rb1) and torch.equal(ri, ri1)
            bx = tb()
            rb2, none = ops.box_rois(bx, pc_range, vs, mutate_centres=False)          # BEV only
            assert none is None and torch.equal(rb, rb2) and torch.equal(bx.cpu(), torch.from_numpy(boxes))
            bx = tb()
            none, ri2 = ops.box_rois(bx, pc_range, vs, mutate_centres=True, want_bev=False, lidar2img=tl)   # image only
            assert none is None and torch.equal(ri, ri2)
            np.testing.assert_array_equal(bx.cpu().numpy(), after)
            rb, ri = rb.cpu().numpy(), ri.cpu().numpy()
            assert np.isfinite(rb).all() and np.isfinite(ri).all()
            np.testing.assert_array_equal(rb[:, 0], ref["bev"][:, 0])
            np.testing.assert_array_equal(ri[:, 0], ref["img"][:, 0])
            hip.append(RR.box_errors(rb, ri, ref))
            orc.append(RR.box_errors(DO.lidar_rois(boxes, pc_range, vs)[0], DO.image_rois(boxes, pc_range, l2i), ref))
            assert hip[-1]["left_out"] <= 0.02
            print(f"\n{name} B {B} P {P} D {box_dim}: " + "  ".join(f"{k}: e_hip {hip[-1][k]:.2e} e_oracle {orc[-1][k]:.2e}"
                                                                      for k in ("a", "b", "bev")))
    h, o = RR.pool_errors(hip), RR.pool_errors(orc)
    print(f"{name} pooled ({h['n_a']} / {h['n_b']} pairs in a / b): " + "  ".join(f"{k}: e_hip {h[k]:.2e} e_oracle {o[k]:.2e}"
                                                                                    for k in ("a", "b", "bev")))
    for k in ("a", "b", "bev"):
        assert h[k] <= 4 * o[k], f"{name} stratum {k}: e_hip {h[k]:.3e} > 4 x e_oracle {o[k]:.3e}"


def test_box_rois_feed_the_camera_sum(dev):
    """box_rois at B = 2 with six cameras into roi_extract(n_sum = n_cam) on maps laid out as the head lays them out (N = n_cam B,
    the RoI's batch id b + cam B naming its map).  The float64 gather takes the ORACLE's batch ids and, per proposal, the
    camera sum.  Its coordinates: the oracle's where the kernel's RoIs equal them bit for bit (the two differ by rounding
    elsewhere, which test_box_rois_against_float64 bounds; a projected box reaches 1e10 px, where that rounding moves sample
    points by more than a map), the kernel's elsewhere -- so a wrong batch id is a wrong feature on every row."""
    B, P, n_cam, C = 2, 129, 6, 96
    rng = np.random.default_rng(11)
    boxes = RR.random_boxes(rng, B, P, 10)
    rig = S.camera_rig(f=177.0, cx=112.0, cy=64.0)                                      # 224 x 128 images
    l2i = RR.perturbed_rigs(rig, B, rng)
    pc_range = list(S.NUSC_RANGE)
    maps = [rng.standard_normal((n_cam * B, C, 32 >> l, 56 >> l)).astype(np.float32) for l in range(4)]
    tm = _maps(maps, True, dev)
    _, ri = ops.box_rois(torch.from_numpy(boxes).to(dev), pc_range, [0.075, 0.075, 0.2], mutate_centres=False,
                         lidar2img=torch.from_numpy(l2i).to(dev))
    got = ops.roi_extract(tm, ri, IMG_STRIDES, 7, 2, FINEST, bin_major=True, n_sum=n_cam)
    got = _chan_major(got, True, 7).cpu().numpy()
    want_rois = DO.image_rois(boxes, pc_range, l2i)
    mine = ri.cpu().numpy()
    np.testing.assert_array_equal(mine[:, 0], want_rois[:, 0])
    assert len(np.unique(want_rois[:, 0])) == n_cam * B
    same = (mine == want_rois).all(1)
    rois = np.where(same[:, None], want_rois, np.concatenate([want_rois[:, :1], mine[:, 1:]], 1))
    R = B * P
    out64 = RR.gather64(tm, rois, IMG_STRIDES, 7, 2, FINEST).view(n_cam, R, C, 7, 7).sum(0).cpu().numpy()
    D = RR.gather_abs64(tm, rois, IMG_STRIDES, 7, 2, FINEST).view(n_cam, R, C, 7, 7).sum(0).cpu().numpy()
    g = RR.gamma(2, n_cam - 1)
    err = np.abs(got - out64)
    seen = (D > 0).any((1, 2, 3))
    print(f"\ncomposition: {int(same.sum())} of {len(same)} RoIs bit-equal to the oracle's, {int(seen.sum())} of {R} proposals seen by a "
          f"camera, max err / (gamma D) = {(err[D > 0] / (g * D[D > 0])).max():.3f}")
    assert seen.sum() > R // 2 and (got[D == 0] == 0).all()
    assert (err <= g * D).all()
