"""The float64 definition of the RoI path (tests/roi_ref.py) against the scalar definition of mmcv RoIAlign, and the two CPU
oracles the HIP kernels are compared with -- the C gather (oracle/srf_oracle.c) and the float32 numpy box geometry
(oracle/decoder_oracle.py) -- against that definition, over the shapes and the RoI domain the GPU tests run
(tests/test_gpu_roi_domain.py)."""
import numpy as np
import pytest
import torch

import roi_ref as RR
from oracle import decoder_oracle as DO
from oracle import oracle as O
from test_oracle_bruteforce import _roi_align_def

CASES = RR.domain_cases()
PS_DEF = ((7, 2), (1, 1), (2, 3), (8, 4), (8, 1), (5, 4))


@pytest.mark.parametrize("pooled,sr", PS_DEF)
def test_definition_matches_the_scalar_definition(pooled, sr):
    """gather64 (vectorised, the level by `levels`) against the plain-Python loop of test_oracle_bruteforce.py on its seven
    RoIs plus inverted, zero-area, fully outside and 1e7-px RoIs.  Both form the scaled corner in float32 and everything
    after it in float64 (coord64), so they agree to float64 rounding; the float32 sample coordinates of the operator proper
    are what the oracle comparison below holds."""
    rng = np.random.default_rng(3)
    strides = [8, 16, 32, 64]
    feats = [rng.standard_normal((2, 5, s, s + 3)).astype(np.float32) for s in (40, 20, 10, 5)]
    rois = np.array([[0, 10.2, 20.7, 60.1, 90.3], [1, -30, -20, 40, 35], [0, 100, 100, 700, 650], [1, 5, 5, 5, 5],
                     [0, 300, 300, 301, 302], [1, 0, 0, 330, 330], [0, 900, 900, 950, 980],
                     [0, 200.5, 90.2, 40.1, 10.7], [1, 310, 250, 20, 30], [0, 120, 40, 60, 140],     # inverted: both axes, both, one
                     [1, 77.7, 33.3, 77.7, 33.3], [0, 150, 60, 150, 200],                            # zero area
                     [1, -900, -800, -500, -400], [0, 400, 10, 600, 200],                            # fully outside
                     [0, -5e6, -5e6 + 3, 5e6 + 11, 5e6], [1, 100, 50, 1e7, 250]], np.float32)        # 1e7 px
    lv = RR.levels(rois, 4)
    assert set(lv.tolist()) == {0, 1, 2, 3}
    got = RR.gather64([torch.from_numpy(f) for f in feats], rois, strides, pooled, sr, coord64=True).numpy()
    some = 0
    for r in range(len(rois)):
        l = int(lv[r])
        want = _roi_align_def(feats[l].astype(np.float64), rois[r], 1.0 / strides[l], pooled, sr)
        np.testing.assert_allclose(got[r], want, rtol=0, atol=1e-12, err_msg=f"RoI {r}")
        some += bool(np.abs(want).max() > 0)
    assert some >= 10


def test_matrix_covers_every_value_on_both_sides_of_512():
    assert 55 <= len(CASES) <= 65
    for side in (lambda c: c["C"] <= 512, lambda c: c["C"] > 512):
        cs = [c for c in CASES if side(c)]
        assert {(c["pooled"], c["sr"]) for c in cs} == set(RR.POOL_SR)
        assert {c["nl"] for c in cs} == {1, 2, 3, 4}
        assert {c["cl"] for c in cs} == {False, True} and {c["bin_major"] for c in cs} == {False, True}
        assert {c["mode"] for c in cs} == set(RR.MODES)
        assert {c["thin"] for c in cs} == {"", "h1", "w1"}
        assert {(c["mode"], c["cl"]) for c in cs} >= {(m, l) for m in ("plain", "sum6", "acc") for l in (False, True)}
    assert {c["C"] for c in CASES} == set(RR.C_LO + RR.C_HI)
    assert len({RR.case_id(c) for c in CASES}) == len(CASES)


def test_boundary_rois_sit_where_they_should_and_few_are_undecidable():
    """The level-boundary RoIs are chosen on the float32 expression alone, 6 .. 12 ulp (of the power of two) either side of 1, 2, 4, 8; at most 1 in
    20 may be dropped for sitting within 4 ulp of the power of two in float64 -- over all the cases' seeds."""
    made = dropped = 0
    for i, c in enumerate(CASES):
        rng = np.random.default_rng(1000 + i)
        r, keep = RR.boundary_rois(rng, 2, RR.EXTENT)
        e32 = RR.level_expr(r)[0].numpy().astype(np.float64)
        T = 2.0 ** np.round(np.log2(e32))
        ulps = np.abs(e32 - T) / (T * 2.0 ** -23)
        assert ((ulps >= 6) & (ulps <= 12)).all() and set(T.tolist()) == {1.0, 2.0, 4.0, 8.0}
        assert (e32 > T).sum() == (e32 < T).sum() == len(r) // 2
        lv = RR.levels(r[keep], 4).numpy()
        want = np.clip(np.floor(np.log2(RR.level_expr(r[keep])[1].numpy())), 0, 3)
        np.testing.assert_array_equal(lv, want)
        made += len(r)
        dropped += int((~keep).sum())
    print(f"\nboundary RoIs: {dropped} of {made} dropped")
    assert dropped * 20 <= made


def _unique_shapes():
    seen, out = set(), []
    for i, c in enumerate(CASES):
        k = (c["C"], c["pooled"], c["sr"], c["nl"], c["thin"])
        if k not in seen:
            seen.add(k)
            out.append((i, c))
    return out


@pytest.mark.parametrize("i,c", _unique_shapes(), ids=[RR.case_id(c) for _, c in _unique_shapes()])
def test_oracle_gather_within_gamma_of_float64(i, c):
    """The C oracle (float32, the thing the kernel must equal bit for bit) against gather64 on the case's maps and RoIs -- NaN /
    Inf coordinates, batch ids outside [0, N), inverted and 1e7-px RoIs and the level-boundary RoIs included:
    |out - out64| <= gamma D element-wise with gamma = (4 + 4 sr^2 + 1) 2^-24 (derivation: roi_ref's docstring)."""
    maps, rois, strides, finest, _ = RR.make_case(c, 1000 + i, R=24)
    out, lvl = O.roi_extract(maps, rois, strides, c["pooled"], c["sr"], finest)
    np.testing.assert_array_equal(lvl, RR.levels(rois, c["nl"], finest).numpy())
    assert np.isfinite(out).all()
    tm = [torch.from_numpy(m) for m in maps]
    out64 = RR.gather64(tm, rois, strides, c["pooled"], c["sr"], finest).numpy()
    D = RR.gather_abs64(tm, rois, strides, c["pooled"], c["sr"], finest).numpy()
    err = np.abs(out.astype(np.float64) - out64)
    g = RR.gamma(c["sr"])
    assert (out[D == 0] == 0).all() and (D > 0).mean() > 0.2
    ratio = float((err[D > 0] / (g * D[D > 0])).max())
    print(f"\n{RR.case_id(c)}: max err / (gamma D) = {ratio:.3f} (gamma = {g:.2e}, max err {err.max():.2e})")
    assert (err <= g * D).all(), ratio


@pytest.mark.parametrize("name", ["nusc", "kitti", "waymo"])
def test_decoder_oracle_rois_against_float64(name):
    """oracle/decoder_oracle.lidar_rois / image_rois (float32 numpy, pinned to the reference by test_oracle_pinned.py) against
    box_rois64 at (B, P) = (1, 200), (2, 900), (3, 129) and box_dim 8 and 10: prints e_oracle = max |delta| / s per stratum,
    pooled over the config's cases -- the yardstick the kernel is held to at 4 x on the GPU -- and asserts the input
    conditions only: every sample with its own camera matrices, at most 2 % of the (camera, box) pairs of any case left out
    for a corner within 0.1 m of the camera plane, both image strata populated (KITTI's single forward camera sees few
    boxes behind it: a handful per case, so the strata are pooled per config)."""
    errs = []
    for B, P in RR.BOX_SHAPES:
        for box_dim in (8, 10):
            boxes, l2i, pc_range, vs = RR.box_inputs(name, B, P, box_dim)
            n_cam = l2i.shape[1]
            assert all(not np.array_equal(l2i[a, c], l2i[b, d]) for a in range(B) for b in range(a) for c in range(n_cam)
                       for d in range(n_cam))
            ref = RR.box_rois64(boxes, pc_range, vs, l2i)
            bev, bm = DO.lidar_rois(boxes, pc_range, vs)
            img = DO.image_rois(boxes, pc_range, l2i)
            np.testing.assert_array_equal(bev[:, 0], ref["bev"][:, 0])
            np.testing.assert_array_equal(img[:, 0], ref["img"][:, 0])
            np.testing.assert_array_equal(bm[..., 3:], boxes[..., 3:])
            assert (np.abs(bm[..., :3] - ref["centres"]) <= ref["centres_tol"]).all()
            e = RR.box_errors(bev, img, ref)
            print(f"\n{name} B {B} P {P} D {box_dim}: e_oracle a {e['a']:.2e} ({e['n_a']} pairs) b {e['b']:.2e} ({e['n_b']}) "
                  f"bev {e['bev']:.2e}; left out {100 * e['left_out']:.2f} %; |img| up to {np.abs(ref['img'][:, 1:]).max():.1e}, "
                  f"|bev| up to {np.abs(ref['bev'][:, 1:]).max():.0f}")
            assert e["left_out"] <= 0.02
            errs.append(e)
    e = RR.pool_errors(errs)
    print(f"{name} pooled: e_oracle a {e['a']:.2e} ({e['n_a']}) b {e['b']:.2e} ({e['n_b']}) bev {e['bev']:.2e}")
    assert e["n_a"] >= 1000 and e["n_b"] >= 100
