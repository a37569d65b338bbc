"""Backward kernels at the shapes training runs them: the sparse convolution (csrc/spconv_bwd.hip, `_SpconvFn`) on bitmap
rulebooks of a nuScenes level 1 at bs = 2 walked down the four strided levels of the nusc_L encoder, the whole encoder in
train mode against a float64 run of the same module, and the RoI gather backward (`srf_roi_extract_bwd_k`,
`_RoIExtractFn`) in the form the heads call it (bin-major, channels-last, C = 128, four levels, an image RoI stack over 12
images).  Every reference is plain float64 torch (index_select / mm / index_add_), no project kernel."""
import copy

import numpy as np
import pytest
import torch

from roi_ref import grad64
from spconv_ref import conv_ref, conv_ref_autograd, dense_grads
from srfdet3d_amd import ops

pytestmark = pytest.mark.gpu

VS = [0.075, 0.075, 0.2]
SHAPE1 = [41, 1472, 1472]
BW_ROWS = 2048              # csrc/spconv_bwd.hip: output rows one workgroup of srf_spconv_bwd_weight_k reduces
C16L_MIN_ROWS = 60000       # csrc/spconv.hip: srf_spconv_c16l_k (16 output channels) from this many output rows up
# the four strided convs of the nusc_L encoder (encoder_paddings and conv_out of srfdet_voxel_nusc_L): ksize, stride, pad
DOWN = [([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 3, 3], [2, 2, 2], [0, 1, 1]),
        ([3, 1, 1], [2, 1, 1], [0, 0, 0])]


@pytest.mark.parametrize("subm", [True, False])
def test_conv_ref_matches_dense_conv3d(dev, subm):
    """Anchor of conv_ref: on a grid small enough to densify it equals conv3d autograd (dense_grads), so it can be trusted at
    sizes where no dense grid fits."""
    rng = np.random.default_rng(7)
    shape = [7, 18, 16]
    idx = np.argwhere(rng.random((2, *shape)) < 0.2).astype(np.int32)
    t = torch.from_numpy(idx).to(dev)
    if subm:
        nbr, _ = ops.rulebook_subm(t, shape, [3, 3, 3], ops.coord_table_build(t, shape, 2))
        out_idx, oshape, st, pd = idx, shape, 1, 1
    else:
        oi, nbr, _, _, oshape = ops.rulebook_strided(t, shape, 2, *DOWN[0])
        out_idx, st, pd = oi.cpu().numpy(), 2, 1
    x = rng.standard_normal((len(idx), 16))
    W = rng.standard_normal((27, 16, 32)) * 0.1
    g = rng.standard_normal((nbr.shape[1], 32))
    want = dense_grads(idx, shape, x, W, g, out_idx, list(oshape), st, pd, (3, 3, 3))
    (out, dx, dW), _ = conv_ref(nbr, *(torch.from_numpy(a).to(dev) for a in (x, W, g)))
    for a, b in zip((out, dx, dW), want):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-12, atol=1e-12)


def _kernel_grads(nbr, x, W, g, subm):
    """(out, d_x, d_W) of ops.spconv_fwd through autograd (srf_spconv_bwd_data / _bwd_weight)."""
    f = x.float().requires_grad_(True)
    w = W.float().requires_grad_(True)
    out = ops.spconv_fwd(f, w, nbr, subm=subm)
    out.backward(g.float())
    return out.detach(), f.grad, w.grad


def _layer_data(kind, A_in, A_out, K, cin, cout, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    if kind == "int":   # every product and partial sum an integer below 2^24: any order of the adds is exact
        r = lambda n, lo, hi: torch.randint(lo, hi + 1, n, generator=gen, device=dev).float()
        return r((A_in, cin), -3, 3), r((K, cin, cout), -2, 2), r((A_out, cout), -2, 2)
    n = lambda *s: torch.randn(*s, generator=gen, device=dev)
    return n(A_in, cin), n(K, cin, cout) / np.sqrt(K * cin), n(A_out, cout)


def _check_conv(nbr, A_in, cin, cout, subm, dev, seed):
    """Both data kinds through the kernels against conv_ref; -> the worst normalised error of (out, d_in, d_W)."""
    K, A_out = nbr.shape
    worst = {}
    for kind in ("int", "gauss"):
        x, W, g = _layer_data(kind, A_in, A_out, K, cin, cout, dev, seed)
        got = _kernel_grads(nbr, x, W, g, subm)
        ref, mag = conv_ref(nbr, x, W, g)
        for name, a, b, m in zip(("out", "d_in", "d_W"), got, ref, mag):
            assert a.shape == b.shape, name
            if kind == "int":
                assert torch.equal(a.double(), b), f"{name}: {(a.double() - b).abs().max().item()} off on integer data"
            else:
                err = ((a.double() - b).abs() / m.clamp_min(1e-300)).max().item()
                assert err <= 1e-5, f"{name}: normalised error {err:.3e}"
                worst[name] = err
    return worst


# ------------------------------------------------------------------------------------------------ levels (bitmap rulebooks)
def _level1(n, batch, seed=2000):
    from oracle import oracle as O
    from srfdet3d_amd import synthetic as S
    idx = []
    for b in range(batch):
        _, c, _ = O.hard_voxelize(S.nuscenes_sweep(seed + b, n[b] if isinstance(n, (list, tuple)) else n), VS, list(S.NUSC_RANGE),
                                  10, 160000)
        idx.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
    return np.concatenate(idx, 0).astype(np.int32)


def _walk(idx0, batch, dev):
    """Level 1 sorted by bitmap rank and the four strided levels below it, built as SparseEncoder.forward builds them
    (sparse.py: sorted_by_bitmap, rulebook_subm_bitmap, rulebook_strided_bitmap).  -> list of dicts per level: rows, SubM
    rulebook (K=27), and the strided rulebook down to the next level."""
    lvl, _, sidx = ops.bitmap_build(torch.from_numpy(idx0).to(dev), SHAPE1, batch)
    levels = []
    idx, shape = sidx, SHAPE1
    for i in range(5):
        d = dict(idx=idx, rows=idx.shape[0], shape=shape)
        if i < 4:
            d["subm"] = ops.rulebook_subm_bitmap(idx, lvl, [3, 3, 3])[0]
            ks, st, pd = DOWN[i]
            oi, nbr, _, out_lvl, osh = ops.rulebook_strided_bitmap(idx, lvl, ks, st, pd)
            d["down"] = nbr
            idx, shape, lvl = oi, osh, out_lvl
        levels.append(d)
    return levels


@pytest.fixture(scope="module")
def levels(dev):
    # 40k points per frame: level 1 holds 67k rows (above C16L_MIN_ROWS), levels 2-4 152k / 146k / 81k
    return _walk(_level1(40000, 2), 2, dev)


# name, level, Cin, Cout, SubM (else the strided conv of that level): every distinct layer of the nusc_L encoder, and Cin = 4
LAYERS = [("conv_input_5_16", 0, 5, 16, True), ("subm_4_16", 0, 4, 16, True), ("subm_16_16", 0, 16, 16, True),
          ("down_16_32", 0, 16, 32, False), ("subm_32_32", 1, 32, 32, True), ("down_32_64", 1, 32, 64, False),
          ("subm_64_64", 2, 64, 64, True), ("down_64_128", 2, 64, 128, False), ("subm_128_128", 3, 128, 128, True),
          ("conv_out_128_128", 3, 128, 128, False)]


@pytest.mark.parametrize("name,li,cin,cout,subm", LAYERS, ids=[n[0] for n in LAYERS])
def test_layer_gradients_at_encoder_scale(dev, levels, name, li, cin, cout, subm):
    L = levels[li]
    nbr = L["subm"] if subm else L["down"]
    A_in, A_out = L["rows"], nbr.shape[1]
    if name == "subm_16_16":   # the 16 -> 16 data gradient runs the LDS-weight form
        assert A_in >= C16L_MIN_ROWS
    worst = _check_conv(nbr, A_in, cin, cout, subm, dev, seed=li * 1000 + cin + 7 * cout)
    print(f"\n{name}: A_in {A_in} A_out {A_out} ({-(-A_out // BW_ROWS)} row blocks, A_out % 32 = {A_out % 32}) "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_encoder_levels_reach_the_cases(levels):
    """The sizes above must keep reaching what the per-layer test exists for: a weight gradient over more than four row
    blocks with a partial last chunk, the 16 -> 16 data gradient in the LDS-weight form, and the 32 -> 16 data gradient
    (srf_spconv_mfma16_k) of the 16 -> 32 strided conv, which writes the level-1 rows and reads the level-2 rows."""
    outs = [(L["rows"], n.shape[1]) for L in levels[:4] for n in (L["subm"], L["down"])]
    assert any(a_out > 4 * BW_ROWS and a_out % 32 != 0 for _, a_out in outs)
    assert levels[0]["rows"] >= C16L_MIN_ROWS            # the data gradients of level 1 (subm_16_16, conv_input, down_16_32)
    assert levels[0]["down"].shape == (27, levels[1]["rows"]) and levels[1]["rows"] > 4 * BW_ROWS   # down_16_32's rulebook


def test_bitmap_subm_rulebooks_are_symmetric(levels):
    """_SpconvFn.backward runs the data gradient of a SubM layer on the table itself with the weights flipped: it needs
    nbr[K-1-k][nbr[k][o]] == o for every pair."""
    for i, L in enumerate(levels[:4]):
        nbr = L["subm"].cpu().numpy()
        K, A = nbr.shape
        assert np.array_equal(nbr[K // 2], np.arange(A)), i   # the centre tap is the identity
        for k in range(K):
            o = np.nonzero(nbr[k] >= 0)[0]
            np.testing.assert_array_equal(nbr[K - 1 - k][nbr[k][o]], o, err_msg=f"level {i} offset {k}")


def test_transpose_rulebook_is_the_inverse(levels):
    for i, L in enumerate(levels[:4]):
        for nbr in (L["down"], L["subm"]):
            a_in = L["rows"]
            got = ops.spconv_transpose_rulebook(nbr, a_in).cpu().numpy()
            n = nbr.cpu().numpy()
            want = np.full((n.shape[0], a_in), -1, np.int32)
            for k in range(n.shape[0]):
                o = np.nonzero(n[k] >= 0)[0]
                assert len(np.unique(n[k][o])) == len(o)      # one output at most per (offset, input row)
                want[k, n[k][o]] = o
            np.testing.assert_array_equal(got, want, err_msg=f"level {i}")


def test_empty_level_through_autograd(dev):
    e = torch.zeros((0, 4), dtype=torch.int32, device=dev)
    lvl, _, sidx = ops.bitmap_build(e, SHAPE1, 2)
    nbr, _ = ops.rulebook_subm_bitmap(sidx, lvl, [3, 3, 3])
    _, dnbr, _, _, _ = ops.rulebook_strided_bitmap(sidx, lvl, *DOWN[0])
    for n, subm, cout in ((nbr, True, 16), (dnbr, False, 32)):
        assert n.shape == (27, 0)
        f = torch.zeros(0, 16, device=dev, requires_grad=True)
        w = torch.randn(27, 16, cout, device=dev, requires_grad=True)
        out = ops.spconv_fwd(f, w, n, subm=subm)
        assert out.shape == (0, cout)
        (out.sum() + 0 * w.sum()).backward()
        assert f.grad.shape == (0, 16) and torch.equal(w.grad, torch.zeros_like(w))


def test_lopsided_batch(dev):
    """One frame of 40k points, one of 400: the small frame's rows sit at the end of every level."""
    levels = _walk(_level1([40000, 400], 2), 2, dev)
    for li, cin, cout in ((0, 16, 16), (1, 32, 32)):
        L = levels[li]
        b = L["idx"][:, 0]
        assert 0 < int((b == 1).sum()) < int((b == 0).sum()) // 20
        _check_conv(L["subm"], L["rows"], cin, cout, True, dev, seed=li + 11)
        _check_conv(L["down"], L["rows"], cin, 2 * cout, False, dev, seed=li + 13)


# ------------------------------------------------------------------------------------------------ the whole encoder
def _ref_spconv_fwd(feats, weight, nbr, alpha=None, beta=None, residual=None, relu=False, pair_counts=None, packed=None,
                    rows_dev=None, tiles=None, subm=False):
    out = conv_ref_autograd(nbr, feats, weight)
    if alpha is not None:
        out = out * alpha
    if beta is not None:
        out = out + beta
    if residual is not None:
        out = out + residual
    return torch.relu(out) if relu else out


def _ref_densify(feats, indices, batch, spatial_shape):
    i = indices.long()
    D, H, W = spatial_shape
    dense = feats.new_zeros(batch, D, H, W, feats.shape[1]).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), feats)
    return dense.permute(0, 4, 1, 2, 3).contiguous()


def test_sparse_encoder_train_mode_matches_float64(dev, monkeypatch):
    """nusc_L SparseEncoderCustom in train mode (BatchNorm1d on batch statistics) at bs = 2: the 21 conv weight gradients
    and the input-feature gradient against the same module in float64 whose convolutions and dense() are conv_ref /
    index_put (the rulebooks are the same bitmap-rank tables: they depend on the coordinates alone).

    The float64 run replays the ReLU masks of the kernel run.  With its own masks it would differ by more than rounding: a
    pre-activation within float32 rounding of zero flips its mask, and one flipped element moves a weight gradient by one
    term, while batch-statistics BatchNorm leaves that gradient a sum with heavy cancellation (its maximum grows like the
    square root of the 150k rows, not like the row count).  Measured on this module: up to 2.3e-3 of max|ref| from the
    kernels and up to 3.5e-3 from torch's own float32 ops, both against float64 with its own masks.  With the masks shared
    the two runs compute the same piecewise-linear function.  So that a wrong forward cannot hide behind the replay, the
    masks float64 would have set otherwise are bounded above: at most one element in a million (19 in 113 million were
    measured), each with a pre-activation within 1e-5 of zero (7e-7 at most was measured)."""
    import srfdet3d_amd  # noqa: F401  registers the modules
    from srfdet3d_amd import workloads
    from srfdet3d_amd.compat.registry import build_middle_encoder
    with torch.random.fork_rng(devices=[dev]):   # the weight init draws from the global generators: leave them as found
        torch.manual_seed(0)
        enc = build_middle_encoder(workloads.model_cfg("srfdet_voxel_nusc_L")["pts_middle_encoder"]).to(dev).train()
    enc64 = copy.deepcopy(enc).double()
    coors = torch.from_numpy(_level1(30000, 2)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    feats = torch.randn(coors.shape[0], 5, generator=gen, device=dev)
    relu = torch.nn.ReLU.forward
    masks, seen = [], dict(flips=0, total=0, flip_pre=0.0)

    def record(self, x):
        masks.append(x.detach() > 0)
        return relu(self, x)

    def replay(self, x):
        m = masks.pop(0)
        flip = (x.detach() > 0) != m
        seen["flips"] += int(flip.sum())
        seen["flip_pre"] = max(seen["flip_pre"], float(x.detach().abs()[flip].max())) if flip.any() else seen["flip_pre"]
        seen["total"] += m.numel()
        return x * m

    def run(m, x):
        x = x.clone().requires_grad_(True)
        bev = m(x, coors, 2)
        g = torch.randn(bev.shape, generator=torch.Generator(device=dev).manual_seed(2), device=dev, dtype=torch.float32)
        (bev * g.to(bev.dtype)).sum().backward()
        ws = {k: p.grad for k, p in m.named_parameters() if k.endswith("weight") and p.dim() >= 3}
        return bev.detach(), x.grad, ws

    monkeypatch.setattr(torch.nn.ReLU, "forward", record)
    bev, gx, gw = run(enc, feats)
    n_relu = len(masks)
    monkeypatch.setattr(ops, "spconv_fwd", _ref_spconv_fwd)
    monkeypatch.setattr(ops, "densify", _ref_densify)
    monkeypatch.setattr(torch.nn.ReLU, "forward", replay)
    bev64, gx64, gw64 = run(enc64, feats.double())
    monkeypatch.undo()
    assert n_relu == 21 and not masks                     # every conv is followed by one ReLU; each mask used once
    assert seen["flips"] <= 1e-6 * seen["total"] and seen["flip_pre"] <= 1e-5, seen
    assert len(gw) == 21 and gw.keys() == gw64.keys()
    assert (bev - bev64).abs().max() <= 1e-4 * bev64.abs().max()
    worst = 0.0
    for k, ref in list(gw64.items()) + [("input", gx64)]:
        got = gw[k] if k != "input" else gx
        assert got is not None and ref.abs().max() > 0, k
        e = ((got.double() - ref).abs().max() / ref.abs().max()).item()
        assert e <= 1e-3, f"{k}: {e:.3e}"
        worst = max(worst, e)
    print(f"\nencoder: worst max|got - ref| / max|ref| over the 22 gradients {worst:.2e}; float64 would flip {seen['flips']} of "
          f"{seen['total']} ReLU masks (largest |pre-activation| among them {seen['flip_pre']:.1e})")


# ------------------------------------------------------------------------------------------------ RoI gather backward
IMG_STRIDES, BEV_STRIDES, FINEST = [4, 8, 16, 32], [8, 16, 32, 64], 56.0
P, SR = 7, 2


ROI_BWD_TOL = 1e-5         # |gradient - float64 gradient| over the sum of |weight * output gradient| of the element


def _roi_grad_ref(shapes, strides, rois, lv, g_bm, dev, chunk=64):
    """float64 gradient of the gather w.r.t. each map, channels-last (N, H, W, C), and its magnitude sums, on the level `lv`
    the kernel chose (tests/roi_ref.py: the geometry in float32 op by op as csrc/roi.hip forms it, mmcv's RoIAlign(aligned)
    rules, float64 from the sample point on).  g_bm: (R, P*P, C) output gradient in bin-major form."""
    return grad64(shapes, strides, rois, g_bm, P, SR, FINEST, lv=lv, dev=dev, chunk=chunk)


def _mmdet_level(rois, nl):
    """mmdet SingleRoIExtractor.map_roi_levels in float64 -> (level, near a boundary)."""
    r = rois.double()
    t = torch.log2(torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / FINEST + 1e-6)
    near = ((t - t.round()).abs() < 1e-4) & (t.round() >= 1) & (t.round() <= nl - 1)
    return t.floor().clamp(0, nl - 1).long(), near


def _run_variants(maps, rois, strides, g_bm, dev):
    """The feature-map gradients of roi_extract_autograd for (bin_major, channels-last) in all four combinations;
    returned channels-last (N, H, W, C) so that they compare directly."""
    out = {}
    for bin_major in (True, False):
        for cl in (True, False):
            fs = [m.to(dev).contiguous(memory_format=torch.channels_last) if cl else m.to(dev).contiguous() for m in maps]
            fs = [f.detach().requires_grad_(True) for f in fs]
            y = ops.roi_extract_autograd(fs, rois.to(dev), strides, P, SR, FINEST, bin_major=bin_major)
            R, C = rois.shape[0], maps[0].shape[1]
            g = g_bm if bin_major else g_bm.view(R, P, P, C).permute(0, 3, 1, 2)
            y.backward(g.contiguous())
            out[(bin_major, cl)] = [f.grad.permute(0, 2, 3, 1) for f in fs]
    return out


def _levels_of(maps, rois, strides, dev):
    return ops.roi_extract([m.to(dev) for m in maps], rois.to(dev), strides, P, SR, FINEST, return_levels=True)[1].cpu()


def _edge_rois(N, extent):
    """wholly outside, straddling the border (two corners), zero-size, very large (coarsest level), n < 0, n >= N."""
    e = float(extent)
    return torch.tensor([[0, e + 50, e + 60, e + 200, e + 180], [N - 1, -300, -250, -100, -90],
                         [0, -40, -30, 40, 50], [N - 1, e - 60, e - 30, e + 70, e + 90],
                         [0, 100, 50, 100, 50], [N - 1, 33.3, 21.7, 33.3, 21.7],
                         [0, -500, -400, e + 600, e + 500], [-1, 10, 10, 90, 80], [N, 10, 10, 90, 80], [N + 5, 5, 5, 300, 280]],
                        dtype=torch.float32)


def _random_rois(g, n, N, extent, batch_idx=None):
    c = torch.rand(n, 2, generator=g) * (extent * 1.2) - extent * 0.1
    wh = torch.exp(torch.rand(n, 2, generator=g) * (np.log(700.0) - np.log(4.0)) + np.log(4.0))
    bi = batch_idx if batch_idx is not None else torch.randint(0, N, (n,), generator=g)
    return torch.cat([bi.float()[:, None], c - wh / 2, c + wh / 2], 1)


def test_roi_extract_backward_training_form(dev):
    """2 x 200 BEV RoIs on four 128-channel BEV maps and 600 image RoIs over 12 images (n_cam 6 x bs 2), with the edge RoIs,
    against the float64 gradient; the four (bin_major, layout) variants of the call agree with it alike."""
    g = torch.Generator().manual_seed(0)
    C = 128
    cases = []
    bev_shapes = [(2, 64 >> l, 64 >> l) for l in range(4)]                   # level 0 covers 512 x 512 BEV pixels
    rb = torch.cat([_random_rois(g, 400, 2, 512, torch.arange(400) // 200), _edge_rois(2, 512)])
    cases.append(("bev", bev_shapes, BEV_STRIDES, rb))
    img_shapes = [(12, 48 >> l, 80 >> l) for l in range(4)]                  # level 0 covers 192 x 320 image pixels
    ri = torch.cat([_random_rois(g, 600, 12, 256, torch.arange(600) % 12), _edge_rois(12, 256)])
    cases.append(("img", img_shapes, IMG_STRIDES, ri))
    for name, shapes, strides, rois in cases:
        maps = [torch.randn(N, C, H, W, generator=g) for N, H, W in shapes]
        lv = _levels_of(maps, rois, strides, dev)
        want, near = _mmdet_level(rois, len(strides))
        assert torch.equal(lv[~near], want[~near]), name
        assert len(set(lv.tolist())) == 4 and int(near.sum()) < 5, name
        gb = torch.randn(rois.shape[0], P * P, C, generator=g).to(dev)
        ref, mag = _roi_grad_ref(shapes, strides, rois, lv, gb, dev)
        worst = 0.0
        for key, got in _run_variants(maps, rois, strides, gb, dev).items():
            for l in range(4):
                assert ref[l].abs().sum() > 0
                err = ((got[l].double() - ref[l]).abs() / mag[l].clamp_min(1e-300)).max().item()
                assert err <= ROI_BWD_TOL, f"{name} bin_major/channels_last {key} level {l}: {err:.3e}"
                worst = max(worst, err)
        print(f"\nroi bwd {name}: {rois.shape[0]} RoIs, levels {torch.bincount(lv, minlength=4).tolist()}, worst normalised error "
              f"{worst:.2e}")


def _exact_rois(g, n, N, shapes, strides):
    """RoIs whose sample points all fall on multiples of 1/4 in feature coordinates: corners on the level's pixel grid (x1 =
    k - 0.5 after the half-pixel shift) and bins 1, 2 or 3 feature pixels wide; the (bin width, bin height) pairs keep each
    RoI well inside its level's area range."""
    fit = {0: [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 3), (3, 2), (3, 3)], 1: [(2, 3), (3, 2), (3, 3)],
           2: [(2, 3), (3, 2), (3, 3)], 3: [(2, 3), (3, 2), (3, 3)]}
    out, want = [], []
    for i in range(n):
        l = i % 4
        _, H, W = shapes[l]
        s = strides[l]
        bw, bh = fit[l][int(torch.randint(0, len(fit[l]), (1,), generator=g))]
        # some reach past the border on either side (on the coarse levels most do: the maps are small)
        kx = int(torch.randint(-3, max(W - 7 * bw, 0) + 4, (1,), generator=g))
        ky = int(torch.randint(-3, max(H - 7 * bh, 0) + 4, (1,), generator=g))
        out.append([i % N, kx * s, ky * s, (kx + 7 * bw) * s, (ky + 7 * bh) * s])
        want.append(l)
    return torch.tensor(out, dtype=torch.float32), torch.tensor(want)


def test_roi_extract_backward_exact(dev):
    """Integer output gradients and RoIs whose bilinear weights are multiples of 1/16: every product and every atomic add
    is exact, so the kernel must equal the float64 gradient bit for bit, in all four call variants."""
    g = torch.Generator().manual_seed(1)
    C = 128
    shapes = [(12, 48 >> l, 80 >> l) for l in range(4)]
    maps = [torch.randn(N, C, H, W, generator=g) for N, H, W in shapes]
    rois, want = _exact_rois(g, 480, 12, shapes, IMG_STRIDES)
    lv = _levels_of(maps, rois, IMG_STRIDES, dev)
    assert torch.equal(lv, want)
    gb = torch.randint(-3, 4, (rois.shape[0], P * P, C), generator=g).float().to(dev)
    ref, _ = _roi_grad_ref(shapes, IMG_STRIDES, rois, lv, gb, dev)
    for key, got in _run_variants(maps, rois, IMG_STRIDES, gb, dev).items():
        for l in range(4):
            assert ref[l].abs().sum() > 0
            d = (got[l].double() - ref[l]).abs().max().item()
            assert d == 0, f"bin_major/channels_last {key} level {l}: {d}"
