"""`srf_pillar_vfe` and `srf_pillar_scatter_nhwc` (csrc/pillar.hip) on the GPU against the definition in tests/pillar_ref.py, the
reference's fixture, `ops.densify` and the torch route of the modules (SRF_PILLAR=0)."""
import copy
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import detgen
import pillar_ref as R
from srfdet3d_amd import nhwc, ops, synthetic as S, workloads
from srfdet3d_amd.plugin.pillar import PillarFeatureNetCustom

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "fusion_nusc.npz"))
VOXEL, RANGE = [0.2, 0.2, 8], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
OFFSET = [VOXEL[d] / 2 + RANGE[d] for d in range(3)]


def run(dev, vox, num, coors, W, scale, shift, voxel, offset, cluster=True, centre=True, legacy=False, rows_dev=None):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    out = ops.pillar_vfe(t(vox, torch.float32), t(num, torch.int32), t(coors, torch.int32), t(W, torch.float32), t(scale, torch.float32),
                         t(shift, torch.float32), voxel, offset, cluster, centre, legacy,
                         None if rows_dev is None else torch.tensor([rows_dev], dtype=torch.int32, device=dev))
    return out.cpu().numpy()


def integer_case(rows, P, nf, cout, seed, cluster=True, num=None):
    """Small integers whose per-pillar coordinate sums are multiples of n (the mean is an integer), integer weights, scale 1, integer shift,
    voxel sizes and offsets that are powers of two: every intermediate of the definition is exact in float32."""
    rng = np.random.default_rng(seed)
    num = (np.arange(rows) % P + 1).astype(np.int32) if num is None else np.asarray(num, np.int32)
    vox = rng.integers(-4, 5, (rows, P, nf)).astype(np.int64)
    for r in range(rows):
        n = int(num[r])
        vox[r, n - 1, :3] -= vox[r, :n, :3].sum(0) % n       # the last live point makes each coordinate sum a multiple of n
        vox[r, n:] = 0
    coors = np.stack([np.zeros(rows), rng.integers(0, 4, rows), rng.integers(0, 16, rows), rng.integers(0, 16, rows)], 1).astype(np.int32)
    K = nf + 3 * cluster + 3
    W = rng.integers(-2, 3, (cout, K)).astype(np.float32)
    shift = rng.integers(-3, 4, cout).astype(np.float32)
    return vox.astype(np.float32), num, coors, W, np.ones(cout, np.float32), shift


@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("nf", [4, 5])
@pytest.mark.parametrize("P", [1, 5, 20])
@pytest.mark.parametrize("rows", [1, 257])
def test_exact_on_integers(dev, rows, P, nf, cout):
    """rows = 257: the last work item of four pillars holds one, the last workgroup of four waves one wave."""
    voxel, offset = [0.5, 0.25, 2.0], [0.25, -8.0, 1.0]
    for legacy in (False, True):
        vox, num, coors, W, scale, shift = integer_case(rows, P, nf, cout, 1000 * rows + 10 * P + nf + legacy)
        want, _ = R.pillar_vfe(vox, num, coors, voxel, offset, W, scale, shift, True, True, legacy)
        assert np.array_equal(want * 8, np.round(want * 8)) and np.abs(want).max() < 2 ** 16     # on a grid float32 holds exactly
        got = run(dev, vox, num, coors, W, scale, shift, voxel, offset, True, True, legacy)
        assert np.array_equal(got.astype(np.float64), want)


def random_case(rows, P, nf, cout, seed):
    rng = np.random.default_rng(seed)
    coors = np.stack([np.zeros(rows), np.zeros(rows), rng.integers(0, 512, rows), rng.integers(0, 512, rows)], 1).astype(np.int32)
    num = (np.arange(rows) % P + 1).astype(np.int32)
    vox = rng.uniform(0, 1, (rows, P, nf))
    vox[:, :, 0] = RANGE[0] + (coors[:, 3:4] + rng.uniform(0.02, 0.98, (rows, P))) * VOXEL[0]
    vox[:, :, 1] = RANGE[1] + (coors[:, 2:3] + rng.uniform(0.02, 0.98, (rows, P))) * VOXEL[1]
    vox[:, :, 2] = rng.uniform(RANGE[2], RANGE[5], (rows, P))
    vox = (vox * (np.arange(P)[None, :, None] < num[:, None, None])).astype(np.float32)
    W = rng.standard_normal((cout, nf + 6)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32) * rng.choice([-1, 1], cout).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    return vox, num, coors, W, scale, shift


def test_random_data_within_the_fma_chain_bound(dev):
    """K chained fmas, the fma of the epilogue and one rounding to spare: gamma_{K+2} times the magnitude of the point that attains the max."""
    rows, P, nf, cout = 300, 20, 5, 64
    vox, num, coors, W, scale, shift = random_case(rows, P, nf, cout, 5)
    want, mag = R.pillar_vfe(vox, num, coors, VOXEL, OFFSET, W, scale, shift, True, True, False)
    got = run(dev, vox, num, coors, W, scale, shift, VOXEL, OFFSET, True, True, False)
    again = run(dev, vox, num, coors, W, scale, shift, VOXEL, OFFSET, True, True, False)
    bound = R.gamma(nf + 6 + 2) * mag
    err = np.abs(got.astype(np.float64) - want)
    print(f"pillar_vfe 300 x 20 x 5 -> 64: worst error / bound = {np.max(err / bound):.4f}")
    assert (err <= bound).all()
    assert got.tobytes() == again.tobytes()


def test_voxel_centre_is_a_product_and_a_sum_not_an_fma(dev):
    """With v = 0.2 and offset 0.1 - 51.2 the two-rounding centre and the fused one differ for some cells; the kernel must give the first.
    The centre is read back through a weight that picks the three x - c features (scale 1, shift 0) of one point at the origin per pillar:
    out = 0 - c, positive on this side of the grid, so the ReLU passes it."""
    idx = np.arange(256)
    v32, o32 = np.float32(0.2), np.float32(OFFSET[0])
    two = (idx.astype(np.float32) * v32).astype(np.float32) + o32
    fused = (idx.astype(np.float64) * np.float64(v32) + np.float64(o32)).astype(np.float32)   # i * v is exact in float64: one rounding
    assert two.dtype == np.float32 and (two != fused).sum() >= 8 and (two < 0).all()
    rows, nf, cout = len(idx), 4, 64
    coors = np.stack([np.zeros(rows), idx[::-1], (idx * 7) % 256, idx], 1).astype(np.int32)
    W = np.zeros((cout, nf + 3), np.float32)
    W[0, nf], W[1, nf + 1], W[2, nf + 2] = 1, 1, 1
    vox = np.zeros((rows, 1, nf), np.float32)
    got = run(dev, vox, np.ones(rows, np.int32), coors, W, np.ones(cout, np.float32), np.zeros(cout, np.float32), [0.2, 0.2, 0.2],
              [OFFSET[0]] * 3, False, True, False)
    for d, col in enumerate((3, 2, 1)):
        assert np.array_equal(got[:, d], -two[coors[:, col]]), "xyz"[d]
    assert (got[:, 3:] == 0).all()


def test_padded_slots_and_both_signs_of_shift(dev):
    """Every real activation is negative.  n < P: the padded slots give relu(shift); n == P: the shift must not enter, the result is 0."""
    rows, P, nf, cout = 12, 4, 4, 64
    num = (np.arange(rows) % P + 1).astype(np.int32)
    vox = np.zeros((rows, P, nf), np.float32)
    vox[:, :, 3] = np.arange(1, P + 1)[None, :] * 4.0
    vox *= (np.arange(P)[None, :, None] < num[:, None, None])
    W = np.zeros((cout, nf), np.float32)
    W[:, 3] = -1.0
    shift = np.where(np.arange(cout) % 2 == 0, 0.5, -0.5).astype(np.float32)
    coors = np.zeros((rows, 4), np.int32)
    got = run(dev, vox, num, coors, W, np.ones(cout, np.float32), shift, VOXEL, OFFSET, False, False, False)
    want, _ = R.pillar_vfe(vox, num, coors, VOXEL, OFFSET, W, np.ones(cout), shift, False, False, False)
    assert np.array_equal(got, want)
    assert (got[num < P] == np.maximum(shift, 0)[None, :]).all() and (got[num == P] == 0).all()


def test_nan_and_infinities(dev):
    rows, P, nf, cout = 8, 5, 5, 64
    vox, num, coors, W, scale, shift = integer_case(rows, P, nf, cout, 77, num=[3, 5, 2, 5, 4, 1, 5, 3])
    vox[0, 1, 3] = np.nan          # a feature of a middle point
    vox[1, 4, 0] = np.inf          # a coordinate: the mean and every x - mean of the pillar
    vox[2, 0, 4] = -np.inf
    vox[3, 0, 3] = np.nan          # the first point of a full pillar
    vox[4, 3, 2] = -np.inf
    voxel, offset = [0.5, 0.25, 2.0], [0.25, -8.0, 1.0]
    want, _ = R.pillar_vfe(vox, num, coors, voxel, offset, W, scale, shift, True, True, False)
    got = run(dev, vox, num, coors, W, scale, shift, voxel, offset, True, True, False)
    assert np.isnan(want[0]).any() and np.isnan(want[3]).any() and np.isinf(want).any()
    assert np.array_equal(got.astype(np.float64), want, equal_nan=True)


@pytest.fixture(scope="module")
def sweep(dev):
    pts = torch.from_numpy(S.nuscenes_sweep(2000)).to(dev)
    static = ops.hard_voxelize(pts, VOXEL, RANGE, 20, 40000, static=True)
    plain = ops.hard_voxelize(pts, VOXEL, RANGE, 20, 40000)
    return pts, static, plain


def test_static_voxelization_feeds_straight_in(dev, sweep):
    _, (voxels, coors4, num, _, vnum), (v, c3, n, _) = sweep
    M, rows = int(vnum.item()), voxels.shape[0]
    assert 0 < M < rows and v.shape[0] == M
    vox, nn_, coors, W, scale, shift = random_case(4, 20, 5, 64, 9)
    t = lambda a: torch.from_numpy(a).to(dev)
    args = (t(W), t(scale), t(shift), VOXEL, OFFSET, True, True, False)
    full = ops.pillar_vfe(voxels, num, coors4, *args)
    live = ops.pillar_vfe(v, n, F.pad(c3, (1, 0), value=0).contiguous(), *args)
    assert torch.equal(full[:M], live) and live.abs().max() > 0
    assert (full[M:] == 0).all()
    counted = ops.pillar_vfe(voxels, num, coors4, *args, rows_dev=vnum)
    assert torch.equal(counted, full)
    half = ops.pillar_vfe(voxels, num, coors4, *args, rows_dev=torch.tensor([M // 2], dtype=torch.int32, device=dev))
    assert torch.equal(half[:M // 2], full[:M // 2]) and (half[M // 2:] == 0).all()


def _raise(name):
    def f(*a, **k):
        raise AssertionError(f"{name} was called: the encoder left the HIP kernel")
    return f


TORCH_OPS = ("linear", "batch_norm", "relu")


def test_reference_fixture_through_the_module(dev, monkeypatch):
    monkeypatch.delenv("SRF_PILLAR", raising=False)
    pfn = PillarFeatureNetCustom(in_channels=5, feat_channels=[64], with_distance=False, voxel_size=VOXEL,
                                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), point_cloud_range=RANGE, legacy=False).eval()
    detgen.load_det_params(pfn, "pfn.")
    pfn = pfn.to(dev)
    Np, Mp = 60, 20
    num = (np.arange(Np) % Mp + 1).astype(np.int32)
    vox = (detgen.det("pfn.voxels", (Np, Mp, 5)) * (np.arange(Mp)[None, :, None] < num[:, None, None])).astype(np.float32)
    pc = np.stack([np.zeros(Np), np.zeros(Np), np.arange(Np) % 512, (np.arange(Np) * 7) % 512], 1).astype(np.int32)
    args = [torch.from_numpy(a).to(dev) for a in (vox, num, pc)]
    with monkeypatch.context() as mp, torch.no_grad():
        for fn in TORCH_OPS:
            mp.setattr(F, fn, _raise("F." + fn))
        mp.setattr(torch, "cat", _raise("torch.cat"))
        out = pfn(*args)
    np.testing.assert_allclose(out.cpu().numpy(), GOLD["pfn.out"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("H,W,rows", [(7, 9, 100), (512, 512, 3000)])
def test_scatter_is_densify_bit_for_bit(dev, H, W, rows):
    B, C = 2, 64
    rng = np.random.default_rng(H)
    cells = rng.choice(B * H * W, rows, replace=False)                 # distinct, as the voxelization makes them
    coors = np.stack([cells // (H * W), rng.integers(0, 5, rows), cells // W % H, cells % W], 1).astype(np.int32)
    coors[rng.choice(rows, rows // 10, replace=False)] = -1            # padding rows in between
    live = rows - rows // 7
    feats = torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)).to(dev)
    feats[3, 5] = -0.0
    c_dev = torch.from_numpy(coors).to(dev)
    garbage = torch.full((B, C, H, W), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
    got = ops.pillar_scatter_nhwc(feats, c_dev, B, H, W, rows_dev=torch.tensor([live], dtype=torch.int32, device=dev), out=garbage)
    assert got.data_ptr() == garbage.data_ptr() and got.shape == (B, C, H, W) and got.stride() == (H * W * C, 1, W * C, C)
    ref_c = coors.copy()
    ref_c[live:] = -1
    ref_c[:, 1] = np.where(ref_c[:, 0] < 0, -1, 0)
    want = ops.densify(feats, torch.from_numpy(ref_c).to(dev), B, [1, H, W]).view(B, C, H, W)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))    # bits, element by element (-0.0 included)
    used = np.zeros((B, H, W), bool)
    keep = ref_c[:, 0] >= 0
    used[ref_c[keep, 0], ref_c[keep, 2], ref_c[keep, 3]] = True
    assert used.sum() == keep.sum() and (got.cpu().numpy().transpose(0, 2, 3, 1)[~used].view(np.int32) == 0).all()
    fresh = ops.pillar_scatter_nhwc(feats[:live], c_dev[:live], B, H, W)
    assert nhwc.is_channels_last(fresh) and torch.equal(fresh, got)


@pytest.fixture(scope="module")
def model(dev):
    torch.manual_seed(0)
    return workloads.build("srfdet_pillar_nusc_L", 64).eval().to(dev)


def torch_route_bound(enc, vox, num, coors):
    """|HIP route - SRF_PILLAR=0 route| per output, both against the definition d (float64 on the float32 decoration):
      HIP:   gamma_{K+2} m                                     (the test above)
      torch: the cluster means differ (another summation order): 2 gamma_P A + 2 u |x - mean| on those three features, through
             |scale_c| sum_k |w_ck| delta_k; a float32 GEMM in any order: gamma_K |scale_c| sum_k |x_k w_ck|; the unfolded BatchNorm
             ((acc - mean) * invstd * gamma + beta, against acc * scale + shift with scale and shift rounded once each): five more roundings
             on |acc scale| + |mean scale| + |beta|
    per point, m = |scale_c| sum_k |x_k w_ck| + |shift_c|; the max over a pillar moves by at most the largest per-point bound."""
    pfn = enc.pfn_layers[0]
    bn = pfn.norm
    W = pfn.linear.weight.detach().double().cpu().numpy()
    scale = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu().numpy()
    rm_s = np.abs(bn.running_mean.double().cpu().numpy() * scale)
    beta = np.abs(bn.bias.detach().double().cpu().numpy())
    shift = bn.bias.detach().double().cpu().numpy() - bn.running_mean.double().cpu().numpy() * scale
    nf, P = vox.shape[2], vox.shape[1]
    K = W.shape[1]
    x = R.decorate(vox, num, coors, VOXEL, OFFSET, True, True, enc.legacy).astype(np.float64)
    live = (np.arange(P)[None, :] < num[:, None])[:, :, None]
    A = np.abs(vox[:, :, :3].astype(np.float64)).sum(1, keepdims=True) / np.maximum(num, 1)[:, None, None]
    delta = np.zeros_like(x)
    delta[:, :, nf:nf + 3] = (2 * R.gamma(P) * A + 2 * R.U32 * np.abs(x[:, :, nf:nf + 3])) * live
    xw = np.einsum("rpk,ck->rpc", np.abs(x), np.abs(W)) * np.abs(scale)
    per_point = (R.gamma(K + 2) * (xw + np.abs(shift)) + R.gamma(K + 5) * (xw + rm_s + beta)
                 + np.einsum("rpk,ck->rpc", delta, np.abs(W)) * np.abs(scale))
    return per_point.max(axis=1)      # the padded slots (x = 0) are among the points: their bound is the shift's


def test_module_level_on_the_pillar_config(dev, model, sweep, monkeypatch):
    pts = sweep[0]
    enc = model.pts_voxel_encoder
    with torch.no_grad():
        voxels, num, coors = model.voxelize([pts])
        monkeypatch.setenv("SRF_PILLAR", "0")
        old = enc(voxels, num, coors)
        canvas_old = model.pts_middle_encoder(old, coors, 1)
        with monkeypatch.context() as mp:                      # the old route hands SECOND an NCHW canvas, which it transposes
            mp.setattr(ops, "to_channels_last", _raise("ops.to_channels_last"))
            with pytest.raises(AssertionError, match="to_channels_last"):
                model.extract_point_features([pts])
        with monkeypatch.context() as mp:
            mp.setattr(F, "linear", _raise("F.linear"))
            with pytest.raises(AssertionError, match="F.linear"):
                enc(voxels, num, coors)
        monkeypatch.delenv("SRF_PILLAR")
        with monkeypatch.context() as mp:
            for fn in TORCH_OPS:
                mp.setattr(F, fn, _raise("F." + fn))
            new = enc(voxels, num, coors)
        bound = torch_route_bound(enc, voxels.cpu().numpy(), num.cpu().numpy(), coors.cpu().numpy())
        err = np.abs(new.double().cpu().numpy() - old.double().cpu().numpy())
        print(f"srfdet_pillar_nusc_L encoder, {voxels.shape[0]} pillars: worst |HIP - torch| / bound = {np.max(err / bound):.4f}")
        assert (err <= bound).all()
        canvas = model.pts_middle_encoder(new, coors, 1)
        assert nhwc.is_channels_last(canvas) and not nhwc.is_channels_last(canvas_old)
        seen = []
        hook = model.pts_backbone.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
        with monkeypatch.context() as mp:
            mp.setattr(ops, "to_channels_last", _raise("ops.to_channels_last"))
            feats = model.extract_point_features([pts])
        hook.remove()
        assert len(seen) == 1 and nhwc.is_channels_last(seen[0]) and seen[0].shape == (1, 64, 512, 512)
        feats = [feats] if torch.is_tensor(feats) else list(feats)
        assert torch.equal(seen[0], canvas) and all(torch.isfinite(f).all() for f in feats)
    # autograd: the torch route
    p = enc.pfn_layers[0].linear.weight
    p.requires_grad_(True)
    try:
        with torch.enable_grad(), monkeypatch.context() as mp:
            mp.setattr(F, "linear", _raise("F.linear"))
            with pytest.raises(AssertionError, match="F.linear"):
                enc(voxels, num, coors)
        with torch.enable_grad():
            assert enc(voxels, num, coors).requires_grad
    finally:
        p.requires_grad_(False)


def test_derived_state_follows_weights_changed(dev, model, sweep, monkeypatch):
    monkeypatch.delenv("SRF_PILLAR", raising=False)
    enc = model.pts_voxel_encoder
    bn = enc.pfn_layers[0].norm
    with torch.no_grad():
        voxels, num, coors = model.voxelize([sweep[0]])
        before = enc(voxels, num, coors)
        saved = bn.weight.data.clone(), bn.running_mean.data.clone()
        try:
            bn.weight.data.mul_(1.5)                 # through .data: neither a version nor a pointer changes
            bn.running_mean.data.add_(0.25)
            model.weights_changed()
            after = enc(voxels, num, coors)
            fresh = copy.deepcopy(enc)
            fresh.__dict__.pop("_srf_derived", None)
            for m in fresh.modules():
                m.__dict__.pop("_srf_derived", None)
            want = fresh(voxels, num, coors)
        finally:
            bn.weight.data.copy_(saved[0]), bn.running_mean.data.copy_(saved[1])
            model.weights_changed()
    assert torch.equal(after, want) and not torch.equal(after, before)
