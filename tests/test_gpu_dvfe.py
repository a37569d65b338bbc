"""`srf_dvfe_fwd` (csrc/dvfe.hip) on the GPU against the definition in tests/dvfe_ref.py: exact on integers, inside the running bound on
random data, the pinned arithmetic of the decoration, non-finite input, empty input, and `DynamicVFECustom` of the five dynamic-voxelization
configs on both routes (SRF_DVFE=0: the torch route).

T, the float32 ulps one tanh may be off, is not a constant of this file: `measure_T` takes it from `torch.tanh` on the GPU (the arithmetic
of the route the kernel replaces) over the very arguments the case produces -- twice its worst error against float64, at least 1 ulp."""
import numpy as np
import pytest
import torch

import dvfe_ref as R
from srfdet3d_amd import ops, synthetic as S, workloads
from srfdet3d_amd.plugin.voxel_encoders import DynamicVFECustom

pytestmark = pytest.mark.gpu

POW2_VOXEL, POW2_OFFSET = [0.5, 0.25, 2.0], [0.25, -8.0, 1.0]
KITTI = ([0.05, 0.05, 0.1], [0.0, -40.0, -3.0, 70.4, 40.0, 1.0])
WAYMO = ([0.1, 0.1, 0.15], [-76.8, -76.8, -2.0, 76.8, 76.8, 4.0])


def measure_T(dev, args):
    """twice the worst error of torch.tanh on the GPU, in float32 ulps of the true value, over `args` (float32); at least 1"""
    args = args[np.isfinite(args)]
    if args.size == 0:
        return 1.0
    got = torch.tanh(torch.from_numpy(args).to(dev)).cpu().numpy().astype(np.float64)
    true = np.tanh(args.astype(np.float64))
    worst = float(np.max(np.abs(got - true) / R.ulp32(true)))
    return max(1.0, 2.0 * worst)


def reference(dev, case):
    """the definition with the T measured on this case's own tanh arguments"""
    first = R.dvfe(*case, T=1.0)
    T = measure_T(dev, first["tanh_args"])
    return R.dvfe(*case, T=T), T


def run(dev, case, grid_zyx, batch, static_rows=None):
    pts, coors, voxel, offset, centre, pos_enc, layers = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    vm = ops.VoxelMap(torch.from_numpy(np.ascontiguousarray(coors, np.int32)).to(dev), grid_zyx, batch, static_rows=static_rows)
    out = ops.dvfe(t(pts), vm, voxel, offset, centre, [t(a) for a in pos_enc], [[t(a) for a in l] for l in layers])
    torch.cuda.synchronize()
    return out.cpu().numpy(), vm


def integer_case(n, nf, widths, seed, d=32, centre=True):
    """Small integers whose per-voxel coordinate sums are multiples of the count (the mean is an integer), integer weights, scale 1, integer
    shifts, voxel sizes and offsets that are powers of two, W2 = 0 and shift2 = 0 (pos is exactly 0): every intermediate of the definition
    that reaches the output is exact in float32.  For n > 1: one voxel of 70 points, one of a single point, every fifth point dropped
    (coordinates -1) in between the others, two batch indices."""
    rng = np.random.default_rng(seed)
    vox_of = np.zeros(n, np.int64)
    if n > 1:
        nv = max(n // 5, 3)
        vox_of = rng.integers(2, nv, n)
        vox_of[rng.choice(n, 70, replace=False)] = 0           # more than a wave of points in one voxel
        vox_of[rng.choice(np.nonzero(vox_of != 0)[0])] = 1     # and one point alone in its voxel
    cells = rng.choice(2 * 4 * 16 * 16, int(vox_of.max()) + 1, replace=False)
    c = cells[vox_of]
    coors = np.stack([c // 1024, c // 256 % 4, c // 16 % 16, c % 16], 1).astype(np.int32)
    if n > 1:
        drop = np.arange(3, n, 5)
        drop = drop[(vox_of[drop] > 1)]
        coors[drop[::2]] = -1
        coors[drop[1::2], 1 + drop[1::2] % 3] = -1             # a -1 in any column drops the point
        assert len(set(coors[(coors >= 0).all(1), 0])) == 2
    pts = rng.integers(-4, 5, (n, nf)).astype(np.int64)
    keys = {}
    for i in range(n):
        if (coors[i] >= 0).all():
            keys.setdefault(tuple(coors[i]), []).append(i)
    for lst in keys.values():
        pts[lst[-1], :3] -= pts[lst, :3].sum(0) % len(lst)     # the last point makes each coordinate sum a multiple of the count
    f = np.float32
    pos_enc = (rng.integers(-2, 3, (d, 3)).astype(f), np.ones(d, f), rng.integers(-2, 3, d).astype(f), np.zeros((d, d), f), np.ones(d, f),
               np.zeros(d, f))
    layers, cin = [], nf + d + 3 * centre
    for w in widths:
        layers.append((rng.integers(-2, 3, (w, cin)).astype(f), np.ones(w, f), rng.integers(-3, 4, w).astype(f)))
        cin = 2 * w
    return pts.astype(f), coors, POW2_VOXEL, POW2_OFFSET, centre, pos_enc, layers


GRID = ([4, 16, 16], 2)


@pytest.mark.parametrize("widths", [(4,), (5, 5)])
@pytest.mark.parametrize("nf", [4, 5])
@pytest.mark.parametrize("n", [1, 257, 700])
def test_exact_on_integers(dev, n, nf, widths):
    """n = 257: the second workgroup of the point kernel holds one point; 700 points: three workgroups, the last one partly filled."""
    case = integer_case(n, nf, widths, 100 * n + 10 * nf + len(widths))
    want = R.dvfe(*case)
    assert np.array_equal(want["out"] * 4, np.round(want["out"] * 4)) and np.abs(want["out"]).max() < 2 ** 20   # float32 holds it exactly
    got, vm = run(dev, case, *GRID)
    M = len(want["coors"])
    assert vm.M == M and np.array_equal(vm.coors.cpu().numpy(), want["coors"])
    if n > 1:
        counts = np.bincount(want["point2voxel"][want["point2voxel"] >= 0])
        assert counts.max() > 64 and counts.min() == 1 and (want["point2voxel"] < 0).sum() >= n // 10
    assert np.array_equal(got.astype(np.float64), want["out"])
    # the static map: more rows than voxels, the live rows equal, the padding rows zero
    full, vms = run(dev, case, *GRID, static_rows=M + 37)
    assert full.shape == (min(M + 37, n), want["out"].shape[1]) and int(vms.num_dev.item()) == M
    assert np.array_equal(full[:M], got) and (full[M:].view(np.int32) == 0).all()


@pytest.mark.parametrize("d,nf,widths,centre", [(16, 3, (1,), False), (64, 8, (16, 16), True), (32, 6, (8, 3), False), (16, 4, (3, 16), True)])
def test_exact_on_integers_at_the_edges_of_the_domain(dev, d, nf, widths, centre):
    """every position-encoder width, the smallest and the largest feature and channel counts, with and without the voxel centre"""
    case = integer_case(300, nf, widths, d + nf, d=d, centre=centre)
    want = R.dvfe(*case)
    assert np.array_equal(want["out"] * 4, np.round(want["out"] * 4)) and np.abs(want["out"]).max() < 2 ** 20
    got, _ = run(dev, case, *GRID)
    assert np.array_equal(got.astype(np.float64), want["out"])


def random_case(n, n_vox, nf, widths, seed, d=32, voxel=WAYMO[0], pc_range=WAYMO[1], centre=True):
    """n points in about n_vox voxels of the grid, weights of the size a trained encoder has, folded BatchNorms of both signs"""
    rng = np.random.default_rng(seed)
    r, vs = np.asarray(pc_range, np.float64), np.asarray(voxel, np.float64)
    grid = np.round((r[3:] - r[:3]) / vs).astype(np.int64)                       # x, y, z
    cells = np.stack([rng.integers(0, grid[0], n_vox), rng.integers(0, grid[1], n_vox), rng.integers(0, grid[2], n_vox)], 1)
    pick = rng.integers(0, n_vox, n)
    c = cells[pick]
    xyz = r[:3] + (c + rng.uniform(0.05, 0.95, (n, 3))) * vs
    pts = np.concatenate([xyz, rng.uniform(0, 1, (n, nf - 3))], 1).astype(np.float32)
    coors = np.stack([rng.integers(0, 2, n_vox)[pick], c[:, 2], c[:, 1], c[:, 0]], 1).astype(np.int32)
    coors[rng.choice(n, n // 10, replace=False)] = -1
    f = np.float32
    lin = lambda co, ci: (rng.standard_normal((co, ci)) * np.sqrt(2.0 / (co + ci))).astype(f)
    bn = lambda co: ((rng.uniform(0.7, 1.4, co) * rng.choice([-1, 1], co)).astype(f), (rng.standard_normal(co) * 0.1).astype(f))
    pos_enc = (lin(d, 3) * f(20), *bn(d), lin(d, d), *bn(d))         # offsets inside a voxel are centimetres: a trained W1 is large
    layers, cin = [], nf + d + 3 * centre
    for w in widths:
        layers.append((lin(w, cin), *bn(w)))
        cin = 2 * w
    offset = [voxel[k] / 2 + pc_range[k] for k in range(3)]
    return (pts, coors, voxel, offset, centre, pos_enc, layers), ([int(grid[2]), int(grid[1]), int(grid[0])], 2)


@pytest.mark.parametrize("widths", [(5,), (5, 5)])
def test_random_data_inside_the_running_bound(dev, widths):
    case, grid = random_case(2000, 600, 5, widths, 11 + len(widths))
    want, T = reference(dev, case)
    got, vm = run(dev, case, *grid)
    again, _ = run(dev, case, *grid)
    assert np.array_equal(vm.coors.cpu().numpy(), want["coors"]) and 500 < vm.M <= 600
    err = np.abs(got.astype(np.float64) - want["out"])
    print(f"dvfe 2000 points, {vm.M} voxels, d = 32, layers {widths}: T = {T:.3f} ulp, worst error / bound = {np.max(err / want['bound']):.4f}, "
          f"worst error {err.max():.3e}, bound there {want['bound'].flat[err.argmax()]:.3e}")
    assert (err <= want["bound"]).all()
    assert got.tobytes() == again.tobytes()


def test_the_mean_is_the_sequential_float32_sum(dev):
    """Voxels of 8-40 points 70 m out: the float32 sum in point order and the correctly rounded mean differ in the last bits, W1 = 8 I
    (padded with zero rows) carries the difference into the net, and the bound -- which knows the sequential sum only -- must hold."""
    rng = np.random.default_rng(21)
    voxel, pc_range = KITTI
    n_vox, d, nf = 60, 32, 4
    counts = rng.integers(8, 41, n_vox)
    ix, iy, iz = rng.integers(1396, 1408, n_vox), rng.integers(0, 1600, n_vox), rng.integers(0, 40, n_vox)
    which = rng.permutation(np.repeat(np.arange(n_vox), counts))
    n = len(which)
    cell = np.stack([ix, iy, iz], 1)[which]
    xyz = np.asarray(pc_range[:3]) + (cell + rng.uniform(0.05, 0.95, (n, 3))) * np.asarray(voxel)
    pts = np.concatenate([xyz, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    coors = np.stack([np.zeros(n), cell[:, 2], cell[:, 1], cell[:, 0]], 1).astype(np.int32)
    vox, p2v, order, offsets, cnt = R.voxel_map(coors)
    seq = R.cluster_means(pts[:, :3], order, offsets, cnt)
    exact = np.stack([pts[p2v == m, :3].astype(np.float64).mean(0) for m in range(len(vox))]).astype(np.float32)
    assert len(vox) == n_vox and ((seq != exact).any(axis=1)).sum() >= 8 and np.abs(pts[:, 0]).min() > 69
    f = np.float32
    W1 = np.zeros((d, 3), f)
    W1[:3] = 8 * np.eye(3, dtype=f)
    base, grid = random_case(10, 5, nf, (4,), 22, voxel=voxel, pc_range=pc_range)
    _, _, _, offset, _, pe, layers = base
    case = (pts, coors, voxel, offset, True, (W1, np.ones(d, f), np.zeros(d, f), *pe[3:]), layers)
    want, T = reference(dev, case)
    got, _ = run(dev, case, grid[0], 1)
    err = np.abs(got.astype(np.float64) - want["out"])
    # what another summation order would change: the means move by an ulp of 70 (7.6e-6), times 8 through W1
    moved = R.dvfe(pts[::-1].copy(), coors[::-1].copy(), *case[2:], T=T)
    shift = np.abs(moved["out"] - want["out"])
    print(f"dvfe mean: T = {T:.3f}, worst error / bound = {np.max(err / want['bound']):.4f}; the reversed point order moves the output by up "
          f"to {shift.max():.3e}, {np.max(shift / want['bound']):.1f} bounds")
    assert (err <= want["bound"]).all()


@pytest.mark.parametrize("voxel,pc_range", [KITTI, WAYMO])
def test_voxel_centre_is_a_product_and_a_sum_not_an_fma(dev, voxel, pc_range):
    """With the configs' voxel sizes the two-rounding centre and the fused one differ for some cells; the kernel must give the first.  One point
    at the origin per voxel, W2 = 0 (pos = 0), and a first layer that picks +(xyz - c) and -(xyz - c) with scale 1 and shift 0: one of the two
    passes the ReLU, and their difference is -c exactly."""
    idx = np.arange(256)
    offset = [voxel[k] / 2 + pc_range[k] for k in range(3)]
    differ = 0
    for k in range(3):
        v32, o32 = np.float32(voxel[k]), np.float32(offset[k])
        fused = (idx.astype(np.float64) * np.float64(v32) + np.float64(o32)).astype(np.float32)   # i * v is exact in float64: one rounding
        differ += ((idx.astype(np.float32) * v32).astype(np.float32) + o32 != fused).sum()
    assert differ >= 8
    n, nf, d = len(idx), 4, 16
    coors = np.stack([np.zeros(n), idx[::-1], (idx * 7) % 256, idx], 1).astype(np.int32)
    f = np.float32
    Wa = np.zeros((6, nf + d + 3), f)
    for k in range(3):
        Wa[k, nf + d + k], Wa[3 + k, nf + d + k] = 1, -1
    pos_enc = (np.ones((d, 3), f), np.ones(d, f), np.zeros(d, f), np.zeros((d, d), f), np.ones(d, f), np.zeros(d, f))
    case = (np.zeros((n, nf), f), coors, voxel, offset, True, pos_enc, [(Wa, np.ones(6, f), np.zeros(6, f))])
    got, vm = run(dev, case, [256, 256, 256], 1)
    vc = vm.coors.cpu().numpy()
    two = R.centres(vc, voxel, offset)                     # (M, 3) x, y, z with the two roundings
    for k in range(3):
        assert np.array_equal(got[:, 3 + k] - got[:, k], two[:, k]), "xyz"[k]
        assert (np.minimum(got[:, k], got[:, 3 + k]) == 0).all()


def test_non_finite_input(dev):
    """A NaN feature, an infinite coordinate and an infinite feature in one point each of a voxel of several, and a voxel whose every point
    is NaN, on the integer case: equal to the definition everywhere, the -inf of the voxels without a single finite activation included."""
    for widths in ((4,), (5, 5)):
        case = integer_case(257, 5, widths, 31 + len(widths))
        pts, coors = case[0], case[1]
        vox, p2v, order, offsets, counts = R.voxel_map(coors)
        multi = [m for m in np.argsort(-counts) if 3 <= counts[m] <= 20][:4]
        lists = [order[offsets[m]:offsets[m] + counts[m]] for m in multi]
        pts[lists[0][1], 3] = np.nan           # a feature of a middle point: the point never wins the max
        pts[lists[1][-1], 0] = np.inf          # a coordinate: the mean, and with it every point of the voxel
        pts[lists[2][0], 4] = -np.inf
        pts[lists[3], 3] = np.nan              # every point of the voxel
        want = R.dvfe(*case)
        got, _ = run(dev, case, *GRID)
        assert np.isneginf(want["out"][multi[3]]).all() and np.isneginf(want["out"][multi[1]]).all()
        assert np.isfinite(want["out"][multi[0]]).all()
        assert np.array_equal(got.astype(np.float64), want["out"], equal_nan=True)


def test_nothing_to_encode(dev):
    """every point out of range (M = 0), and no points at all"""
    case = integer_case(257, 5, (5, 5), 41)
    gone = (case[0], np.full_like(case[1], -1), *case[2:])
    out, vm = run(dev, gone, *GRID)
    assert vm.M == 0 and out.shape == (0, 5)
    full, vms = run(dev, gone, *GRID, static_rows=64)
    assert full.shape == (64, 5) and (full == 0).all() and int(vms.num_dev.item()) == 0
    none = (case[0][:0], case[1][:0], *case[2:])
    out, vm = run(dev, none, *GRID)
    assert vm.M == 0 and out.shape == (0, 5)


# ------------------------------------------------------------------------------------------------------ the modules of the five configs
CONFIGS = [("srfdet_voxel_kitti_L", "kitti_sweep", 1000), ("srfdet_voxel_kitti_LC", "kitti_sweep", 1000),
           ("srfdet_dvoxel_waymo_L", "waymo_sweep", 5000), ("srfdet_dvoxel_waymo_LC", "waymo_sweep", 5000),
           ("srfdet_dvoxel_nusc_L", "nuscenes_sweep", 2000)]


def build_encoder(name, dev):
    torch.manual_seed(0)
    model = workloads.build(name, 16).eval()
    g = torch.Generator().manual_seed(1)
    for m in model.pts_voxel_encoder.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            with torch.no_grad():
                m.weight.copy_(1 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    model.pts_voxel_encoder.to(dev)
    return model


@pytest.mark.parametrize("name,sweep,seed", CONFIGS)
def test_module_level_on_every_dynamic_config(dev, monkeypatch, name, sweep, seed):
    model = build_encoder(name, dev)
    enc = model.pts_voxel_encoder
    assert isinstance(enc, DynamicVFECustom)
    pts = torch.from_numpy(getattr(S, sweep)(seed, 6000)).to(dev)
    calls = []
    real = ops.dvfe
    monkeypatch.setattr(ops, "dvfe", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        p, coors = model.voxelize([pts])
        monkeypatch.delenv("SRF_DVFE", raising=False)
        assert enc.hip_route(p)
        new, vc = enc(p, coors)
        assert len(calls) == 1
        monkeypatch.setenv("SRF_DVFE", "0")
        assert not enc.hip_route(p)
        old, vc_old = enc(p, coors)
        assert len(calls) == 1                                   # the torch route does not come near the kernel
        monkeypatch.delenv("SRF_DVFE")
    assert torch.equal(vc, vc_old) and new.shape == old.shape and vc.shape[0] > 500
    pos_enc, layers = R.encoder_params(enc)
    case = (p.cpu().numpy(), coors.cpu().numpy(), [enc.vx, enc.vy, enc.vz], [enc.x_offset, enc.y_offset, enc.z_offset], enc._with_voxel_center,
            pos_enc, layers)
    want, T = reference(dev, case)
    assert np.array_equal(vc.cpu().numpy(), want["coors"])
    err = np.abs(new.double().cpu().numpy() - want["out"])
    err_old = np.abs(old.double().cpu().numpy() - want["out"])
    print(f"{name}: {p.shape[0]} points, {vc.shape[0]} voxels, T = {T:.3f} ulp; kernel route worst error / bound = "
          f"{np.max(err / want['bound']):.4f} (worst error {err.max():.3e}); torch route {np.max(err_old / want['bound']):.4f} "
          f"({err_old.max():.3e})")
    assert (err <= want["bound"]).all()

    # where the kernel must not be taken
    with torch.no_grad():
        enc.train()
        assert not enc.hip_route(p)
        enc.eval()
        assert enc.hip_route(p)
        with torch.autocast("cuda", dtype=torch.float16):
            assert not enc.hip_route(p)
        enc.return_point_feats = True
        assert not enc.hip_route(p)
        enc.return_point_feats = False
        assert not enc.hip_route(p.double()) and not enc.hip_route(p.cpu())
    with torch.enable_grad():
        q = p.clone().requires_grad_(True)
        assert not enc.hip_route(q)
        out, _ = enc(q, coors)
        assert out.requires_grad and len(calls) == 1


def test_static_voxel_map_through_the_module(dev, monkeypatch):
    """the fixed-shape voxel map of a captured frame (`static_rows` on the scatters, as `extract_bev_static` sets it): the live rows equal
    the eager ones, the padding rows are zeros with coordinates -1"""
    monkeypatch.delenv("SRF_DVFE", raising=False)
    model = build_encoder("srfdet_dvoxel_waymo_L", dev)
    enc = model.pts_voxel_encoder
    pts = torch.from_numpy(S.waymo_sweep(5000, 6000)).to(dev)
    with torch.no_grad():
        p, coors = model.voxelize([pts])
        eager, vc = enc(p, coors)
        M = vc.shape[0]
        static_coors = coors.clone()                              # the voxel map is cached on the coordinate tensor
        scatters = [enc.scatter, enc.vfe_scatter, enc.cluster_scatter]
        rows = M + (p.shape[0] - M) // 2                          # the map holds at most one voxel per point
        assert rows > M
        for sc in scatters:
            sc.static_rows = rows
        try:
            full, vcs = enc(p, static_coors)
        finally:
            for sc in scatters:
                sc.static_rows = None
    assert full.shape == (rows, eager.shape[1]) and int(enc.cluster_scatter.last_map_static.num_dev.item()) == M
    assert torch.equal(full[:M], eager) and torch.equal(vcs[:M], vc)
    assert (full[M:] == 0).all() and (vcs[M:] == -1).all()
