"""tests/pillar_ref.py (the definition of `srf_pillar_vfe`) against the torch module, the reference's own fixture and its padded-slot rule;
`ops.pillar_vfe_ok` as a table.  No GPU."""
import copy
import os

import numpy as np
import pytest
import torch

import detgen
import pillar_ref as R
from srfdet3d_amd import ops
from srfdet3d_amd.plugin.pillar import PillarFeatureNetCustom

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "fusion_nusc.npz"))
VOXEL, RANGE = [0.2, 0.2, 8], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
U64 = 2.0 ** -53


def offsets(voxel=VOXEL, rng=RANGE):
    return [voxel[d] / 2 + rng[d] for d in range(3)]


def make_net(nf, cluster=True, centre=True, legacy=False, cout=64, prefix="pfn."):
    net = PillarFeatureNetCustom(in_channels=nf, feat_channels=[cout], with_distance=False, with_cluster_center=cluster,
                                 with_voxel_center=centre, voxel_size=VOXEL, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01),
                                 point_cloud_range=RANGE, legacy=legacy).eval()
    return detgen.load_det_params(net, prefix)


def fold64(net):
    """(W, scale, shift) of the net's one layer in float64."""
    pfn = net.pfn_layers[0]
    bn = pfn.norm
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return pfn.linear.weight.detach().double().numpy(), scale.numpy(), shift.numpy()


def pillars(rows, P, nf, seed):
    """Points inside their own cells of the 512 x 512 grid, n cycling through 1..P, zero-padded."""
    rng = np.random.default_rng(seed)
    coors = np.stack([np.zeros(rows), np.zeros(rows), rng.integers(0, 512, rows), rng.integers(0, 512, rows)], 1).astype(np.int32)
    num = (np.arange(rows) % P + 1).astype(np.int32)
    vox = rng.uniform(0, 1, (rows, P, nf))
    vox[:, :, 0] = RANGE[0] + (coors[:, 3:4] + rng.uniform(0.02, 0.98, (rows, P))) * VOXEL[0]
    vox[:, :, 1] = RANGE[1] + (coors[:, 2:3] + rng.uniform(0.02, 0.98, (rows, P))) * VOXEL[1]
    vox[:, :, 2] = rng.uniform(RANGE[2], RANGE[5], (rows, P))
    vox = (vox * (np.arange(P)[None, :, None] < num[:, None, None])).astype(np.float32)
    return vox, num, coors


@pytest.mark.parametrize("nf", [4, 5])
@pytest.mark.parametrize("cluster", [False, True])
@pytest.mark.parametrize("centre", [False, True])
@pytest.mark.parametrize("legacy", [False, True])
def test_definition_against_the_torch_module(nf, cluster, centre, legacy):
    """Decoration: bit for bit the float32 module's, except the cluster-mean terms (torch sums in another order).  Both means lie within
    gamma_P * sum|x| / n of the exact one and each difference x - mean adds one rounding, so those terms differ by at most
    2 gamma_P A + 2 u |x - mean|, A = sum_p |x_p| / n.
    Outputs against the module in float64: a decorated value of the definition differs from the float64 one by at most
      d_mean   = gamma_P A + u |x - mean|                                  (the float32 mean, the rounded difference)
      d_centre = gamma_4 (|idx| v + |off|) + u |x - c|                     (v and off rounded to float32, product, sum; the difference)
    and the raw features by nothing; through the layer that is |scale_c| sum_k |w_ck| d_k per point, and the max over the points moves
    by no more than the largest of them (ReLU and max are 1-Lipschitz).  Float64 roundoff of either side is counted at 2^13 u64."""
    rows, P = 24, 6
    net = make_net(nf, cluster, centre, legacy)
    vox, num, coors = pillars(rows, P, nf, 7 * nf + 2 * cluster + centre)
    seen = []
    hook = net.pfn_layers[0].register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().numpy().copy()))
    with torch.no_grad():
        net(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(coors))
    hook.remove()
    mine = R.decorate(vox, num, coors, VOXEL, offsets(), cluster, centre, legacy)
    assert mine.shape == seen[0].shape == (rows, P, nf + 3 * cluster + 3 * centre)
    cols = np.ones(mine.shape[2], bool)
    live = (np.arange(P)[None, :] < num[:, None])[:, :, None]
    A = np.abs(vox[:, :, :3].astype(np.float64)).sum(1, keepdims=True) / num[:, None, None]
    if cluster:
        cols[nf:nf + 3] = False
        d = np.abs(mine[:, :, nf:nf + 3].astype(np.float64))
        bound = (2 * R.gamma(P) * A + 2 * R.U32 * d) * live
        assert (np.abs(mine[:, :, nf:nf + 3].astype(np.float64) - seen[0][:, :, nf:nf + 3]) <= bound).all()
    assert np.array_equal(mine[:, :, cols], seen[0][:, :, cols])

    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        want = net64(torch.from_numpy(vox).double(), torch.from_numpy(num), torch.from_numpy(coors)).numpy()
    W, scale, shift = fold64(net)
    out, mag = R.pillar_vfe(vox, num, coors, VOXEL, offsets(), W, scale, shift, cluster, centre, legacy)
    delta = np.zeros(mine.shape, np.float64)
    if cluster:
        delta[:, :, nf:nf + 3] = R.gamma(P) * A + R.U32 * np.abs(mine[:, :, nf:nf + 3])
    if centre:
        reach = (np.abs(coors[:, [3, 2, 1]]) * np.asarray(VOXEL) + np.abs(offsets()))[:, None, :]
        fc = mine[:, :, -3:].astype(np.float64)
        d_c = R.gamma(4) * reach + R.U32 * np.abs(fc)
        delta[:, :, -3:] = d_c
        if legacy:
            delta[:, :, :3] = d_c
    per_point = np.einsum("rpk,ck->rpc", delta * live, np.abs(W)) * np.abs(scale)
    bn = net.pfn_layers[0].norm
    slack = 2.0 ** 13 * U64 * (mag + np.abs(bn.running_mean.numpy() * scale) + np.abs(bn.bias.detach().numpy()))
    bound = per_point.max(axis=1) + slack
    err = np.abs(out - want)
    print(f"nf {nf} cluster {cluster} centre {centre} legacy {legacy}: worst error / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()


def test_definition_against_the_reference_fixture():
    """`pfn.out` was made by the reference's own PillarFeatureNetCustom; the inputs are those of
    test_fusion_fixtures.py::test_pillar_feature_net_matches_reference, and so is the tolerance."""
    net = make_net(5, legacy=False)
    Np, Mp = 60, 20
    num = (np.arange(Np) % Mp + 1).astype(np.int32)
    vox = (detgen.det("pfn.voxels", (Np, Mp, 5)) * (np.arange(Mp)[None, :, None] < num[:, None, None])).astype(np.float32)
    pc = np.stack([np.zeros(Np), np.zeros(Np), np.arange(Np) % 512, (np.arange(Np) * 7) % 512], 1).astype(np.int32)
    W, scale, shift = fold64(net)
    out, _ = R.pillar_vfe(vox, num, pc, VOXEL, offsets(), W, scale, shift, True, True, False)
    np.testing.assert_allclose(out, GOLD["pfn.out"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("n,want", [(3, 0.5), (4, 0.0)])
def test_padded_slots_contribute_relu_of_the_shift(n, want):
    """All real activations negative, shift = +0.5 before the ReLU's clamp of the real points: a pillar with n < P returns the shift (its
    padded slots give relu(bn(0))), a full one returns 0.  The torch module, which is the reference's code, agrees."""
    P, nf, cout = 4, 4, 64
    net = make_net(nf, cluster=False, centre=False, cout=cout)
    bn = net.pfn_layers[0].norm
    with torch.no_grad():
        net.pfn_layers[0].linear.weight.zero_()
        net.pfn_layers[0].linear.weight[:, 3] = -1.0          # activation = -feature 3
        bn.weight.fill_(1.0), bn.bias.fill_(0.5), bn.running_mean.zero_(), bn.running_var.fill_(1.0 - bn.eps)
    vox = np.zeros((1, P, nf), np.float32)
    vox[0, :n, 3] = [1.0, 2.0, 3.0, 4.0][:n]                  # v = -f + 0.5 < 0 for every real point
    vox[0, :n, :3] = 0.25
    num, coors = np.array([n], np.int32), np.zeros((1, 4), np.int32)
    W, scale, shift = fold64(net)
    out, mag = R.pillar_vfe(vox, num, coors, VOXEL, offsets(), W, scale, shift, False, False, False)
    assert (out == want).all()
    # the shift slot, or the first of the (clamped, equal) real points: f = 1 (scale is 1 up to the float32 rounding of 1 - eps)
    np.testing.assert_allclose(mag, 0.5 if n < P else 1.0 + 0.5, rtol=1e-6, atol=0)
    with torch.no_grad():
        ref = net(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(coors)).numpy()
    np.testing.assert_allclose(ref, np.full((1, cout), want, np.float32), rtol=0, atol=1e-6)


VFE_OK = [  # rows, P, nf, Cout, taken
    (40000, 20, 5, 64, True), (40000, 20, 4, 64, True), (0, 20, 5, 64, True), (1, 1, 3, 64, True), (1, 64, 8, 256, True),
    (100, 20, 5, 128, True), (100, 20, 5, 192, True),
    (100, 20, 5, 32, False), (100, 20, 5, 96, False), (100, 20, 5, 320, False), (100, 20, 5, 0, False),     # Cout % 64, <= 256
    (100, 20, 2, 64, False), (100, 20, 9, 64, False),                                                      # 3 <= nf <= 8
    (100, 0, 5, 64, False), (100, 65, 5, 64, False),                                                       # 1 <= P <= 64
    ((1 << 29) // (20 * 5) + 1, 20, 5, 64, False), ((1 << 29) // 512 - 1, 64, 8, 64, True), ((1 << 29) // 512, 64, 8, 64, False),  # voxels < 2^31 B
    ((1 << 29) // 256, 1, 3, 256, False), ((1 << 29) // 256 - 1, 1, 3, 256, True),                         # out < 2^31 bytes
]


@pytest.mark.parametrize("rows,P,nf,cout,taken", VFE_OK)
def test_pillar_vfe_ok_table(rows, P, nf, cout, taken):
    assert ops.pillar_vfe_ok(rows, P, nf, cout) is taken


def test_scatter_ok_table():
    assert ops.pillar_scatter_ok(40000, 64, 1, 512, 512) and ops.pillar_scatter_ok(0, 4, 1, 1, 1)
    assert not ops.pillar_scatter_ok(10, 6, 1, 8, 8)                      # whole float4s
    assert not ops.pillar_scatter_ok(10, 64, 8, 1024, 1024)               # the canvas: 2^31 bytes
    assert not ops.pillar_scatter_ok((1 << 29) // 64, 64, 1, 8, 8)        # feats: 2^31 bytes
