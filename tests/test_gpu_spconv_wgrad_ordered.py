"""srf_spconv_bwd_weight_ordered (csrc/spconv_bwd.hip): the sparse convolution's weight gradient with the partial sums of the row
ranges (BW_ROWS = 2048 output rows each) stored and added in ascending range order.

The order is pinned without a model of the MFMA's internal rounding: a single range must equal the atomic entry (one partial added to
zero is exact; `torch.equal` compares values, so the -0 the ordered entry may store where the atomic one leaves +0 counts as equal), and
several ranges must equal the numpy float32 sum, ascending, of the entry's own results on each range alone."""
import numpy as np
import pytest
import torch

from spconv_ref import dense_grads
from srfdet3d_amd import _lib, ops

pytestmark = pytest.mark.gpu
BW_ROWS = 2048
ROWS = [1, 2047, 2048, 2049, 4097]
CHANNELS = [(5, 16), (16, 16), (64, 128), (128, 128)]
_RULEBOOKS = {}


def rulebook(A, dev):
    """A distinct random sites of a small grid (two samples) and their 27-offset submanifold rulebook -> (idx numpy, shape, nbr)."""
    if A not in _RULEBOOKS:
        shape = [4, 20, 20] if A <= 2049 else [6, 24, 24]
        rng = np.random.default_rng(A)
        cells = np.sort(rng.choice(2 * int(np.prod(shape)), A, replace=False))
        idx = np.stack([cells // int(np.prod(shape)), (cells // (shape[1] * shape[2])) % shape[0], (cells // shape[2]) % shape[1],
                        cells % shape[2]], 1).astype(np.int32)
        t = torch.from_numpy(idx).to(dev)
        nbr, _ = ops.rulebook_subm(t, shape, [3, 3, 3], ops.coord_table_build(t, shape, 2))
        _RULEBOOKS[A] = (idx, shape, nbr)
    return _RULEBOOKS[A]


def pointwise(A, dev):
    """K = 1: every output row reads one input row (a permutation), a tenth of them none."""
    g = torch.Generator().manual_seed(A)
    nbr = torch.randperm(A, generator=g).int()
    none = torch.rand(A, generator=g) < 0.1
    none[0] = False                                                          # (A = 1 keeps its row)
    nbr[none] = -1
    return nbr.view(1, A).to(dev)


def _call(entry, f, g, nbr, rows=None, r0=0, ws_bytes=None):
    """The ordered or the atomic entry on output rows [r0, r0 + rows) of (g, nbr) -> (code, grad_W)."""
    L = _lib.lib()
    K, (A_in, Cin), Cout = nbr.shape[0], f.shape, g.shape[1]
    rows = g.shape[0] - r0 if rows is None else rows
    gw = torch.full((K, Cin, Cout), float("nan"), device=f.device)
    ld = nbr.stride(0) if nbr.shape[1] > 0 else 0
    p_nbr, p_g = nbr.data_ptr() + 4 * r0, g.data_ptr() + 4 * r0 * Cout
    if entry == "atomic":
        return L.srf_spconv_bwd_weight(f.data_ptr(), A_in, Cin, p_g, rows, Cout, p_nbr, ld, K, gw.data_ptr(), ops._stream()), gw
    need = L.srf_spconv_bwd_weight_ordered_workspace_bytes(rows, Cin, Cout, K)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=f.device)
    rc = L.srf_spconv_bwd_weight_ordered(f.data_ptr(), A_in, Cin, p_g, rows, Cout, p_nbr, ld, K, gw.data_ptr(), ws.data_ptr(),
                                         need if ws_bytes is None else ws_bytes, ops._stream())
    torch.cuda.synchronize()
    return rc, gw


def _data(A, cin, cout, dev, integer=False):
    g = torch.Generator().manual_seed(1000 * cin + cout + A)
    if integer:
        return torch.randint(-4, 5, (A, cin), generator=g).float().to(dev), torch.randint(-4, 5, (A, cout), generator=g).float().to(dev)
    return torch.randn(A, cin, generator=g).to(dev), torch.randn(A, cout, generator=g).to(dev)


def _float64(f, g, nbr):
    out = []
    for k in range(nbr.shape[0]):
        ok = nbr[k] >= 0
        x = f.double()[nbr[k].clamp(min=0).long()] * ok[:, None]
        out.append(x.t() @ g.double())
    return torch.stack(out)


@pytest.mark.parametrize("A", ROWS)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_ranges_are_added_in_ascending_order(dev, cin, cout, A):
    f, g = _data(A, cin, cout, dev)
    for nbr in (rulebook(A, dev)[2], pointwise(A, dev)):
        rc, got = _call("ordered", f, g, nbr)
        assert rc == 0 and torch.isfinite(got).all() and got.abs().sum() > 0
        if A <= BW_ROWS:
            rc, atomic = _call("atomic", f, g, nbr)
            assert rc == 0 and torch.equal(got, atomic)                      # values: -0 == +0
            continue
        want = None
        for r0 in range(0, A, BW_ROWS):
            rc, part = _call("ordered", f, g, nbr, rows=min(BW_ROWS, A - r0), r0=r0)
            assert rc == 0
            part = part.cpu().numpy()
            want = part if want is None else (want + part).astype(np.float32)   # starting from range 0's value, one rounding per range
        assert np.array_equal(got.cpu().numpy(), want), (nbr.shape[0], int((got.cpu().numpy() != want).sum()))
        rc, again = _call("ordered", f, g, nbr)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))   # two calls, the same bytes


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_integer_data_is_exact(dev, cin, cout):
    """Small integers: every product and sum is exact in float32 whatever the order -- ordered == atomic == float64."""
    A = 4097
    f, g = _data(A, cin, cout, dev, integer=True)
    for nbr in (rulebook(A, dev)[2], pointwise(A, dev)):
        (rc, got), (rc2, atomic) = _call("ordered", f, g, nbr), _call("atomic", f, g, nbr)
        assert rc == 0 and rc2 == 0
        ref = _float64(f, g, nbr)
        assert ref.abs().max() < 2 ** 24 and ref.abs().sum() > 0
        assert torch.equal(got.double(), ref) and torch.equal(atomic, got)


@pytest.mark.parametrize("cin,cout,A", [(5, 16, 4097), (64, 128, 2049)])
def test_random_data_against_float64_conv3d(dev, cin, cout, A):
    """The assertion tests/test_gpu_spconv_bwd.py::test_subm_conv_gradients applies to the atomic route: within 1e-4 of the largest
    element of the float64 conv3d autograd gradient on the densified grid."""
    idx, shape, nbr = rulebook(A, dev)
    rng = np.random.default_rng(cin * 131 + cout)
    feats = rng.standard_normal((A, cin)).astype(np.float32)
    W = (rng.standard_normal((27, cin, cout)) * 0.1).astype(np.float32)
    gout = rng.standard_normal((A, cout)).astype(np.float32)
    _, _, ref_gw = dense_grads(idx, shape, feats, W, gout, idx, shape, 1, 1, (3, 3, 3))
    rc, got = _call("ordered", torch.from_numpy(feats).to(dev), torch.from_numpy(gout).to(dev), nbr)
    rc2, atomic = _call("atomic", torch.from_numpy(feats).to(dev), torch.from_numpy(gout).to(dev), nbr)
    assert rc == 0 and rc2 == 0
    e_ord, e_at = (np.abs(x.cpu().numpy() - ref_gw).max() / np.abs(ref_gw).max() for x in (got, atomic))
    print(f"\nspconv wgrad ({cin}, {cout}) A {A}: max error over max |ref| ordered {e_ord:.2e}, atomic {e_at:.2e}")
    assert e_ord <= 1e-4


def test_empty_inputs_and_the_workspace(dev):
    f, g = _data(100, 16, dev=dev, cout=32)
    nbr = pointwise(100, dev)
    rc, got = _call("ordered", f, g, nbr[:, :0].contiguous(), rows=0)        # A_out == 0: zeros
    assert rc == 0 and (got == 0).all()
    f5, g5 = _data(5000, 16, 32, dev)
    nbr5 = pointwise(5000, dev)
    need = _lib.lib().srf_spconv_bwd_weight_ordered_workspace_bytes(5000, 16, 32, 1)
    assert need == 3 * 16 * 32 * 4
    for short in (need - 1, 0):
        rc, got = _call("ordered", f5, g5, nbr5, ws_bytes=short)
        assert rc == -2 and torch.isnan(got).all()                           # refused before any launch
    rc, got = _call("ordered", f5, g5, nbr5)
    assert rc == 0 and torch.isfinite(got).all()


def test_through_autograd_under_the_switch(dev, monkeypatch):
    A, cin, cout = 4097, 16, 32
    _, _, nbr = rulebook(A, dev)
    f, g = _data(A, cin, cout, dev)
    w = torch.randn(27, cin, cout, generator=torch.Generator().manual_seed(3)).to(dev)

    def wgrad():
        wl = w.clone().requires_grad_(True)
        ops.spconv_fwd(f, wl, nbr, subm=True).backward(g)
        return wl.grad

    monkeypatch.setenv("SRF_DETERMINISTIC", "1")
    a, b = wgrad(), wgrad()
    rc, direct = _call("ordered", f, g, nbr)
    assert rc == 0 and torch.equal(a.view(torch.int32), direct.view(torch.int32)) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    monkeypatch.delenv("SRF_DETERMINISTIC")
    rc, atomic = _call("atomic", f, g, nbr)
    c = wgrad()                                                              # unset: the atomic entry, to rounding the same gradient
    assert (c - a).abs().max() <= 1e-5 * a.abs().max() and (atomic - a).abs().max() <= 1e-5 * a.abs().max()


def test_a_residual_block_repeats_its_weight_gradients(dev, monkeypatch):
    """Two backward passes of one SparseBasicBlock in train mode (batch statistics, two 64-channel SubM convolutions over 4097 rows:
    three row ranges) under the switch give identical weight gradients."""
    from srfdet3d_amd.sparse import SparseBasicBlock, SparseConvTensor
    monkeypatch.setenv("SRF_DETERMINISTIC", "1")
    A, C = 4097, 64
    idx, shape, _ = rulebook(A, dev)
    torch.manual_seed(0)
    block = SparseBasicBlock(C, C, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01)).to(dev).train()
    feats, cot = _data(A, C, C, dev)

    def grads():
        block.zero_grad(set_to_none=True)
        x = SparseConvTensor(feats.clone().requires_grad_(True), torch.from_numpy(idx).to(dev), shape, 2)
        (block(x).features * cot).sum().backward()
        return [block.conv1.weight.grad.clone(), block.conv2.weight.grad.clone()]

    a, b = grads(), grads()
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and x.abs().sum() > 0
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
