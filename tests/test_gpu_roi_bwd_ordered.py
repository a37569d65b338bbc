"""srf_roi_extract_bwd_ordered (csrc/roi_bwd_ordered.hip) on the GPU: bit-equal to its numpy float32 definition
(tests/roi_bwd_ordered_ref.py) over channel counts, (pooled, sampling ratio), map and gradient layouts and the case table of
tests/test_roi_bwd_ordered_ref.py; the untouched elements keep a sentinel; the integer construction agrees exactly with the atomic route
and float64; the float64 bar of the atomic route; repeatability; the edges of the ABI; the route through autograd and the head.

The definition costs (contributing records) x C float32 operations in numpy, so the RoIs of a case are chosen under a budget: the edge
RoIs, the clamped, the invalid and the empty-level rows of the table always, the 64 duplicates and the random RoIs as far as it reaches
(all of them at C = 20; at (8, 4) with 516 channels the table's rows and a few random RoIs)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import roi_bwd_ordered_ref as OR
import roi_ref as RR
from srfdet3d_amd import _lib, ops
from srfdet3d_amd._lib import FeatMap
from test_gpu_train_grads import ROI_BWD_TOL, _edge_rois, _random_rois

pytestmark = pytest.mark.gpu
TABLE = OR.case_table()
SENTINEL = -7.5
assert ROI_BWD_TOL == OR.ROI_BWD_TOL


def call_ordered(grads, rois, pooled, sr, gout, strides3, C, strides=OR.STRIDES, finest=OR.FINEST, ws=None, ws_bytes=None):
    """srf_roi_extract_bwd_ordered itself -> return code.  grads: the maps to store into (their strides are the layout)."""
    L = _lib.lib()
    nl, R = len(grads), rois.shape[0]
    fm = (FeatMap * nl)(*[ops._featmap(g, 1.0 / s) for g, s in zip(grads, strides)])
    gp = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in grads])
    need = L.srf_roi_extract_bwd_ordered_workspace_bytes(R, pooled, sr)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=rois.device)
    return L.srf_roi_extract_bwd_ordered(fm, gp, nl, C, rois.data_ptr(), R, pooled, sr, float(finest), gout.data_ptr(), *strides3,
                                         ws.data_ptr(), need if ws_bytes is None else ws_bytes, ops._stream())


def run_ordered(shapes, C, rois, pooled, sr, g_bm, cl, bin_major, dev, fill=0.0):
    """-> per level (N, H, W, C) on the host.  g_bm (R, pooled^2, C) on the device."""
    grads = [torch.full((N, C, H, W), fill, device=dev) for N, H, W in shapes]
    if cl:
        grads = [g.contiguous(memory_format=torch.channels_last) for g in grads]
    bins = pooled * pooled
    gout = g_bm.contiguous() if bin_major else g_bm.permute(0, 2, 1).contiguous()
    s3 = (bins * C, 1, C) if bin_major else (C * bins, bins, 1)
    assert call_ordered(grads, rois.to(dev).contiguous(), pooled, sr, gout, s3, C) == 0
    torch.cuda.synchronize()
    return [g.permute(0, 2, 3, 1).contiguous().cpu() for g in grads]


def case_rois(C, pooled, sr, seed):
    """The RoIs of one (C, pooled, sr) point, see the module docstring -> (rois (n, 5) float32 tensor, names of the parts)."""
    g = torch.Generator().manual_seed(seed)
    per = pooled * pooled * sr * sr * 4 * C
    room = int(45e6 // per)
    level2 = torch.tensor([[2, 20.0, 10.0, 300.0, 260.0]])                  # sqrt(area) in [224, 448): the table's empty level
    parts = [("edge", torch.cat([_edge_rois(4, 256), level2])), ("clamp", torch.from_numpy(TABLE["clamp"])), ("invalid", torch.from_numpy(TABLE["invalid"])),
             ("empty_level", torch.from_numpy(TABLE["empty_level"]))]
    room -= sum(len(p) for _, p in parts)
    if room >= 64 + 8:
        parts.append(("dup64", torch.from_numpy(TABLE["dup64"])))
        room -= 64
    n = max(8, min(60, room))
    parts.append(("random", _random_rois(g, n, 4, 256, torch.arange(n) % 4)))
    return torch.cat([p for _, p in parts]).float(), [k for k, _ in parts]


@pytest.mark.parametrize("C", [20, 256, 516])
@pytest.mark.parametrize("pooled,sr", [(7, 2), (2, 3), (8, 4)])
def test_bit_equal_to_the_definition_and_the_sentinel_stays(dev, C, pooled, sr):
    rois, names = case_rois(C, pooled, sr, 100 * C + pooled)
    assert C != 20 or "dup64" in names
    lv = RR.levels(rois, 4, OR.FINEST)
    assert len(set(lv.tolist())) == 4
    g = torch.Generator().manual_seed(C + sr)
    gb = torch.randn(rois.shape[0], pooled * pooled, C, generator=g)
    want = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois.numpy(), gb.numpy(), pooled, sr, fill=SENTINEL)
    hit = OR.touched(OR.SHAPES, OR.STRIDES, rois.numpy(), pooled, sr)
    assert all(h.any() for h in hit) and not any(h.all() for h in hit[:3])   # (the 240 pixels of level 3 may all be hit)
    for cl in (True, False):
        for bin_major in (True, False):
            got = run_ordered(OR.SHAPES, C, rois, pooled, sr, gb.to(dev), cl, bin_major, dev, fill=SENTINEL)
            for l in range(4):
                w = torch.from_numpy(want[l])
                assert (got[l][~torch.from_numpy(hit[l])] == SENTINEL).all(), f"sentinel overwritten: nhwc {cl} bin-major {bin_major} level {l}"
                assert torch.equal(got[l], w), (f"nhwc {cl} bin-major {bin_major} level {l}: {(got[l] != w).sum().item()} elements differ, "
                                                f"max {(got[l] - w).abs().max().item():.3e}")


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_case_table_alone(dev, name):
    """Each row set of the table on its own (a level or three without any record, nothing but zero records, nothing but duplicates)."""
    rois = torch.from_numpy(TABLE[name])
    C, pooled, sr = 36, 7, 2
    gb = torch.randn(rois.shape[0], pooled * pooled, C, generator=torch.Generator().manual_seed(5))
    want = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois.numpy(), gb.numpy(), pooled, sr, fill=SENTINEL)
    for cl, bin_major in ((True, True), (False, False)):
        got = run_ordered(OR.SHAPES, C, rois, pooled, sr, gb.to(dev), cl, bin_major, dev, fill=SENTINEL)
        for l in range(4):
            assert torch.equal(got[l], torch.from_numpy(want[l])), (name, cl, l)


def _atomic(shapes, maps_like, rois, pooled, sr, gb, cl, bin_major, dev):
    from test_gpu_roi_domain import _bwd
    return [g.cpu() for g in _bwd(maps_like, rois, pooled, sr, gb, cl, bin_major, dev)]


def test_integer_form_agrees_with_the_atomic_route_and_float64(dev, monkeypatch):
    """The construction of test_gpu_roi_domain.py::test_backward_exact_at_256_channels_and_sr_3: weights that are multiples of 1/16 and
    output gradients 9 x small integers make every product and every add exact, in any order: ordered == atomic == float64."""
    monkeypatch.delenv("SRF_DETERMINISTIC", raising=False)
    g = torch.Generator().manual_seed(2)
    C, pooled, sr = 256, 7, 3
    shapes = [(12, 48 >> l, 80 >> l) for l in range(4)]
    fit = {0: [(3, 3), (3, 6), (6, 3), (6, 6)], 1: [(3, 6), (6, 3), (6, 6)], 2: [(3, 6), (6, 3), (6, 6)], 3: [(3, 6), (6, 3), (6, 6)]}
    rows, lvl = [], []
    for i in range(360):
        l = i % 4
        _, H, W = shapes[l]
        s = OR.STRIDES[l]
        bw2, bh2 = fit[l][int(torch.randint(0, len(fit[l]), (1,), generator=g))]     # bin sizes in half pixels
        kx = int(torch.randint(-3, max(W - 7 * bw2 // 2, 0) + 4, (1,), generator=g))
        ky = int(torch.randint(-3, max(H - 7 * bh2 // 2, 0) + 4, (1,), generator=g))
        rows.append([i % 12, kx * s, ky * s, kx * s + 7 * bw2 * s / 2, ky * s + 7 * bh2 * s / 2])
        lvl.append(l)
    rois = torch.tensor(rows, dtype=torch.float32)
    assert torch.equal(RR.levels(rois, 4, OR.FINEST), torch.tensor(lvl))
    for _, t, w in RR.taps(rois, shapes, OR.STRIDES, pooled, sr):
        assert torch.equal(w * 16, (w * 16).round()) and ((w > 0) & (w < 1)).any()
    maps = [torch.zeros(N, C, H, W) for N, H, W in shapes]
    gb = (9 * torch.randint(-3, 4, (rois.shape[0], pooled * pooled, C), generator=g)).float().to(dev)
    ref, _ = RR.grad64(shapes, OR.STRIDES, rois, gb, pooled, sr, OR.FINEST, dev=dev, chunk=32)
    for cl, bin_major in ((True, True), (False, False), (True, False)):
        got = run_ordered(shapes, C, rois, pooled, sr, gb, cl, bin_major, dev)
        atomic = _atomic(shapes, maps, rois, pooled, sr, gb, cl, bin_major, dev)
        for l in range(4):
            assert ref[l].abs().sum() > 0
            assert (got[l].double() - ref[l].cpu()).abs().max().item() == 0, (cl, bin_major, l)
            assert torch.equal(got[l], atomic[l]), (cl, bin_major, l)


@pytest.mark.parametrize("C", [128, 256, 516])
@pytest.mark.parametrize("pooled,sr", [(7, 2), (2, 3), (8, 4)])
def test_against_float64_under_the_bar_of_the_atomic_route(dev, C, pooled, sr, monkeypatch):
    """tests/test_gpu_roi_domain.py::test_backward_against_float64, its inputs, normalisation and constant (ROI_BWD_TOL,
    tests/test_gpu_train_grads.py:299), applied to the ordered route; both routes' worst errors side by side."""
    monkeypatch.delenv("SRF_DETERMINISTIC", raising=False)
    g = torch.Generator().manual_seed(100 * C + pooled)
    shapes = [(4, 48 >> l, 80 >> l) for l in range(4)]
    rois = torch.cat([_random_rois(g, 240, 4, 256, torch.arange(240) % 4), _edge_rois(4, 256)])
    maps = [torch.randn(N, C, H, W, generator=g) for N, H, W in shapes]
    gb = torch.randn(rois.shape[0], pooled * pooled, C, generator=g).to(dev)
    ref, mag = RR.grad64(shapes, OR.STRIDES, rois, gb, pooled, sr, OR.FINEST, dev=dev, chunk=16)
    worst = {"ordered": 0.0, "atomic": 0.0}
    for cl, bin_major in ((True, True), (False, False)):
        routes = {"ordered": run_ordered(shapes, C, rois, pooled, sr, gb, cl, bin_major, dev),
                  "atomic": _atomic(shapes, maps, rois, pooled, sr, gb, cl, bin_major, dev)}
        for l in range(4):
            assert ref[l].abs().sum() > 0
            for name, got in routes.items():
                err = ((got[l].to(dev).double() - ref[l]).abs() / mag[l].clamp_min(1e-300)).max().item()
                worst[name] = max(worst[name], err)
                if name == "ordered":
                    assert err <= ROI_BWD_TOL, f"channels_last {cl} level {l}: {err:.3e}"
    print(f"\nroi bwd C {C} pooled {pooled} sr {sr}: worst normalised error ordered {worst['ordered']:.2e}, atomic {worst['atomic']:.2e}")


def test_two_calls_give_the_same_bytes(dev):
    rois = torch.cat([torch.from_numpy(TABLE["dup64"]), torch.from_numpy(TABLE["clamp"])])
    C, pooled, sr = 256, 7, 2
    gb = torch.randn(rois.shape[0], pooled * pooled, C, generator=torch.Generator().manual_seed(9)).to(dev)
    for cl, bin_major in ((True, True), (False, False)):
        a = run_ordered(OR.SHAPES, C, rois, pooled, sr, gb, cl, bin_major, dev)
        b = run_ordered(OR.SHAPES, C, rois, pooled, sr, gb, cl, bin_major, dev)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert a[0].abs().sum() > 0


def test_edges_of_the_abi(dev):
    C, pooled, sr = 20, 7, 2
    rois = torch.from_numpy(TABLE["clamp"]).to(dev)
    grads = [torch.full((N, C, H, W), SENTINEL, device=dev) for N, H, W in OR.SHAPES]
    gout = torch.randn(len(rois), 49, C, device=dev)
    s3 = (49 * C, 1, C)
    need = _lib.lib().srf_roi_extract_bwd_ordered_workspace_bytes(len(rois), pooled, sr)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    # R == 0: SRF_OK, nothing launched, nothing written (a NULL workspace is fine)
    assert call_ordered(grads, rois[:0], pooled, sr, gout, s3, C, ws=torch.empty(0, dtype=torch.uint8, device=dev), ws_bytes=0) == 0
    assert call_ordered(grads, rois, pooled, sr, gout, s3, C, ws=ws, ws_bytes=need - 1) == -2       # one byte short
    assert call_ordered(grads, rois, pooled, sr, gout, s3, C, ws=ws[4:], ws_bytes=need) == -3      # not 16-byte aligned
    assert call_ordered(grads, rois, pooled, sr, gout, s3, C, ws=ws[1:], ws_bytes=need) == -3
    torch.cuda.synchronize()
    assert all((g == SENTINEL).all() for g in grads)                                                 # none of them reached a kernel
    assert call_ordered(grads, rois, pooled, sr, gout, s3, C, ws=ws[16:], ws_bytes=need) == 0      # 16-byte aligned is enough
    torch.cuda.synchronize()
    want = OR.grad_ordered(OR.SHAPES, OR.STRIDES, rois.cpu().numpy(), gout.cpu().numpy(), pooled, sr, fill=SENTINEL)
    for l in range(4):
        assert torch.equal(grads[l].permute(0, 2, 3, 1).cpu(), torch.from_numpy(want[l]))


class _Recorder:
    """Stands where `_lib.lib()` stands: forwards every entry point and notes its name."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("srf_"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def _autograd(rois, maps, pooled, sr, gb, bin_major, dev):
    fs = [m.to(dev).detach().requires_grad_(True) for m in maps]
    y = ops.roi_extract_autograd(fs, rois.to(dev), OR.STRIDES, pooled, sr, OR.FINEST, bin_major=bin_major)
    R, C = rois.shape[0], maps[0].shape[1]
    y.backward((gb if bin_major else gb.view(R, pooled, pooled, C).permute(0, 3, 1, 2)).contiguous())
    return [f.grad.permute(0, 2, 3, 1).contiguous().cpu() for f in fs]


def test_through_autograd_and_the_switch(dev, monkeypatch):
    g = torch.Generator().manual_seed(4)
    C, pooled, sr = 64, 7, 2
    rois = torch.cat([_random_rois(g, 40, 4, 256, torch.arange(40) % 4), torch.from_numpy(TABLE["clamp"])])
    maps = [torch.randn(N, C, H, W, generator=g) for N, H, W in OR.SHAPES]
    gb = torch.randn(rois.shape[0], pooled * pooled, C, generator=g).to(dev)
    real = _lib.lib()
    rec = _Recorder(real)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    # unset: the call sequence of before -- the gather, then the atomic entry and nothing else
    monkeypatch.delenv("SRF_DETERMINISTIC", raising=False)
    _autograd(rois, maps, pooled, sr, gb, True, dev)
    roi_calls = lambda: [c for c in rec.calls if "roi" in c]
    assert roi_calls() == ["srf_roi_extract", "srf_roi_extract_bwd"], rec.calls
    monkeypatch.setenv("SRF_DETERMINISTIC", "0")
    rec.calls.clear()
    _autograd(rois, maps, pooled, sr, gb, True, dev)
    assert roi_calls() == ["srf_roi_extract", "srf_roi_extract_bwd"], rec.calls
    # on: the ordered entry, equal to the direct call, for both layouts of the output gradient
    monkeypatch.setenv("SRF_DETERMINISTIC", "1")
    for bin_major in (True, False):
        rec.calls.clear()
        got = _autograd(rois, maps, pooled, sr, gb, bin_major, dev)
        assert roi_calls() == ["srf_roi_extract", "srf_roi_extract_bwd_ordered_workspace_bytes", "srf_roi_extract_bwd_ordered"], rec.calls
        direct = run_ordered(OR.SHAPES, C, rois, pooled, sr, gb, False, bin_major, dev)
        for l in range(4):
            assert torch.equal(got[l], direct[l]), (bin_major, l)
    # a shape the ordered entry refuses raises under the switch: no fall-back to the atomic entry
    monkeypatch.setattr(rec, "srf_roi_extract_bwd_ordered", lambda *a: -3, raising=False)
    rec.calls.clear()
    with pytest.raises(RuntimeError, match="roi_extract_bwd_ordered"):
        _autograd(rois, maps, pooled, sr, gb, True, dev)
    assert "srf_roi_extract_bwd" not in rec.calls


def test_head_level_gather_repeats_bit_for_bit(dev, monkeypatch):
    """`_StageBase._img_rois_feats` (gather over all cameras + camera sum) on bs = 2, 32 proposals, 6 cameras, C = 256, maps of
    16 x 28 ... 2 x 4: the gradients w.r.t. the maps under a fixed upstream weight, evaluated twice under the switch."""
    from srfdet3d_amd.plugin.heads import _StageBase
    from srfdet3d_amd.roi import SingleRoIExtractor
    monkeypatch.setenv("SRF_DETERMINISTIC", "1")
    bs, n_p, n_cam, C = 2, 32, 6, 256
    g = torch.Generator().manual_seed(11)
    sizes = [(16, 28), (8, 14), (4, 7), (2, 4)]
    feats = [torch.randn(bs, n_cam, C, h, w, generator=g).to(dev).requires_grad_(True) for h, w in sizes]
    n = n_cam * bs * n_p
    ctr = torch.rand(n, 2, generator=g) * torch.tensor([112.0, 64.0])
    wh = torch.exp(torch.rand(n, 2, generator=g) * np.log(40.0) + np.log(4.0))
    ids = (torch.arange(n) // n_p) % bs + (torch.arange(n) // (bs * n_p)) * bs                         # cam-major rows, id b + cam B
    rois = torch.cat([ids.float()[:, None], ctr - wh / 2, ctr + wh / 2], 1).to(dev)
    pooler = SingleRoIExtractor(dict(type="RoIAlign", output_size=7, sampling_ratio=2), C, [4, 8, 16, 32])
    stub = types.SimpleNamespace(corrected_cam_indexing=False)
    stub._gather = lambda f, r, p: _StageBase._gather(stub, f, r, p)
    upstream = torch.randn(bs * n_p, 49, C, generator=g).to(dev)

    def once():
        out = _StageBase._img_rois_feats(stub, feats, rois, pooler, bs, n_p, n_cam)
        assert tuple(out.shape) == (bs * n_p, 49, C)
        return [x.cpu() for x in torch.autograd.grad((out * upstream).sum(), feats)]

    a, b = once(), once()
    assert sum(x.abs().sum().item() for x in a) > 0
    for l, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), l
