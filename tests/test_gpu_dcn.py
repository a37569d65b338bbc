"""srf_dcnv2_nhwc (csrc/dcn.hip) and its route through ops / compat.dcn / dense.conv_bn_act / the Waymo LC backbone.

Oracle: the repository's own definition, compat.dcn.modulated_deform_conv2d, evaluated in float64 on the CPU on the same f32
inputs cast up (itself held to hand-computable cases by tests/test_configs.py::test_dcnv2_definition).

Error metric: e(y) = max|y - y64| / max(D), D = the same operator applied to |x|, |w| and the same offsets and mask in float64
(sum |w| m bilinear(|x|): the scale of the f32 chain's rounding error).

Tolerance rule (nothing fixed in advance): in the same test
  e_torch = the SRF_DCN=0 route (torch, f32, on the GPU): what the module computed before the kernel existed,
  e_chain = ops.conv_gemm_nhwc (the f32-MFMA chain the kernel shares) on the same x and w as a plain 3x3 convolution against its
            own float64 result, same normalisation,
and e_hip <= 2 * max(e_torch, e_chain): the factor covers what the blend adds per term on top of the chain (three roundings for the
bilinear sample, one for the mask) and a different summation order; a wrong corner, tap order or a missing mask shows at 1e-2.
Every figure is printed before it is asserted (pytest -s shows them; DESIGN.md section 7 quotes them).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from srfdet3d_amd import ops, synthetic as S, workloads
from srfdet3d_amd.compat import dcn as D
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes

pytestmark = pytest.mark.gpu


def _out_size(H, W, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def _inputs(seed, N, C, H, W, Cout, k=3, s=1, p=1, d=1, G=1, sigma=3.0, logits=True, planted=True):
    """x, offset (N, 2KG, Ho, Wo), mask (N, KG, Ho, Wo) -- logits or values in [0, 1] -- and weight, all f32 on the CPU; with the
    planted pixels of the issue in image 0 (needs Ho >= 4, Wo >= 6)."""
    g = torch.Generator().manual_seed(seed)
    K = k * k
    Ho, Wo = _out_size(H, W, k, s, p, d)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Cout, C, k, k, generator=g) / (k * C ** 0.5)
    off = torch.randn(N, 2 * K * G, Ho, Wo, generator=g) * sigma
    m = torch.randn(N, K * G, Ho, Wo, generator=g) * 1.5 if logits else torch.rand(N, K * G, Ho, Wo, generator=g)
    if planted:
        assert Ho >= 4 and Wo >= 6
        # base position of tap t at output pixel (oy, ox): oy s - p + (t // k) d, ox s - p + (t % k) d
        ty = torch.arange(K).div(k, rounding_mode="floor").float() * d
        tx = (torch.arange(K) % k).float() * d

        def put(oy, ox, py=None, px=None, dy=None, dx=None):
            for gi in range(G):
                ys = off[0, gi * 2 * K:(gi + 1) * 2 * K:2, oy, ox]
                xs = off[0, gi * 2 * K + 1:(gi + 1) * 2 * K:2, oy, ox]
                if dy is not None:
                    ys.copy_(torch.as_tensor(dy, dtype=torch.float32).expand(K))
                if dx is not None:
                    xs.copy_(torch.as_tensor(dx, dtype=torch.float32).expand(K))
                if py is not None:
                    ys.copy_(py - (oy * s - p + ty))
                if px is not None:
                    xs.copy_(px - (ox * s - p + tx))

        put(0, 0, dy=0.0, dx=0.0)                                                     # all-zero offsets
        put(0, 1, dy=torch.randint(-3, 4, (K,), generator=g).float(), dx=torch.randint(-3, 4, (K,), generator=g).float())  # integers
        put(1, 0, dy=-40.0, dx=-40.0)                                                 # fully outside
        put(1, 1, dy=1e4, dx=1e4)
        put(1, 2, dy=-40.0)                                                           # outside along one axis only
        put(1, 3, dx=1e4)
        put(2, 0, py=-0.37, px=2.3)                                                   # the border bands, every side
        put(2, 1, py=H - 1 + 0.6, px=1.75)
        put(2, 2, py=1.2, px=-0.25)
        put(2, 3, py=2.5, px=W - 1 + 0.8)
        put(2, 4, py=-0.5, px=-0.5)                                                   # and the corners
        put(2, 5, py=H - 0.5, px=W - 0.5)
        m[0, :, 3, 0] = float("-inf") if logits else 0.0                              # mask exactly 0 and exactly 1
        m[0, :, 3, 1] = float("inf") if logits else 1.0
    return x, off, m, w


def _ref64(x, off, m, w, bias, s, p, d, G, logits):
    """(y64, D) of the definition in float64 on the CPU; D = the operator on |x|, |w|, the same offsets and |mask| (no bias)."""
    x, off, m, w = x.double(), off.double(), m.double(), w.double()
    if logits:
        m = torch.sigmoid(m)
    y = D.modulated_deform_conv2d(x, off, m, w, None if bias is None else bias.double(), s, p, d, 1, G)
    scale = D.modulated_deform_conv2d(x.abs(), off, m.abs(), w.abs(), None, s, p, d, 1, G)
    return y, scale


def _torch_route(x, off, m, w, bias, s, p, d, G, logits, dev):
    """The SRF_DCN=0 arithmetic: compat.dcn.modulated_deform_conv2d in f32 on the GPU."""
    xg, og, mg, wg = x.to(dev), off.to(dev), m.to(dev), w.to(dev)
    with torch.no_grad():
        return D.modulated_deform_conv2d(xg, og, torch.sigmoid(mg) if logits else mg, wg, None if bias is None else bias.to(dev), s, p, d, 1, G)


def _hip(x, off, m, w, bias, s, p, d, G, logits, dev, scale=None, relu=False):
    """ops.dcnv2_nhwc on channels-last copies; offsets and mask as two views of ONE (N, Ho, Wo, 3KG) buffer in mmcv's order."""
    KG2 = off.shape[1]
    xh = x.to(dev).permute(0, 2, 3, 1).contiguous()
    om = torch.cat((off, m), 1).to(dev).permute(0, 2, 3, 1).contiguous()
    k = w.shape[-1]
    y = ops.dcnv2_nhwc(xh, om[..., :KG2], om[..., KG2:], ops.pack_conv_gemm_weights(w.to(dev)), w.shape[0], (k, k), s, p, d, G, logits,
                       scale, None if bias is None else bias.to(dev), relu)
    return y.permute(0, 3, 1, 2)


def _e_chain(x, w, dev, scale=None, shift=None, relu=False):
    """ops.conv_gemm_nhwc (f32 MFMA) on x, w as a plain 3x3 / stride 1 / padding 1 convolution against float64, normalised by
    conv(|x|, |w|) (times |scale|, plus |shift|, when the epilogue is tested); also returns the GPU result."""
    Cout = w.shape[0]
    xh = x.to(dev).permute(0, 2, 3, 1).contiguous()
    y = ops.conv_gemm_nhwc(xh, ops.pack_conv_gemm_weights(w.to(dev)), Cout, (3, 3), 1, 1, None if scale is None else scale.to(dev),
                           None if shift is None else shift.to(dev), relu).permute(0, 3, 1, 2).cpu().double()
    y64 = F.conv2d(x.double(), w.double(), None, 1, 1)
    n64 = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)
    if scale is not None:
        y64, n64 = y64 * scale.double().view(1, -1, 1, 1), n64 * scale.double().abs().view(1, -1, 1, 1)
    if shift is not None:
        y64, n64 = y64 + shift.double().view(1, -1, 1, 1), n64 + shift.double().abs().view(1, -1, 1, 1)
    if relu:
        y64 = y64.clamp_min(0)
    return ((y - y64).abs().max() / n64.max()).item()


CASES = {
    # name: (N, C, H, W, Cout, stride, pad, dilation, G, bias)
    "waymo_s16_256": (5, 256, 40, 60, 256, 1, 1, 1, 1, False),
    "waymo_s32_512": (5, 512, 20, 30, 512, 1, 1, 1, 1, False),
    "ragged_32_48": (1, 32, 9, 7, 48, 1, 1, 1, 1, False),
    "ragged_64_64": (2, 64, 20, 30, 64, 1, 1, 1, 1, False),
    "ragged_96_160": (3, 96, 17, 33, 160, 1, 1, 1, 1, False),
    "s2_d2_g2_bias": (2, 64, 20, 30, 64, 2, 2, 2, 2, True),
}


@pytest.mark.parametrize("logits", [True, False], ids=["logits", "values"])
@pytest.mark.parametrize("case", list(CASES))
def test_operator_against_float64(case, logits, dev):
    N, C, H, W, Cout, s, p, d, G, with_bias = CASES[case]
    x, off, m, w = _inputs(11 + len(case), N, C, H, W, Cout, 3, s, p, d, G, 3.0, logits)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(5)) if with_bias else None
    y64, scale = _ref64(x, off, m, w, bias, s, p, d, G, logits)
    norm = scale.max()
    e_torch = ((_torch_route(x, off, m, w, bias, s, p, d, G, logits, dev).cpu().double() - y64).abs().max() / norm).item()
    e_chain = _e_chain(x, w, dev)
    y = _hip(x, off, m, w, bias, s, p, d, G, logits, dev)
    assert tuple(y.shape) == tuple(y64.shape)
    err = (y.cpu().double() - y64).abs()
    e_hip = (err.max() / norm).item()
    # the planted pixels (image 0, rows 0-3) on their own, so that a fault there is named
    e_planted = (err[0, :, :4, :6].max() / norm).item()
    print(f"\nDCN {case} {'logits' if logits else 'values'}: e_hip {e_hip:.3e} (planted pixels {e_planted:.3e})  e_torch {e_torch:.3e}  "
          f"e_chain {e_chain:.3e}  bound {2 * max(e_torch, e_chain):.3e}")
    assert torch.isfinite(y).all()
    assert e_hip <= 2 * max(e_torch, e_chain), (e_hip, e_torch, e_chain)


def test_zero_and_integer_offsets_are_plain_convolutions(dev):
    """Zero offsets with a unit mask are the plain convolution; a constant integer offset is the convolution of the shifted map:
    both equal ops.conv_gemm_nhwc on the same packed weight to within e_chain (the gathered operand is then exact)."""
    N, C, H, W, Cout = 2, 64, 20, 30, 64
    x, off, m, w = _inputs(3, N, C, H, W, Cout, logits=False, planted=False)
    e_chain = _e_chain(x, w, dev)
    norm = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1).max()
    pw = ops.pack_conv_gemm_weights(w.to(dev))
    xh = x.to(dev).permute(0, 2, 3, 1).contiguous()
    plain = ops.conv_gemm_nhwc(xh, pw, Cout, (3, 3), 1, 1).permute(0, 3, 1, 2)
    y0 = _hip(x, torch.zeros_like(off), torch.ones_like(m), w, None, 1, 1, 1, 1, False, dev)
    e0 = ((y0 - plain).abs().max().double().cpu() / norm).item()
    # offset (dy, dx) = (1, -2) everywhere: tap (ky, kx) of output (oy, ox) reads x[oy + ky, ox + kx - 3], zero outside the map
    dy, dx = 1, -2
    offi = torch.zeros_like(off)
    offi[:, 0::2], offi[:, 1::2] = dy, dx
    xp = torch.zeros(N, C, H + 2, W + 2)                    # xp[a, b] = x[a - 1 + dy, b - 1 + dx]: the padded, shifted map
    ys, xs = torch.arange(H + 2) - 1 + dy, torch.arange(W + 2) - 1 + dx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    xp[:, :, oky.nonzero()[:, None, 0], okx.nonzero()[None, :, 0]] = x[:, :, ys[oky]][:, :, :, xs[okx]]
    shifted = ops.conv_gemm_nhwc(xp.to(dev).permute(0, 2, 3, 1).contiguous(), pw, Cout, (3, 3), 1, 0).permute(0, 3, 1, 2)
    y1 = _hip(x, offi, torch.ones_like(m), w, None, 1, 1, 1, 1, False, dev)
    e1 = ((y1 - shifted).abs().max().double().cpu() / norm).item()
    print(f"\nDCN special cases: zero offsets vs conv_gemm {e0:.3e}, integer offsets vs shifted conv_gemm {e1:.3e}, e_chain {e_chain:.3e}")
    assert e0 <= e_chain and e1 <= e_chain, (e0, e1, e_chain)


def test_epilogue_and_pixel_pitch(dev):
    """scale / shift / relu against float64 under the same rule; x read from, and y written into, a channel slice of a wider
    buffer (pixel pitch > channels): the neighbouring channels of y stay untouched."""
    N, C, H, W, Cout = 2, 64, 20, 30, 80
    x, off, m, w = _inputs(21, N, C, H, W, Cout, logits=True)
    g = torch.Generator().manual_seed(8)
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    y64, nrm = _ref64(x, off, m, w, None, 1, 1, 1, 1, True)
    y64 = (y64 * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0)
    norm = (nrm * scale.double().abs().view(1, -1, 1, 1) + shift.double().abs().view(1, -1, 1, 1)).max()
    yt = torch.relu(_torch_route(x, off, m, w, None, 1, 1, 1, 1, True, dev) * scale.to(dev).view(1, -1, 1, 1) + shift.to(dev).view(1, -1, 1, 1))
    e_torch = ((yt.cpu().double() - y64).abs().max() / norm).item()
    e_chain = _e_chain(x, w, dev, scale, shift, True)
    xbuf = torch.full((N, H, W, C + 24), 7.0, device=dev)
    xbuf[..., 8:8 + C] = x.to(dev).permute(0, 2, 3, 1)
    ybuf = torch.full((N, H, W, Cout + 16), -3.0, device=dev)
    om = torch.cat((off, m), 1).to(dev).permute(0, 2, 3, 1).contiguous()
    out = ops.dcnv2_nhwc(xbuf[..., 8:8 + C], om[..., :18], om[..., 18:], ops.pack_conv_gemm_weights(w.to(dev)), Cout, (3, 3), 1, 1, 1, 1, True,
                         scale.to(dev), shift.to(dev), True, out=ybuf[..., 4:4 + Cout])
    assert out.data_ptr() == ybuf[..., 4:4 + Cout].data_ptr()
    assert (ybuf[..., :4] == -3.0).all() and (ybuf[..., 4 + Cout:] == -3.0).all() and (xbuf[..., :8] == 7.0).all()
    e_hip = ((ybuf[..., 4:4 + Cout].permute(0, 3, 1, 2).cpu().double() - y64).abs().max() / norm).item()
    print(f"\nDCN epilogue + pitch: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  e_chain {e_chain:.3e}")
    assert (ybuf[..., 4:4 + Cout] >= 0).all()
    assert e_hip <= 2 * max(e_torch, e_chain), (e_hip, e_torch, e_chain)


def test_determinism(dev):
    x, off, m, w = _inputs(31, 3, 96, 17, 33, 160, logits=True)
    a = _hip(x, off, m, w, None, 1, 1, 1, 1, True, dev)
    b = _hip(x, off, m, w, None, 1, 1, 1, 1, True, dev)
    assert torch.equal(a, b)
    nchw = ops.modulated_deform_conv2d(x.to(dev), off.to(dev), torch.sigmoid(m).to(dev), w.to(dev), None, 1, 1, 1, 1, 1)
    assert nchw.is_contiguous() and torch.equal(nchw, ops.modulated_deform_conv2d(x.to(dev), off.to(dev), torch.sigmoid(m).to(dev), w.to(dev),
                                                                                 None, 1, 1, 1, 1, 1))


def _random_pack(seed, cin, cout, **kw):
    torch.manual_seed(seed)
    pack = D.ModulatedDeformConv2dPack(cin, cout, 3, 1, 1, **kw)
    with torch.no_grad():
        pack.conv_offset.weight.normal_(0, 1.0 / (3 * cin ** 0.5))     # its init zeros it: offsets ~ N(0, 1) pixels on N(0, 1) inputs
        pack.conv_offset.bias.normal_(0, 0.5)
        if pack.bias is not None:
            pack.bias.normal_(0, 0.5)
    return pack.eval()


def _no_grid_sample(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("F.grid_sample called: the torch route of compat.dcn ran")
    monkeypatch.setattr(F, "grid_sample", boom)


def _module_errors(pack, x, dev, monkeypatch):
    """(e_hip, e_torch, e_chain) of one module forward; the float64 module on the CPU is the reference."""
    with torch.no_grad():
        p64 = copy.deepcopy(pack).double()
        y64 = p64(x.double())
        o1, o2, mm = torch.chunk(p64.conv_offset(x.double()), 3, dim=1)
        norm = D.modulated_deform_conv2d(x.double().abs(), torch.cat((o1, o2), 1), torch.sigmoid(mm), p64.weight.abs(), None, pack.stride,
                                         pack.padding, pack.dilation, 1, pack.deform_groups).max()
        if pack.bias is not None:
            norm = norm + pack.bias.double().abs().max()
        gp = copy.deepcopy(pack).to(dev)
        monkeypatch.setenv("SRF_DCN", "0")
        yt = gp(x.to(dev))
        monkeypatch.delenv("SRF_DCN")
        with monkeypatch.context() as mp:
            _no_grid_sample(mp)
            yh = gp(x.to(dev))
    e_chain = _e_chain(x, pack.weight.detach(), dev)
    return gp, yh, ((yh.cpu().double() - y64).abs().max() / norm).item(), ((yt.cpu().double() - y64).abs().max() / norm).item(), e_chain


def test_module_hip_route_and_weight_cache(dev, monkeypatch):
    pack = _random_pack(2, 64, 96, bias=True)
    x = torch.randn(2, 64, 20, 30, generator=torch.Generator().manual_seed(1))
    gp, yh, e_hip, e_torch, e_chain = _module_errors(pack, x, dev, monkeypatch)
    print(f"\nDCN module 64->96: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  e_chain {e_chain:.3e}")
    assert yh.is_contiguous() and tuple(yh.shape) == (2, 96, 20, 30)
    assert e_hip <= 2 * max(e_torch, e_chain), (e_hip, e_torch, e_chain)
    # in-place updates of both weights: the packed copies follow
    with torch.no_grad():
        gp.weight.mul_(-1.5)
        gp.conv_offset.weight.mul_(0.5)
        pack.weight.mul_(-1.5)
        pack.conv_offset.weight.mul_(0.5)
    _, yh2, e_hip2, e_torch2, e_chain2 = _module_errors(pack, x, dev, monkeypatch)
    with torch.no_grad():
        with monkeypatch.context() as mp:
            _no_grid_sample(mp)
            yh3 = gp(x.to(dev))
    print(f"DCN module after the in-place update: e_hip {e_hip2:.3e}  e_torch {e_torch2:.3e}  e_chain {e_chain2:.3e}")
    assert e_hip2 <= 2 * max(e_torch2, e_chain2)
    assert torch.equal(yh3, yh2) and not torch.allclose(yh3, yh)      # the cached module == a fresh copy of the updated one


def test_conv_bn_act_runs_batchnorm_and_relu_in_the_epilogue(dev, monkeypatch):
    """dense.conv_bn_act on a DCN conv2 with a foldable eval BatchNorm (what _Bottleneck calls): BatchNorm, the module's bias and the
    ReLU in the kernel's epilogue, against float64 under the same rule; in training mode of the BatchNorm the torch modules run."""
    from srfdet3d_amd import dense
    pack = _random_pack(7, 64, 96, bias=True)
    bn = torch.nn.BatchNorm2d(96).eval()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(96, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(96, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(96, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(96, generator=g) * 0.1)
    x = torch.randn(2, 64, 20, 30, generator=g)
    with torch.no_grad():
        p64, b64 = copy.deepcopy(pack).double(), copy.deepcopy(bn).double()
        y64 = torch.relu(b64(p64(x.double())))
        sc = (b64.weight / torch.sqrt(b64.running_var + b64.eps)).abs().view(1, -1, 1, 1)
        o1, o2, mm = torch.chunk(p64.conv_offset(x.double()), 3, dim=1)
        norm = ((D.modulated_deform_conv2d(x.double().abs(), torch.cat((o1, o2), 1), torch.sigmoid(mm), p64.weight.abs(), p64.bias.abs(),
                                           1, 1, 1, 1, 1) + b64.running_mean.abs().view(1, -1, 1, 1)) * sc + b64.bias.abs().view(1, -1, 1, 1)).max()
        gp, gb, xg = copy.deepcopy(pack).to(dev), copy.deepcopy(bn).to(dev), x.to(dev)
        monkeypatch.setenv("SRF_DCN", "0")
        yt = dense.conv_bn_act(gp, gb, True, xg)
        monkeypatch.delenv("SRF_DCN")
        with monkeypatch.context() as mp:
            _no_grid_sample(mp)
            yh = dense.conv_bn_act(gp, gb, True, xg)
        scale, shift = dense._fold_bn2d(gb)
        e_chain = _e_chain(x, pack.weight.detach(), dev, scale.cpu(), (shift + gp.bias * scale).cpu(), True)
        e_hip, e_torch = ((yh.cpu().double() - y64).abs().max() / norm).item(), ((yt.cpu().double() - y64).abs().max() / norm).item()
        print(f"\nDCN conv_bn_act 64->96 + bias + BN + ReLU: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  e_chain {e_chain:.3e}")
        assert yh.is_contiguous() and (yh >= 0).all()
        assert e_hip <= 2 * max(e_torch, e_chain), (e_hip, e_torch, e_chain)
        gb.train()                     # not foldable: conv and BatchNorm as modules (the kernel still runs the convolution)
        want = torch.relu(copy.deepcopy(gb)(gp(xg)))
        assert torch.equal(dense.conv_bn_act(gp, gb, True, xg), want)


def _direct(pack, x):
    """The module's forward written out: compat.dcn.modulated_deform_conv2d called directly; -> output and all gradients."""
    ref = copy.deepcopy(pack)
    ref.zero_grad()
    x2 = x.detach().clone().requires_grad_(True)
    o1, o2, m = torch.chunk(ref.conv_offset(x2), 3, dim=1)
    y2 = D.modulated_deform_conv2d(x2, torch.cat((o1, o2), dim=1), torch.sigmoid(m), ref.weight, ref.bias, 1, 1, 1, 1, 1)
    y2.square().sum().backward()
    return [y2.detach(), x2.grad, ref.weight.grad, ref.bias.grad, ref.conv_offset.weight.grad, ref.conv_offset.bias.grad]


def test_module_under_autograd_is_the_torch_function(dev, monkeypatch):
    """With grad enabled the module is today's torch code: its output and all gradients (input, weight, bias, conv_offset.*) equal a
    direct call of compat.dcn.modulated_deform_conv2d.

    torch.equal is asked wherever torch's own kernels give the same bits twice.  They do not always: the backward of F.grid_sample
    adds into the input gradient with float atomics, MIOpen settles its algorithm on the first call of a shape, and its weight
    gradients differ from call to call now and then (measured between evaluations of the SAME code: d input by 2.4e-7 every time, d
    weight or d conv_offset.weight by ~2e-5 in some runs, everything else reproducible).  So after a warm-up the module runs three
    times and the direct call four times; a tensor on which the direct calls agree bit for bit must be torch.equal to a module
    run's; one on which they differ must have a module run within twice the largest difference between direct calls.  In every
    case the call itself is pinned: the module hands the unchanged function the input tensor, its own parameters and the chunks of
    its conv_offset output, once, and returns that call's result object -- the same autograd graph."""
    pack = _random_pack(3, 64, 64, bias=True).to(dev)
    x = torch.randn(2, 64, 12, 16, device=dev, requires_grad=True)
    pack(x).square().sum().backward()          # warm-up: MIOpen's forward / backward choices for these shapes
    pack.zero_grad()
    x.grad = None
    calls = []
    orig = D.modulated_deform_conv2d

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append((a, k, out))
        return out

    with monkeypatch.context() as mp:
        mp.setattr(D, "modulated_deform_conv2d", spy)
        y = pack(x)
    assert len(calls) == 1 and not calls[0][1] and calls[0][2] is y
    a = calls[0][0]
    assert a[0] is x and a[3] is pack.weight and a[4] is pack.bias and tuple(a[5:]) == (1, 1, 1, 1, 1)
    with torch.no_grad():
        o1, o2, m = torch.chunk(pack.conv_offset(x), 3, dim=1)
        assert torch.equal(a[1], torch.cat((o1, o2), dim=1)) and torch.equal(a[2], torch.sigmoid(m))
    y.square().sum().backward()

    def through_module(y=None):
        if y is None:
            pack.zero_grad()
            x.grad = None
            y = pack(x)
            y.square().sum().backward()
        return [t.detach().clone() for t in (y, x.grad, pack.weight.grad, pack.bias.grad, pack.conv_offset.weight.grad, pack.conv_offset.bias.grad)]

    got = [through_module(y), through_module(), through_module()]
    want = [_direct(pack, x) for _ in range(4)]
    names = ["output", "d input", "d weight", "d bias", "d conv_offset.weight", "d conv_offset.bias"]
    for i, name in enumerate(names):
        assert all(g[i].shape == want[0][i].shape for g in got)
        spread = max((a[i] - b[i]).abs().max().item() for a in want for b in want)
        cross = min((g[i] - w[i]).abs().max().item() for g in got for w in want)
        print(f"\nDCN autograd {name}: direct calls differ by up to {spread:.3e}, nearest module / direct pair by {cross:.3e}")
        if spread == 0:
            assert any(torch.equal(g[i], want[0][i]) for g in got), name
        else:
            assert cross <= 2 * spread, name


def test_module_unsupported_shapes_take_the_torch_route(dev, monkeypatch):
    cases = [(_random_pack(4, 64, 64, groups=2), torch.randn(1, 64, 10, 12)),            # convolution groups
             (_random_pack(5, 32, 32, deform_groups=2), torch.randn(1, 32, 10, 12)),     # Cin / G = 16
             (_random_pack(6, 64, 64).half(), torch.randn(1, 64, 10, 12).half())]        # f16
    for pack, x in cases:
        pack, x = pack.to(dev), x.to(dev)
        with torch.no_grad():
            assert not pack.hip_route(x)
            got = pack(x)
            monkeypatch.setenv("SRF_DCN", "0")
            want = pack(x)
            monkeypatch.delenv("SRF_DCN")
        assert torch.equal(got, want)


def _randomize_bn(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _randomize_conv_offset(backbone, img, seed=0):
    """Every `conv_offset` ~ N(0, s) with s chosen per layer from the layer's own input (one CPU forward; a pre-hook sets the layer's
    weight just before it runs) so that its offsets have a standard deviation of about one pixel."""
    g = torch.Generator().manual_seed(seed)
    layers = [m for m in backbone.modules() if isinstance(m, D.ModulatedDeformConv2dPack)]

    def hook(mod, args):
        cin = mod.in_channels
        rms = args[0].square().mean().sqrt().clamp_min(1e-6)
        mod.conv_offset.weight.copy_(torch.randn(mod.conv_offset.weight.shape, generator=g) / (3 * cin ** 0.5 * rms))
        mod.conv_offset.bias.copy_(torch.randn(mod.conv_offset.bias.shape, generator=g) * 0.1)

    hooks = [m.register_forward_pre_hook(hook) for m in layers]
    with torch.no_grad():
        backbone(img)
    for h in hooks:
        h.remove()
    return len(layers)


def test_waymo_lc_backbone(dev, monkeypatch):
    torch.manual_seed(6)
    bb = workloads.build("srfdet_dvoxel_waymo_LC", 32).eval().img_backbone
    _randomize_bn(bb, 6)
    img = torch.from_numpy(S.camera_images(3100, n_cam=5, h=160, w=256))[0]
    assert _randomize_conv_offset(bb, img) == 26
    with torch.no_grad():
        assert all(m.conv_offset.weight.abs().max() > 0 for m in bb.modules() if isinstance(m, D.ModulatedDeformConv2dPack))
        ref = copy.deepcopy(bb).double()(img.double())
        gb = copy.deepcopy(bb).to(dev)
        monkeypatch.setenv("SRF_DCN", "0")
        yt = gb(img.to(dev))
        monkeypatch.delenv("SRF_DCN")
        with monkeypatch.context() as mp:
            _no_grid_sample(mp)          # all 26 layers must take the kernel
            yh = gb(img.to(dev))
    assert len(yh) == len(ref)
    for lvl, (h, t, r) in enumerate(zip(yh, yt, ref)):
        top = r.abs().max()
        e_hip, e_torch = ((h.cpu().double() - r).abs().max() / top).item(), ((t.cpu().double() - r).abs().max() / top).item()
        print(f"\nWaymo LC img_backbone level {lvl} {tuple(h.shape)}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}")
    for lvl, (h, t, r) in enumerate(zip(yh, yt, ref)):
        top = r.abs().max()
        e_hip, e_torch = ((h.cpu().double() - r).abs().max() / top).item(), ((t.cpu().double() - r).abs().max() / top).item()
        assert e_hip <= 2 * e_torch, (lvl, e_hip, e_torch)


def test_waymo_lc_graph_replays_on_the_kernel(dev, monkeypatch):
    """srfdet_dvoxel_waymo_LC through enable_hip_graphs() with F.grid_sample patched to raise: capture + three replays; pre-NMS scores
    and boxes agree with the eager HIP route to the tolerances of
    test_gpu_integration.py::test_remaining_reference_configs_run_and_graphs_agree for this config."""
    torch.manual_seed(4)
    cpu = workloads.build("srfdet_dvoxel_waymo_LC", 32).eval()
    _randomize_bn(cpu, 4)
    imgs = S.camera_images(3000, n_cam=5, h=160, w=256)
    _randomize_conv_offset(cpu.img_backbone, torch.from_numpy(imgs)[0], 4)
    eager = copy.deepcopy(cpu).to(dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    rig = S.camera_rig(n_cam=5, f=1266.0 * 256 / 1600, cx=128.0, cy=80.0)
    metas[0]["lidar2img"] = [m for m in rig]
    img = torch.from_numpy(imgs).to(dev)
    pts = [torch.from_numpy(S.waymo_sweep(7000 + i, 40000)).to(dev) for i in range(2)]
    _no_grid_sample(monkeypatch)
    with torch.no_grad():
        want = []
        for p in pts:
            mt = copy.deepcopy(metas)
            f_img, f_pt = eager.extract_feat(img, [p], mt)
            s, b = eager.bbox_head.decode(*eager.bbox_head(f_img, f_pt, mt))
            assert torch.isfinite(s).all() and torch.isfinite(b).all()
            want.append((s, b))
    g = copy.deepcopy(cpu).to(dev).enable_hip_graphs()
    with torch.no_grad():
        g.simple_test(img, [pts[0]], copy.deepcopy(metas))                     # eager pass + capture
        for i in (1, 0, 1):
            g.simple_test(img, [pts[i]], copy.deepcopy(metas))
            e = g._graphed_frame.entry if g._graphed_frame is not None else list(g._graphed_tail.entries.values())[-1]
            torch.testing.assert_close(e["scores"], want[i][0], rtol=0, atol=2e-4)
            tight = torch.isclose(e["boxes"], want[i][1], rtol=1e-3, atol=2e-3)
            assert tight.float().mean().item() >= 0.99, f"{(~tight).sum().item()} of {tight.numel()} box entries differ"
            torch.testing.assert_close(e["boxes"], want[i][1], rtol=1e-2, atol=2e-3)
