"""Host side of the DCNv2 operator (no GPU): the C ABI's declaration, export and argument validation, the CPU behaviour of the
Python layers."""
import os
import re

import pytest
import torch

from srfdet3d_amd import _lib, ops
from srfdet3d_amd.compat import dcn as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "srfdet3d.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+srf_dcnv2_nhwc\s*\(", header)
    assert "srf_dcnv2_nhwc" in _lib.SIGNATURES
    L = _lib.lib()
    assert L.srf_dcnv2_nhwc is not None
    # one argument type per parameter of the declaration
    decl = re.search(r"\bint\s+srf_dcnv2_nhwc\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["srf_dcnv2_nhwc"][1])


def _call(L, N=1, H=20, W=30, Cin=64, x_ld=64, off_ld=18, mask_ld=9, Cout=64, kh=3, kw=3, stride=1, pad=1, dil=1, groups=1, G=1, y_ld=64,
          ptr=None):
    return L.srf_dcnv2_nhwc(ptr, N, H, W, Cin, x_ld, ptr, off_ld, ptr, mask_ld, 1, ptr, Cout, kh, kw, stride, pad, dil, groups, G, None, None, 0,
                            ptr, y_ld, None)


def test_argument_validation_before_any_hip_call():
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    assert _call(L) == EINVAL                           # null pointers
    assert _call(L, N=0) == 0                           # an empty batch is nothing to do
    assert _call(L, H=0) == EINVAL and _call(L, stride=0) == EINVAL and _call(L, dil=0) == EINVAL and _call(L, G=0) == EINVAL
    assert _call(L, x_ld=32) == EINVAL and _call(L, y_ld=32) == EINVAL             # pixel pitch below the channel count
    assert _call(L, off_ld=17) == EINVAL and _call(L, mask_ld=8) == EINVAL        # fewer than 2 K G / K G channels
    assert _call(L, G=2, off_ld=18, mask_ld=9) == EINVAL
    assert _call(L, groups=2) == EUNSUPPORTED                                      # convolution groups
    assert _call(L, Cin=48, x_ld=48) == EUNSUPPORTED                               # Cin / G % 32
    assert _call(L, G=2, off_ld=36, mask_ld=18) == EINVAL                          # Cin / G = 32: taken (then the null pointers)
    assert _call(L, Cin=32, x_ld=32, G=2, off_ld=36, mask_ld=18) == EUNSUPPORTED   # Cin / G = 16
    assert _call(L, Cin=96, x_ld=96, G=2, off_ld=36, mask_ld=18) == EUNSUPPORTED   # Cin / G = 48
    assert _call(L, H=1) == EUNSUPPORTED and _call(L, W=1) == EUNSUPPORTED
    assert _call(L, N=64, H=512, W=512, Cin=32, x_ld=32) == EUNSUPPORTED           # 2 GiB of input
    assert _call(L, kh=1, kw=1, pad=0, off_ld=2, mask_ld=1) == EINVAL              # 1x1: taken
    assert _call(L, H=2, W=2, pad=0) == EINVAL                                     # no output pixel


def test_dcnv2_supported_answers_as_documented():
    assert ops.dcnv2_supported(5, 256, 40, 60) and ops.dcnv2_supported(5, 512, 20, 30)
    assert ops.dcnv2_supported(2, 64, 20, 30, 1, 2) and ops.dcnv2_supported(1, 32, 9, 7)
    assert not ops.dcnv2_supported(2, 64, 20, 30, groups=2)
    assert not ops.dcnv2_supported(2, 32, 20, 30, deform_groups=2)       # Cin / G = 16
    assert not ops.dcnv2_supported(2, 48, 20, 30) and not ops.dcnv2_supported(2, 96, 20, 30, deform_groups=2)
    assert not ops.dcnv2_supported(2, 64, 20, 30, deform_groups=3)       # Cin % G
    assert not ops.dcnv2_supported(2, 64, 1, 30) and not ops.dcnv2_supported(2, 64, 20, 1)
    assert not ops.dcnv2_supported(64, 32, 512, 512)                     # 2 GiB
    assert ops.dcnv2_supported(2, 64, 20, 30, x_ld=88) and not ops.dcnv2_supported(2, 64, 20, 30, x_ld=66)
    assert ops.dcnv2_out_size(20, 30, 3, 2, 2, 2) == (10, 15) and ops.dcnv2_out_size(40, 60, (3, 3), 1, 1, 1) == (40, 60)


def test_ops_refuse_cpu_tensors():
    x, off, m, w = torch.randn(1, 32, 8, 8), torch.zeros(1, 18, 8, 8), torch.ones(1, 9, 8, 8), torch.randn(32, 32, 3, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.modulated_deform_conv2d(x, off, m, w, None, 1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError):
        ops.dcnv2_nhwc(x.permute(0, 2, 3, 1).contiguous(), off.permute(0, 2, 3, 1).contiguous(), m.permute(0, 2, 3, 1).contiguous(), w, 32,
                       (3, 3), 1, 1)


def test_module_on_cpu_is_the_function_bit_for_bit(monkeypatch):
    torch.manual_seed(0)
    pack = D.ModulatedDeformConv2dPack(32, 48, 3, 1, 1, bias=True)
    with torch.no_grad():
        pack.conv_offset.weight.normal_(0, 0.05)
        pack.conv_offset.bias.normal_(0, 0.5)
        pack.bias.normal_()
    x = torch.randn(2, 32, 9, 11)
    assert not pack.hip_route(x)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            got = pack(x)
            o1, o2, m = torch.chunk(pack.conv_offset(x), 3, dim=1)
            want = D.modulated_deform_conv2d(x, torch.cat((o1, o2), dim=1), torch.sigmoid(m), pack.weight, pack.bias, 1, 1, 1, 1, 1)
        assert torch.equal(got, want)
    monkeypatch.setenv("SRF_DCN", "0")
    assert not ops.dcn_enabled()
    monkeypatch.delenv("SRF_DCN")
    assert ops.dcn_enabled()
