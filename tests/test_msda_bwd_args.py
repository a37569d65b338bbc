"""Host side of the multi-scale deformable attention backward (no GPU): the C ABI's declaration, export and argument validation, the CPU
behaviour of the Python layer, and that the attention module on CPU tensors still trains through the torch core."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from srfdet3d_amd import _lib, ops
from srfdet3d_amd.compat import transformer as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "srfdet3d.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+srf_msda_bwd\s*\(", header)
    assert "srf_msda_bwd" in _lib.SIGNATURES
    L = _lib.lib()
    assert L.srf_msda_bwd is not None
    decl = re.search(r"\bint\s+srf_msda_bwd\s*\(([^;]*)\)\s*;", header).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["srf_msda_bwd"][1]) == 23
    assert L.srf_abi_version() == 1
    text = header[header.index("/* srf_msda_bwd"):header.index("int srf_msda_bwd")]
    assert "ADDS" in text and "atomic" in text and "arrive" in text          # the header says what is and is not reproducible


def _call(L, B=1, shapes=((16, 12), (8, 6), (4, 3), (2, 1)), Q=254, heads=8, d=16, P=4, value_ld=None, offs_ld=None, logits_ld=None,
          gout_ld=None, gvalue_ld=None, goffs_ld=None, glogits_ld=None, ptr=None, no_shapes=False, outs=None, **tensors):
    """`ptr` stands for every tensor not named; `outs` (default `ptr`) for the three outputs not named."""
    nl = len(shapes)
    C, ns = heads * d, heads * nl * P
    flat = None if no_shapes else _lib.hi([v for hw in shapes for v in hw])
    outs = ptr if outs is None else (None if outs == "null" else outs)
    pick = lambda name, default: tensors.get(name, default)
    ld = lambda v, width: width if v is None else v
    return L.srf_msda_bwd(pick("value", ptr), ld(value_ld, C), B, flat, nl, pick("ref", ptr), pick("offs", ptr), ld(offs_ld, 2 * ns),
                          pick("logits", ptr), ld(logits_ld, ns), Q, heads, d, P, pick("grad_out", ptr), ld(gout_ld, C),
                          pick("grad_value", outs), ld(gvalue_ld, C), pick("grad_offs", outs), ld(goffs_ld, 2 * ns),
                          pick("grad_logits", outs), ld(glogits_ld, ns), None)


def test_argument_validation_before_any_hip_call():
    L = _lib.lib()
    ok = ctypes.c_void_p(4096)        # an aligned non-null address that is never dereferenced: every call below returns before a launch
    # nothing to do: all three outputs NULL (whatever the inputs), or no rows
    assert _call(L) == 0 and _call(L, ptr=ok, outs="null") == 0
    assert _call(L, B=0, ptr=ok) == 0 and _call(L, Q=0, ptr=ok) == 0 and _call(L, B=0) == 0
    # null inputs with an output wanted
    assert _call(L, grad_value=ok) == EINVAL and _call(L, grad_offs=ok) == EINVAL and _call(L, grad_logits=ok) == EINVAL
    for name in ("value", "ref", "offs", "logits", "grad_out"):
        assert _call(L, ptr=ok, **{name: None}) == EINVAL, name
    assert _call(L, B=-1) == EINVAL and _call(L, Q=-1) == EINVAL
    assert _call(L, heads=0) == EINVAL and _call(L, d=0) == EINVAL and _call(L, P=0) == EINVAL and _call(L, shapes=()) == EINVAL
    assert _call(L, no_shapes=True) == EINVAL
    assert _call(L, shapes=((16, 12), (0, 6))) == EINVAL and _call(L, shapes=((16, -1),)) == EINVAL
    assert _call(L, value_ld=124) == EINVAL and _call(L, gout_ld=64) == EINVAL              # a pitch below the row's width
    assert _call(L, offs_ld=255) == EINVAL and _call(L, logits_ld=127) == EINVAL
    assert _call(L, ptr=ok, gvalue_ld=124) == EINVAL and _call(L, ptr=ok, goffs_ld=255) == EINVAL and _call(L, ptr=ok, glogits_ld=127) == EINVAL
    assert _call(L, gvalue_ld=124) == 0 and _call(L, ptr=ok, outs="null", goffs_ld=1) == 0  # a NULL output's pitch is ignored
    # the documented unsupported cases, in the forward's order: before the nothing-to-do answer and the null pointers
    assert _call(L, d=8) == EUNSUPPORTED and _call(L, d=64) == EUNSUPPORTED and _call(L, d=24) == EUNSUPPORTED
    assert _call(L, shapes=((2, 2),) * 5) == EUNSUPPORTED and _call(L, P=5) == EUNSUPPORTED
    assert _call(L, B=4200000) == EUNSUPPORTED                                             # 2 GiB of value rows (254 rows of 512 B each)
    assert _call(L, shapes=((2048, 2048),), Q=1) == EUNSUPPORTED                           # 2 GiB in one level
    assert _call(L, B=1, Q=2100000) == EUNSUPPORTED                                        # 2 GiB of offsets
    # the new tensors alone past 2 GiB (the inputs stay NULL: the same sizes with the forward's pitches end in EINVAL, so they are taken)
    assert _call(L, Q=1100000, grad_value=ok) == EINVAL and _call(L, Q=1100000, gout_ld=512, grad_value=ok) == EUNSUPPORTED
    assert _call(L, B=16500, Q=1, grad_value=ok) == EINVAL and _call(L, B=16500, Q=1, gvalue_ld=132, grad_value=ok) == EUNSUPPORTED
    assert _call(L, Q=1050000, grad_offs=ok) == EINVAL and _call(L, Q=1050000, goffs_ld=1024, grad_offs=ok) == EUNSUPPORTED
    assert _call(L, Q=1050000, grad_logits=ok) == EINVAL and _call(L, Q=1050000, glogits_ld=1024, grad_logits=ok) == EUNSUPPORTED
    assert _call(L, Q=1050000, glogits_ld=1024, grad_offs=ok) == EINVAL                    # ... and not where that output is NULL
    assert _call(L, value_ld=130, ptr=ok) == EUNSUPPORTED and _call(L, gout_ld=134, ptr=ok) == EUNSUPPORTED   # pitch % 4
    assert _call(L, offs_ld=258, ptr=ok) == EUNSUPPORTED and _call(L, logits_ld=129, ptr=ok) == EUNSUPPORTED
    assert _call(L, gvalue_ld=130, ptr=ok) == EUNSUPPORTED and _call(L, goffs_ld=258, ptr=ok) == EUNSUPPORTED
    assert _call(L, glogits_ld=129, ptr=ok) == EUNSUPPORTED
    odd = ctypes.c_void_p(4096 + 8)
    for name in ("value", "ref", "offs", "logits", "grad_out", "grad_value", "grad_offs", "grad_logits"):
        assert _call(L, ptr=ok, **{name: odd}) == EUNSUPPORTED, name                       # a base that is not 16-byte aligned
    # taken: head_dim 16 and 32, L = 1, P = 1, wider pitches -- then the null inputs
    assert _call(L, d=32, grad_value=ok) == EINVAL and _call(L, shapes=((5, 7),), Q=3, P=1, grad_offs=ok) == EINVAL
    assert _call(L, value_ld=192, offs_ld=384, logits_ld=384, gout_ld=132, gvalue_ld=192, goffs_ld=384, glogits_ld=384, grad_logits=ok) == EINVAL


def test_ops_refuse_cpu_tensors():
    shapes = [(4, 3)]
    value, ref = torch.zeros(12, 128), torch.zeros(12, 1, 2)
    offs, logits = torch.zeros(12, 64), torch.zeros(12, 32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.msda_backward(value, shapes, ref, offs, logits, 8, 4, torch.zeros(12, 128))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.msda_autograd(value, shapes, ref, offs, logits, 8, 4)


def test_train_switch_follows_both_variables(monkeypatch):
    monkeypatch.delenv("SRF_MSDA", raising=False)
    monkeypatch.delenv("SRF_MSDA_TRAIN", raising=False)
    assert ops.msda_train_enabled()
    monkeypatch.setenv("SRF_MSDA_TRAIN", "0")
    assert not ops.msda_train_enabled() and ops.msda_enabled()
    monkeypatch.delenv("SRF_MSDA_TRAIN")
    monkeypatch.setenv("SRF_MSDA", "0")
    assert not ops.msda_train_enabled()


def test_attention_on_cpu_tensors_trains_through_the_torch_core(monkeypatch):
    """Under grad on CPU tensors the module takes `multi_scale_deformable_attn_pytorch` and never the node; its float32 gradients are
    what the same module computes in float64, to float32 rounding."""
    shapes = [(4, 3), (2, 1)]
    S, C = 14, 128
    calls = []
    core = T.multi_scale_deformable_attn_pytorch
    monkeypatch.setattr(T, "multi_scale_deformable_attn_pytorch", lambda *a: (calls.append("torch"), core(*a))[1])
    monkeypatch.setattr(ops, "msda_autograd", lambda *a, **k: pytest.fail("the node ran on CPU tensors"))
    torch.manual_seed(3)
    att = T.MultiScaleDeformableAttention(embed_dims=C, num_levels=2, num_points=3, dropout=0.0)
    with torch.no_grad():
        att.sampling_offsets.weight.normal_(0, 0.05)
        att.attention_weights.weight.normal_(0, 0.1)
    x = torch.randn(S, 2, C)
    pos = torch.randn(S, 2, C) * 0.5
    refp = torch.rand(2, S, 2, 2)
    cot = torch.randn(S, 2, C)
    grads = {}
    for dtype in (torch.float32, torch.float64):
        m = T.MultiScaleDeformableAttention(embed_dims=C, num_levels=2, num_points=3, dropout=0.0).to(dtype)
        m.load_state_dict({k: v.to(dtype) for k, v in att.state_dict().items()})
        q = x.to(dtype).clone().requires_grad_()
        out = m(q, query_pos=pos.to(dtype), reference_points=refp.to(dtype), spatial_shapes=shapes)
        (out * cot.to(dtype)).sum().backward()
        grads[dtype] = [q.grad] + [p.grad for p in m.parameters()]
    assert calls == ["torch", "torch"]
    for g32, g64 in zip(grads[torch.float32], grads[torch.float64]):
        err = (g32.double() - g64).abs().max().item() / g64.abs().max().item()
        assert np.isfinite(err) and err < 1e-4, err
