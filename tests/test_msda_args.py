"""Host side of the multi-scale deformable attention operator (no GPU): the C ABI's declaration, export and argument validation, the
shape predicate, the CPU behaviour of the Python layer."""
import ctypes
import os
import re

import pytest
import torch

from srfdet3d_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "srfdet3d.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+srf_msda_fwd\s*\(", header)
    assert "srf_msda_fwd" in _lib.SIGNATURES
    L = _lib.lib()
    assert L.srf_msda_fwd is not None
    decl = re.search(r"\bint\s+srf_msda_fwd\s*\(([^;]*)\)\s*;", header).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["srf_msda_fwd"][1])
    assert L.srf_abi_version() == 1


def _call(L, B=1, shapes=((16, 12), (8, 6), (4, 3), (2, 1)), Q=254, heads=8, d=16, P=4, value_ld=None, offs_ld=None, logits_ld=None,
          out_ld=None, ptr=None, no_shapes=False, value=None, ref=None, offs=None, logits=None, out=None):
    nl = len(shapes)
    C, ns = heads * d, heads * nl * P
    flat = None if no_shapes else _lib.hi([v for hw in shapes for v in hw])
    pick = lambda p: ptr if p is None else p
    return L.srf_msda_fwd(pick(value), C if value_ld is None else value_ld, B, flat, nl, pick(ref), pick(offs),
                          2 * ns if offs_ld is None else offs_ld, pick(logits), ns if logits_ld is None else logits_ld, Q, heads, d, P,
                          pick(out), C if out_ld is None else out_ld, None)


def test_argument_validation_before_any_hip_call():
    L = _lib.lib()
    ok = ctypes.c_void_p(4096)        # an aligned non-null address that is never dereferenced: every call below is refused first
    assert _call(L) == EINVAL                                         # null tensors with B Q > 0
    assert _call(L, B=0) == 0 and _call(L, Q=0) == 0                  # the empty call is nothing to do
    assert _call(L, B=-1) == EINVAL and _call(L, Q=-1) == EINVAL
    assert _call(L, heads=0) == EINVAL and _call(L, d=0) == EINVAL and _call(L, P=0) == EINVAL and _call(L, shapes=()) == EINVAL
    assert _call(L, no_shapes=True) == EINVAL
    assert _call(L, shapes=((16, 12), (0, 6))) == EINVAL and _call(L, shapes=((16, -1),)) == EINVAL
    assert _call(L, value_ld=124) == EINVAL and _call(L, out_ld=64) == EINVAL              # a pitch below the row's width
    assert _call(L, offs_ld=255) == EINVAL and _call(L, logits_ld=127) == EINVAL
    # the documented unsupported cases
    assert _call(L, d=8) == EUNSUPPORTED and _call(L, d=64) == EUNSUPPORTED and _call(L, d=24) == EUNSUPPORTED
    assert _call(L, shapes=((2, 2),) * 5) == EUNSUPPORTED and _call(L, P=5) == EUNSUPPORTED
    assert _call(L, B=4200000) == EUNSUPPORTED                                             # 2 GiB of value rows (254 rows of 512 B each)
    assert _call(L, shapes=((2048, 2048),), Q=1) == EUNSUPPORTED                           # 2 GiB in one level
    assert _call(L, B=1, Q=2100000) == EUNSUPPORTED                                        # 2 GiB of offsets
    assert _call(L, value_ld=130, ptr=ok) == EUNSUPPORTED and _call(L, out_ld=134, ptr=ok) == EUNSUPPORTED   # pitch % 4
    assert _call(L, offs_ld=258, ptr=ok) == EUNSUPPORTED and _call(L, logits_ld=129, ptr=ok) == EUNSUPPORTED
    odd = ctypes.c_void_p(4096 + 8)
    for name in ("value", "ref", "offs", "logits", "out"):
        assert _call(L, ptr=ok, **{name: odd}) == EUNSUPPORTED, name                       # a base that is not 16-byte aligned
    # taken: head_dim 16 and 32, L = 1, P = 1, wider pitches -- then the null pointers
    assert _call(L, d=32) == EINVAL and _call(L, shapes=((5, 7),), Q=3, P=1) == EINVAL
    assert _call(L, value_ld=192, offs_ld=384, logits_ld=384, out_ld=132) == EINVAL


def test_msda_supported_answers_as_documented():
    S = 254
    assert ops.msda_supported(2, S, S, 8, 16, 4, 4) and ops.msda_supported(1, S, 3, 8, 32, 4, 4)
    assert ops.msda_supported(1, 35, 35, 8, 16, 1, 1) and ops.msda_supported(1, 44965, 44965, 8, 16, 4, 4)
    assert ops.msda_supported(0, S, 0, 8, 16, 4, 4)
    assert not ops.msda_supported(1, S, S, 8, 8, 4, 4) and not ops.msda_supported(1, S, S, 8, 64, 4, 4)
    assert not ops.msda_supported(1, S, S, 8, 16, 5, 4) and not ops.msda_supported(1, S, S, 8, 16, 4, 5)
    assert not ops.msda_supported(1, S, S, 8, 16, 0, 4) and not ops.msda_supported(1, S, S, 0, 16, 4, 4)
    assert ops.msda_supported(1, S, S, 8, 16, 4, 4, value_ld=192, offs_ld=384, logits_ld=384, out_ld=132)
    assert not ops.msda_supported(1, S, S, 8, 16, 4, 4, value_ld=130) and not ops.msda_supported(1, S, S, 8, 16, 4, 4, out_ld=124)
    assert not ops.msda_supported(1, S, S, 8, 16, 4, 4, offs_ld=258) and not ops.msda_supported(1, S, S, 8, 16, 4, 4, logits_ld=126)
    assert not ops.msda_supported(4200000, S, 1, 8, 16, 4, 4) and not ops.msda_supported(1, S, 2100000, 8, 16, 4, 4)
    # the predicate and the entry point agree on the 2 GiB edge of the value table (null tensors: a shape that is taken ends in EINVAL)
    L = _lib.lib()
    for B in (16500, 16512, 16513, 16600):      # B x 254 rows x 512 B around 2^31
        assert ops.msda_supported(B, S, 1, 8, 16, 4, 4) == (B * S * 512 < 2 ** 31)
        assert _call(L, B=B, Q=1) == (EINVAL if B * S * 512 < 2 ** 31 else EUNSUPPORTED)


def test_ops_refuse_cpu_tensors(monkeypatch):
    shapes = [(4, 3)]
    value, ref = torch.zeros(12, 128), torch.zeros(12, 1, 2)
    offs, logits = torch.zeros(12, 64), torch.zeros(12, 32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.msda(value, shapes, ref, offs, logits, 8, 4)
    monkeypatch.setenv("SRF_MSDA", "0")
    assert not ops.msda_enabled()
    monkeypatch.delenv("SRF_MSDA")
    assert ops.msda_enabled()
