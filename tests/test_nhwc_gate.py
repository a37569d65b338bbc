"""The gates of the channels-last executor say yes and no where they did before they were rewritten over one plan per network and the
limit functions of srfdet3d_amd/ops.py.  Every verdict of tests/golden/nhwc_gate.json was recorded from the gates as they were
(tests/golden/make_nhwc_gate.py: meta tensors, `fusable` stubbed to true); TABLE repeats, in the open, the rows that were measured
when the rewrite was asked for.  The limit functions carry their verdict and its source line as tests/test_train_conv_limits.py
does; the tensor gate `nhwc.takes` is pinned row by row.  CPU only."""
import functools
import json

import pytest
import torch

import make_nhwc_calls as calls
import make_nhwc_gate as gen
from srfdet3d_amd import nhwc, ops

P30 = 1 << 30
TABLE = {
    "V-99-eSE 1x3x32x48": True,
    "V-99-eSE 6x3x928x1600": True,
    "V-99-eSE 1x3x1792x3072": True,
    "V-99-eSE 1x3x1856x3200": False,       # the 768-wide stage-2 buffer reaches 2^30 bytes per image
    "V-99-eSE train(), norm_eval=True": True,      # `VoVNet.train()` leaves the BatchNorms in eval mode
    "V-99-eSE train(), norm_eval=False": False,
    "V-39-eSE": True,
    "V-39-eSE input_ch=5": False,
    "V-19-slim-dw-eSE": False,             # depthwise
    "SECOND 1x128x184x184": True,
    "SECOND 1x128x1500x1500": False,
    "SECOND 100 input channels": False,
    "SECOND(64, [72, 128], [1, 1], [1, 2])": False,
    "FPN channels-last": True,
    "FPN NCHW-contiguous": False,
    "FPN on_output, 5 outputs": True,
    "FPN on_input": False,
    "DPG stair": True,
    "head.img_level_consumer": True,
    "head.img_level_consumer, SRF_IMG_NHWC=0": False,
}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(gen.OUT) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _asked():
    return gen.record()


def test_the_fixture_holds_every_row_and_both_verdicts():
    g = _golden()
    assert sorted(g) == sorted(_asked())
    assert {k: g[k] for k in TABLE} == TABLE
    for part in ("V-", "SECOND", "FPN", "DPG stair", "/pts_neck"):
        assert {v for k, v in g.items() if part in k} == {True, False}, part
    assert sum(k.split("/")[0] in gen.CONFIGS for k in g) == 2 * 11 + 3 + 6      # BEV backbone and neck of all eleven; 3 VoVNets, 6 image necks


@pytest.mark.parametrize("row", sorted(json.load(open(gen.OUT))))
def test_gate_verdict_is_the_recorded_one(row):
    assert _asked()[row] is _golden()[row]


# (function, arguments, verdict, reason)
LIMITS = [
    (ops.quads_ok, (64,), True, "csrc/conv.hip:907"),
    (ops.quads_ok, (66,), False, "66 & 3 (csrc/conv.hip:907; srf_gemm_check_1x1: x_ld & 3, csrc/gemm_host.hpp; csrc/nhwc.hip:65)"),
    (ops.operand_ok, (64, 4096), True, "srf_gemm_check_1x1: x_ld & 3, (uintptr_t)x & 15 (csrc/gemm_host.hpp)"),
    (ops.operand_ok, (64, 4104), False, "8 bytes past a 16-byte boundary: (uintptr_t)x & 15 (csrc/conv.hip:907; srf_gemm_check_1x1 and srf_gemm_check_conv, csrc/gemm_host.hpp)"),
    (ops.operand_ok, (62, 4096), False, "x_ld & 3 (csrc/conv.hip:907; srf_gemm_check_1x1 and srf_gemm_check_conv, csrc/gemm_host.hpp)"),
    (ops.wino3x3_channels_ok, (8,), True, "csrc/conv.hip:885"),
    (ops.wino3x3_channels_ok, (12,), False, "12 & 7: srf_wino3x3_packed_weight_bytes answers 0 (csrc/conv.hip:885), the launch refuses (:907)"),
    (ops.wino3x3_range_ok, ((1 << 22) - 1, 64), True, "256 (2^22 - 1) = 2^30 - 256 (csrc/conv.hip:909)"),
    (ops.wino3x3_range_ok, (1 << 22, 64), False, "256 * 2^22 = 2^30: `>=` refuses (csrc/conv.hip:909)"),
    (ops.stem_channels_ok, (3, 64), True, "csrc/conv.hip:1352"),
    (ops.stem_channels_ok, (4, 64), True, "Cin > 4 refuses (csrc/conv.hip:1352)"),
    (ops.stem_channels_ok, (5, 64), False, "Cin > 4 (csrc/conv.hip:1352)"),
    (ops.stem_channels_ok, (3, 32), False, "Cout != 64 (csrc/conv.hip:1352)"),
    (ops.ese_channels_ok, (1024,), True, "as the gate held it: out_channels <= 1024"),
    (ops.ese_channels_ok, (1028,), False, "as the gate held it: out_channels > 1024 (the bound of srf_nhwc_colmean, csrc/nhwc.hip:137)"),
    (ops.ese_channels_ok, (1022,), False, "C & 3: srf_ese_gate (csrc/decoder.hip:445), srf_nhwc_affine (csrc/nhwc.hip:65)"),
    (ops.gemm_k_ok, (768,), True, "the 768-wide buffer of a stage-2 block of V-99-eSE (srf_gemm_check_1x1: K & 31, csrc/gemm_host.hpp)"),
    (ops.gemm_k_ok, (720,), False, "the stage-5 buffer of V-19-slim-eSE: 720 & 31 (srf_gemm_check_1x1: K & 31, csrc/gemm_host.hpp)"),
    # the executor applies the range of srf_wino3x3 to every buffer a 3x3 layer reads, whichever Winograd kernel runs the layer
    (nhwc._img_fits, (1024, 1024, 255), True, "`4 * H * W * ld < (1 << 30)`, as the gates held it"),
    (nhwc._img_fits, (1024, 1024, 256), False, "2^30 (csrc/conv.hip:909)"),
    (nhwc._img_fits, (464, 800, 768), False, "1.14e9 bytes: stage 2 of V-99-eSE at 1856 x 3200"),
    (nhwc._img_fits, (448, 768, 768), True, "1.06e9 bytes: stage 2 of V-99-eSE at 1792 x 3072"),
]


@pytest.mark.parametrize("fn,args,want,why", LIMITS, ids=[f"{r[0].__name__}{r[1]}" for r in LIMITS])
def test_limit(fn, args, want, why):
    assert fn(*args) is want, why


def test_the_shape_walk_gives_the_buffers_of_v99():
    """`plan_shapes` at 6 x 928 x 1600: the stem at 464 x 800 x 64, then per stage the block buffers, Cin + 5 w wide, at 232 x 400,
    116 x 200, 58 x 100 and 29 x 50 -- the one place these numbers are computed."""
    plan = nhwc.vovnet_plan(calls.vovnet())
    assert nhwc.plan_shapes(plan, 928, 1600)[0][1] == (464, 800, 64, 0, 64)
    outs = [slot for s, slot in nhwc.plan_shapes(plan, 928, 1600) if s.kind == "out"]
    assert outs == [(232, 400, 256, 0, 256), (116, 200, 512, 0, 512), (58, 100, 768, 0, 768), (29, 50, 1024, 0, 1024)]
    widths = sorted({slot.width for s, slot in nhwc.plan_shapes(plan, 928, 1600) if s.kind == "layer"})
    assert widths == [128 + 5 * 128, 256 + 5 * 160, 512 + 5 * 160, 512 + 5 * 192, 768 + 5 * 192, 768 + 5 * 224, 1024 + 5 * 224]
    assert nhwc.plan_shapes(plan, 1856, 3200) is None and nhwc.plan_shapes(plan, 1792, 3072) is not None


def test_the_tensor_gate(monkeypatch):
    """`nhwc.takes`: the switch, `dense.fusable`, and channels-last strides where asked -- the condition its seven call sites spelled out."""
    nchw, cl = gen.meta(2, 8, 4, 4), gen.meta(2, 8, 4, 4, channels_last=True)
    assert nhwc.takes() is True                                             # no tensor: the switch alone
    assert not nhwc.takes(torch.zeros(2, 8, 4, 4))                          # a CPU tensor is not fusable
    with gen.stubbed():
        assert nhwc.takes(nchw) and nhwc.takes(cl) and nhwc.takes(cl, channels_last=True)
        assert not nhwc.takes(nchw, channels_last=True)
        assert not nhwc.takes(gen.meta(2, 1, 4, 4, channels_last=True), channels_last=True)     # one channel: both layouts at once
        assert not nhwc.takes(gen.meta(8, 4, 4), channels_last=True)
        monkeypatch.setenv("SRF_IMG_NHWC", "0")
        assert not nhwc.takes() and not nhwc.takes(cl) and not nhwc.takes(cl, channels_last=True)
        monkeypatch.setenv("SRF_IMG_NHWC", "1")
        assert nhwc.takes(cl, channels_last=True)


def test_the_switches_are_listed_once(monkeypatch):
    assert sorted(nhwc._SWITCHES) == ["FPN_FORK", "IMG_NHWC", "WINO43"]
    for name in nhwc._SWITCHES:
        monkeypatch.delenv("SRF_" + name, raising=False)
    assert (nhwc.switch("IMG_NHWC"), nhwc.switch("WINO43"), nhwc.switch("FPN_FORK")) == ("1", "1", "2")
    assert nhwc.enabled() and nhwc.wino43_enabled()
    monkeypatch.setenv("SRF_WINO43", "0")
    assert nhwc.enabled() and not nhwc.wino43_enabled()
    with pytest.raises(KeyError):
        nhwc.switch("GEMM_SPLIT")      # a switch of ops.py
