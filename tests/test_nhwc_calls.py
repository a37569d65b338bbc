"""The channels-last executor (srfdet3d_amd/nhwc.py) makes the sequence of `ops` calls recorded in tests/golden/nhwc_calls.json -- same
kernels, same order, same arguments (shapes, strides, storage offsets, which buffer a slice lies in, scalars, which optional arguments
are None), held as one digest per kernel call.  The file was recorded from the executor as it was before its gates and forwards were written over one plan per network
(tests/golden/make_nhwc_calls.py); with unchanged kernels, an unchanged sequence gives unchanged bits.  CPU only: the `ops` functions
are replaced by recording stand-ins."""
import functools
import json

import pytest

import make_nhwc_calls as gen

CASES = ["vovnet99", "vovnet99/upto_stage3", "vovnet19/stem_out", "vovnet99/wino43_off", "vovnet99+fpn/bf16", "fpn/img", "fpn/img_consumer",
         "fpn/bev_bn_extra", "second/voxel", "second/pillar", "second/128"]


@functools.lru_cache(maxsize=None)
def _recorded():
    from srfdet3d_amd import nhwc, ops
    return gen.record(nhwc, ops)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases_and_every_op_of_the_executor():
    assert sorted(_golden()) == sorted(CASES) == sorted(_recorded())
    seen = {c["op"] for calls in _recorded().values() for c in calls}
    assert seen == set(gen.STANDINS) | {"nhwc_maxpool3s2_ceil", "-- routes --"}
    calls = {k: sum(1 + int(line.split()[-2]) for line in v) for k, v in _golden().items()}      # kernel calls + their pack calls
    assert (calls["vovnet99"], calls["fpn/img"], calls["second/128"]) == (265, 24, 35) == tuple(len(_recorded()[k]) for k in ("vovnet99", "fpn/img", "second/128"))


@pytest.mark.parametrize("case", CASES)
def test_executor_makes_the_recorded_calls(case):
    got, want = gen.layers(_recorded()[case]), _golden()[case]
    assert [gen.brief(g).rsplit(" ", 1)[0] for g in got] == [w.rsplit(" ", 1)[0] for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert gen.brief(g) == w, f"kernel call {i}: {json.dumps(g, sort_keys=True)}"


def test_the_bf16_mode_reports_a_route_for_every_layer():
    routes = _recorded()["vovnet99+fpn/bf16"][-1]
    assert routes["op"] == "-- routes --" and len(routes["args"]) == 106 and {r["route"] for r in routes["args"]} == {"bf16"}
    assert gen.brief([routes]) == _golden()["vovnet99+fpn/bf16"][-1]


def test_the_stand_ins_are_taken_off_again_and_pack_calls_are_looked_up_by_name():
    from srfdet3d_amd import nhwc, ops
    _recorded()
    for name in (*gen.STANDINS, "nhwc_maxpool3s2_ceil", "nhwc_ld", "wino43_supported"):
        assert getattr(ops, name).__module__ == ops.__name__, name
    assert all(isinstance(v, str) and callable(getattr(ops, v)) for v in nhwc._PACK.values())


def test_one_call_builds_one_plan(monkeypatch):
    """Gate + forward through the entry a caller uses: every conv -> BatchNorm -> ReLU triple of V-99-eSE (3 stem layers, 16 blocks of 5
    layers and a concat convolution) is looked at once, and the calls are those of the forward alone."""
    import make_nhwc_gate as gate
    import torch
    from srfdet3d_amd import nhwc, ops
    seen, real = [], nhwc._cbr
    monkeypatch.setattr(nhwc, "_cbr", lambda mods: seen.append(1) or real(mods))
    net, calls = gen.vovnet(), []
    with gate.stubbed(), gen.recording(nhwc, ops, calls), torch.no_grad():
        out = nhwc.vovnet(net, gen._image())
    assert list(out) == gen.STAGES and len(seen) == 3 + 16 * 6 == 99
    assert [gen.brief(c) for c in gen.layers(calls)] == _golden()["vovnet99"]
    with gen._env("SRF_IMG_NHWC", "0"), gate.stubbed():
        assert nhwc.vovnet(net, gen._image()) is None and len(seen) == 99      # refused before any walk
