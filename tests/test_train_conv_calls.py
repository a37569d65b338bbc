"""The autograd nodes of srfdet3d_amd/train_conv.py make the sequence of `ops` calls recorded in tests/golden/train_conv_calls.json
-- same kernels, same order, same arguments (shapes, strides, scalars, which optional arguments are None) -- forward and backward.
The file was recorded from the nodes as they were before they were written over one layer primitive
(tests/golden/make_train_conv_calls.py); with unchanged kernels, an unchanged sequence gives unchanged bits.  The `<case>/bf16`
records -- the same nodes inside `train_conv.mfma_dtype(torch.bfloat16)`, with the mode's route report -- were recorded before the
three bf16-product modes were put on one context class (srfdet3d_amd/mfma_mode.py).  CPU only: the `ops` functions are replaced by
recording stand-ins."""
import functools
import json

import pytest

import make_train_conv_calls as gen

CASES = ["_Wino43Conv", "_Wino43Conv/nchw_no_bias", "_ConvAffineRelu/3x3", "_ConvAffineRelu/1x1_bias_frozen", "_OSAChain",
         "_OSAChain/frozen_x", "_Conv1x1", "_ESEApply"]
# inside the mode: every executed direction of every case is on the bf16 route (so that no f32 sequence can be recorded in its place)
BF16_DIRECTIONS = {"_Wino43Conv": 3, "_Wino43Conv/nchw_no_bias": 3, "_ConvAffineRelu/3x3": 3, "_ConvAffineRelu/1x1_bias_frozen": 2,
                   "_OSAChain": 9, "_OSAChain/frozen_x": 8, "_Conv1x1": 3}
CASES += [c + gen.BF16 for c in BF16_DIRECTIONS]


@functools.lru_cache(maxsize=None)
def _recorded():
    from srfdet3d_amd import ops, train_conv
    return gen.record(train_conv, ops)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases_and_every_op_of_the_nodes():
    assert sorted(_golden()) == sorted(CASES) == sorted(_recorded())
    seen = {c["op"] for calls in _golden().values() for c in calls}
    assert seen == set(gen.STANDINS) | {"-- backward --", "-- routes --"}


@pytest.mark.parametrize("case", CASES)
def test_node_makes_the_recorded_calls(case):
    got, want = json.loads(json.dumps(_recorded()[case])), _golden()[case]
    assert [c["op"] for c in got] == [c["op"] for c in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i} ({w['op']})"


@pytest.mark.parametrize("case", list(BF16_DIRECTIONS))
def test_in_the_mode_every_direction_takes_the_bf16_route(case):
    for rec in (_recorded(), _golden()):
        routes = rec[case + gen.BF16][-1]
        assert routes["op"] == "-- routes --" and len(routes["args"]) == BF16_DIRECTIONS[case]
        assert [(r["route"], r["why"]) for r in routes["args"]] == [("bf16", None)] * BF16_DIRECTIONS[case]
        assert not any(c["op"] in ("wino43", "pack_wino43_weights", "conv_wgrad_nhwc") for c in rec[case + gen.BF16])


def test_a_route_record_keeps_its_key_order():
    """(the fixture is written with sorted keys; the order is that of the record the mode builds)"""
    for case in BF16_DIRECTIONS:
        assert all(list(r) == ["layer", "direction", "route", "why"] for r in _recorded()[case + gen.BF16][-1]["args"])


def test_the_stand_ins_are_taken_off_again():
    from srfdet3d_amd import ops
    _recorded()
    for name in (*gen.STANDINS, "nhwc_ld"):
        assert getattr(ops, name).__module__ == ops.__name__, name
