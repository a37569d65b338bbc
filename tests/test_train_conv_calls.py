"""The autograd nodes of srfdet3d_amd/train_conv.py make the sequence of `ops` calls recorded in tests/golden/train_conv_calls.json
-- same kernels, same order, same arguments (shapes, strides, scalars, which optional arguments are None) -- forward and backward.
The file was recorded from the nodes as they were before they were written over one layer primitive
(tests/golden/make_train_conv_calls.py); with unchanged kernels, an unchanged sequence gives unchanged bits.  CPU only: the `ops`
functions are replaced by recording stand-ins."""
import functools
import json

import pytest

import make_train_conv_calls as gen

CASES = ["_Wino43Conv", "_Wino43Conv/nchw_no_bias", "_ConvAffineRelu/3x3", "_ConvAffineRelu/1x1_bias_frozen", "_OSAChain",
         "_OSAChain/frozen_x", "_Conv1x1", "_ESEApply"]


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
    assert seen == set(gen.STANDINS) | {"-- backward --"}


@pytest.mark.parametrize("case", CASES)
def test_node_makes_the_recorded_calls(case):
    got, want = json.loads(json.dumps(_recorded()[case])), _golden()[case]
    assert [c["op"] for c in got] == [c["op"] for c in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {i} ({w['op']})"


def test_the_stand_ins_are_taken_off_again():
    from srfdet3d_amd import ops
    _recorded()
    for name in gen.STANDINS:
        assert getattr(ops, name).__module__ == ops.__name__, name
