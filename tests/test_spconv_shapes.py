"""Which (K, Cin, Cout) has which sparse-convolution kernel and which row plan: the answers of the five shape questions `ops` asks the
built library (csrc/spconv_frame.hpp, srf_spconv_shape), over a grid of every layer shape in use and their neighbours, for each value of
the SRF_SPCONV_ORDER switch, against tests/golden/spconv_shapes.json.  The file was recorded from the tree as it was while the rule was
written out in srf_packed_layout, sb_shape_ok, ops.spconv_tiles_wanted and ops.spconv_order_wanted
(`python tests/test_spconv_shapes.py` rewrites it from the tree this file lies in).  Host calls only: no GPU, no launch."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spconv_shapes.json")
KS, CINS, COUTS = (1, 3, 9, 27, 28), (4, 5, 16, 32, 48, 64, 128, 256), (16, 32, 64, 128, 256)
GRID = [(K, cin, cout) for K in KS for cin in CINS for cout in COUTS]
MODES = ("0", "1", "2")
QUESTIONS = ("packed_supported", "bf16_supported", "tiles_wanted", "order_wanted", "order_wanted rows=99999", "order_wanted rows=100000")


def answers(ops, mode):
    """{"K,Cin,Cout": one character per question, '1' = yes} under SRF_SPCONV_ORDER = mode"""
    before = os.environ.get("SRF_SPCONV_ORDER")
    os.environ["SRF_SPCONV_ORDER"] = mode
    try:
        return {f"{K},{cin},{cout}": "".join("1" if a else "0" for a in (
            ops.spconv_packed_supported(K, cin, cout), ops.spconv_bf16_supported(K, cin, cout), ops.spconv_tiles_wanted(cin, cout),
            ops.spconv_order_wanted(cin, cout, K), ops.spconv_order_wanted(cin, cout, K, rows=99_999),
            ops.spconv_order_wanted(cin, cout, K, rows=100_000))) for K, cin, cout in GRID}
    finally:
        if before is None:
            del os.environ["SRF_SPCONV_ORDER"]
        else:
            os.environ["SRF_SPCONV_ORDER"] = before


@pytest.mark.parametrize("mode", MODES)
def test_the_shape_answers_are_the_recorded_ones(mode):
    from srfdet3d_amd import ops
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["questions"] == list(QUESTIONS) and sorted(want["answers"]) == sorted(MODES)
    got = answers(ops, mode)
    assert sorted(got) == sorted(want["answers"][mode]) and len(got) == len(GRID) == 200
    wrong = {k: (got[k], w) for k, w in want["answers"][mode].items() if got[k] != w}
    assert not wrong, wrong


def test_the_recorded_answers_hold_every_kind_of_shape():
    """the grid is no vacuous one: every packed layout, the bf16 form, both plan kinds, and the switch and the row threshold all show"""
    with open(GOLDEN) as f:
        a = json.load(f)["answers"]
    col = lambda mode, q: {k for k, v in a[mode].items() if v[QUESTIONS.index(q)] == "1"}
    assert col("1", "bf16_supported") == {"27,32,64", "27,64,64", "27,64,128", "27,128,128", "3,128,128"} < col("1", "packed_supported")
    assert col("1", "order_wanted") == {"27,16,32", "27,32,32"} == col("2", "order_wanted rows=99999") == col("1", "order_wanted rows=100000")
    assert not col("0", "order_wanted") and not col("1", "order_wanted rows=99999")
    assert "1,64,128" in col("0", "tiles_wanted") and "27,16,32" in col("1", "tiles_wanted") - col("0", "tiles_wanted")
    assert all(col(m, "packed_supported") == col("1", "packed_supported") for m in MODES)


def test_the_recorders_stand_ins_are_the_librarys():
    """the shape rules tests/golden/make_sparse_calls.py stands in for the library with, so that it can record without one"""
    import make_sparse_calls as gen
    from srfdet3d_amd import ops
    for K, cin, cout in GRID:
        assert gen._packed_supported(K, cin, cout) == ops.spconv_packed_supported(K, cin, cout), (K, cin, cout)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from srfdet3d_amd import ops as _ops
    with open(GOLDEN, "w") as f:
        json.dump({"questions": list(QUESTIONS), "answers": {m: answers(_ops, m) for m in MODES}}, f, indent=0, sort_keys=True)
        f.write("\n")
