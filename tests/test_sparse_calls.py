"""The sparse encoder (srfdet3d_amd/sparse.py, plugin/middle_encoders.py) makes the sequence of `ops` calls recorded in
tests/golden/sparse_calls.json -- same calls, same order, same arguments (shapes, strides, which storage: which layers share a rulebook, a
row plan, a bitmap, a device row count; scalars; which optional arguments are None), held as one digest per call.  The file was recorded
from the encoder as it was while rulebooks, plans and counts lay in `SparseConvTensor.indice_dict` under pointer keys
(tests/golden/make_sparse_calls.py); with unchanged kernels, an unchanged sequence gives unchanged bits.  CPU only: the `ops` functions
are replaced by recording stand-ins."""
import functools
import json

import pytest

import make_sparse_calls as gen


@functools.lru_cache(maxsize=None)
def _recorded():
    from srfdet3d_amd import ops
    return gen.record(ops)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases_and_every_op_a_cpu_tensor_reaches():
    assert sorted(_golden()) == sorted(gen.CASES) == sorted(_recorded()) and len(gen.CASES) == 19
    seen = {c["op"] for calls in _recorded().values() for c in calls}
    assert seen == set(gen.STANDINS) - {"densify_bev"} | {"-- counts --"}      # (densify_bev: behind an is_cuda test)
    ops_of = lambda case: [line.rsplit(" ", 1)[0] for line in _golden()[case]]
    # the 32-channel order plan: only above ops.SPCONV_ORDER_MIN_ROWS, once for the strided 16 -> 32 rulebook, once for the level's SubM one
    assert [ops_of(f"srfdet_voxel_nusc_L/static/{n}").count("spconv_order") for n in gen.ROWS] == [0, 2]
    # train(): no packed weight and no plan
    assert set(ops_of(gen.TRAIN_CASE)) == {"bitmap_build", "rulebook_subm_bitmap", "rulebook_strided_bitmap", "spconv_fwd", "densify"}


@pytest.mark.parametrize("case", gen.CASES)
def test_encoder_makes_the_recorded_calls(case):
    got, want = _recorded()[case], _golden()[case]
    assert [g["op"] for g in got] == [w.rsplit(" ", 1)[0] for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert gen.brief(g) == w, f"call {i}: {json.dumps(g, sort_keys=True)}"


@pytest.mark.parametrize("case", [c for c in gen.CASES if "/static/" in c])
def test_index_pass_makes_the_index_calls_of_the_forward(case):
    """`SparseEncoderCustom.index_pass` -- what the static frame runs on its second stream -- makes, in order and on the same shared
    objects, the calls of the single-stream forward that are no convolution, weight pack or densify."""
    import torch
    from srfdet3d_amd import ops
    config, _, rows = case.split("/")
    enc = gen.encoder(config).eval().requires_grad_(False)
    calls = []
    with gen.recording(ops, calls), torch.no_grad():
        x = gen.sorted_input(enc, int(rows), 1, gen.static_caps(enc, int(rows)))
        steps = sum(1 for _ in enc.index_pass(x.level))
    assert steps == 2 + len(enc.encoder_layers)                # one per top-level module: one event each
    assert gen.index_calls(calls) == gen.index_calls(_recorded()[case]) and len(calls) > 10
    assert [(k, out.rows_dev.shape, out.indices.shape[0]) for k, out in x.level.chain()] == \
        [(k, torch.Size([1]), cap) for k, cap in gen.static_caps(enc, int(rows)).items() if k != "__rows__"]


def test_the_stand_ins_are_taken_off_again():
    from srfdet3d_amd import ops
    _recorded()
    for name in (*gen.STANDINS, "spconv_packed_supported"):
        assert getattr(ops, name).__module__ == ops.__name__, name
