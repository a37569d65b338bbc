#!/usr/bin/env python3
"""Generate tests/golden/sparse_calls.json: the sequence of `ops` calls the sparse encoder (srfdet3d_amd/sparse.py,
plugin/middle_encoders.py) makes on CPU tensors, for the encoders of three configs on the hash route, the eager bitmap route and the
static (capacity) route, at 5 000 and at 120 000 input rows, plus one train() case.  The `ops` functions the encoder calls are replaced
by stand-ins that record their arguments and return tensors of the right shape: per call the op's name and, for every parameter of the
real function's signature (defaults filled in), a tensor's shape, strides, storage offset and the serial number of its storage in order
of first appearance within the case, a scalar's value, a bitmap level or hash table by the serial of its buffer, null for None.  The
serial is what shows which layers share a rulebook, a row plan, a level's bitmap or its device row count.  A static case ends with a
record of the (indice_key, device count, capacity) list the encoder returns.  The file holds one line per call: the op and a digest of
its record; `--full FILE` writes the records themselves, for comparing two trees call by call.

The stand-ins look at no coordinate: an eager strided conv on A rows gives `live_rows(A)` = 7 * A // 8 + 1 output rows (120 000 -> 105 001:
the 32-channel layers of the second level stay above ops.SPCONV_ORDER_MIN_ROWS, so their order plan is reached), a static one its
capacity, the eager size + 300.  `ops.spconv_packed_supported` and `ops.spconv_plan_kind` are stood in for by their shape rule
(csrc/spconv_frame.hpp, srf_spconv_shape; tests/test_spconv_shapes.py holds the stand-ins to it), so that no library is loaded.  `ops.densify_bev` has a stand-in too, but lies behind an `is_cuda` test that no CPU tensor passes: the
recorded encoders end in `densify`.  tests/test_sparse_calls.py runs the same recorder on the tree under test and compares: same calls,
same order, same arguments, same sharing -- with unchanged kernels, unchanged bits.

The committed file was written from the commit BEFORE rulebooks, plans and row counts moved from `SparseConvTensor.indice_dict` to
`sparse.Level` / `sparse.Rulebook`, from a checkout of it made by hand (this script runs no git command):

usage:  python tests/golden/make_sparse_calls.py [--tree CHECKOUT]      (default: the tree this file lies in)
"""
import argparse
import contextlib
import hashlib
import inspect
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "sparse_calls.json")
CONFIGS = ["srfdet_voxel_nusc_L", "srfdet_voxel_kitti_L", "srfdet_dvoxel_waymo_L"]
ROUTES = ["hash", "bitmap", "static"]
ROWS = [5000, 120000]
TRAIN_CASE = "srfdet_voxel_nusc_L/bitmap/5000/train"
CASES = [f"{c}/{r}/{n}" for c in CONFIGS for r in ROUTES for n in ROWS] + [TRAIN_CASE]
NOT_INDEX = ("spconv_fwd", "pack_spconv_weights", "densify", "densify_bev", "-- counts --")   # every other call is an index call
HEADROOM = 300


def live_rows(a):
    return 7 * a // 8 + 1


class _Serials:
    """Storage -> its number in order of first appearance; the storages are held so that no address comes back within a case."""

    def __init__(self):
        self.seen, self.held = {}, []

    def __call__(self, t):
        s = t.untyped_storage()
        if s.data_ptr() not in self.seen:
            self.seen[s.data_ptr()] = len(self.seen)
            self.held.append(s)
        return self.seen[s.data_ptr()]


class _Handle:
    """What stands for an ops.BitmapLevel (with its grid `shape`) or an ops.CoordTable: told apart by its buffer."""

    def __init__(self, kind, shape=None):
        self.kind, self.shape, self.buf = kind, shape, torch.zeros(1, dtype=torch.int32)


def _describe(v, serial):
    if isinstance(v, torch.Tensor):
        return dict(shape=list(v.shape), stride=list(v.stride()), offset=v.storage_offset(), storage=serial(v))
    if isinstance(v, _Handle):
        return {v.kind: serial(v.buf)}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list)):
        return [_describe(e, serial) for e in v]
    raise TypeError(f"cannot describe {type(v)}")


def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def _out_shape(shape, ksize, stride, pad):
    return [int((shape[d] + 2 * pad[d] - ksize[d]) // stride[d] + 1) for d in range(3)]


def _bitmap_build(indices, spatial_shape, batch, want_order=True, padded=False):
    A = indices.shape[0]
    return _Handle("bitmap", list(spatial_shape)), torch.arange(A, dtype=torch.int32), _i32(A, 4)


def _rulebook_subm_bitmap(sorted_indices, level, ksize, want_counts=True):
    K = math.prod(ksize)
    return _i32(K, sorted_indices.shape[0]), (_i32(K) if want_counts else None)


def _rulebook_strided_bitmap(indices, level, ksize, stride, pad, out_capacity=None):
    K, oshape = math.prod(ksize), _out_shape(level.shape, ksize, stride, pad)
    out_lvl = _Handle("bitmap", oshape)
    if out_capacity is not None:
        return _i32(out_capacity, 4), _i32(K, out_capacity), None, out_lvl, oshape, _i32(1)
    A_out = live_rows(indices.shape[0])
    return _i32(A_out, 4), _i32(K, A_out), _i32(K), out_lvl, oshape


def _rulebook_strided(indices, spatial_shape, batch, ksize, stride, pad):
    K, A_out = math.prod(ksize), live_rows(indices.shape[0])
    return _i32(A_out, 4), _i32(K, A_out), _i32(K), _Handle("table"), _out_shape(spatial_shape, ksize, stride, pad)


def _spconv_fwd(feats, weight, nbr, alpha=None, beta=None, residual=None, relu=False, pair_counts=None, packed=None, rows_dev=None,
                tiles=None, subm=False):
    return torch.zeros(nbr.shape[1], weight.shape[2])


# name -> what the stand-in returns (the arguments are bound to the REAL function's signature first)
STANDINS = {
    "bitmap_build": _bitmap_build,
    "rulebook_subm_bitmap": _rulebook_subm_bitmap,
    "rulebook_strided_bitmap": _rulebook_strided_bitmap,
    "coord_table_build": lambda indices, spatial_shape, batch: _Handle("table"),
    "rulebook_subm": lambda indices, spatial_shape, ksize, table: (_i32(math.prod(ksize), indices.shape[0]), _i32(math.prod(ksize))),
    "rulebook_strided": _rulebook_strided,
    "spconv_tiles": lambda nbr, rows_dev=None: _i32(1),
    "spconv_order": lambda nbr, rows_dev=None: _i32(1),
    "pack_spconv_weights": lambda weight: torch.zeros(1),
    "spconv_fwd": _spconv_fwd,
    "densify": lambda feats, indices, batch, spatial_shape: torch.zeros(batch, feats.shape[1], *spatial_shape),
    "densify_bev": lambda feats, level, batch, spatial_shape: torch.zeros(batch, feats.shape[1] * spatial_shape[0], *spatial_shape[1:]),
}


def _packed_supported(K, Cin, Cout):
    """ops.spconv_packed_supported without the library: srf_spconv_shape of csrc/spconv_frame.hpp."""
    return 0 < K <= 27 and ((K == 27 and Cout == 32 and Cin in (16, 32)) or (Cout == 64 and Cin in (32, 64))
                            or (Cout == 128 and Cin in (64, 128)))


def _plan_kind(K, Cin, Cout):
    """ops.spconv_plan_kind without the library: a row order for the 32-channel layout, row ranges for the other."""
    return (2 if Cout == 32 else 1) if _packed_supported(K, Cin, Cout) else 0


@contextlib.contextmanager
def recording(ops, calls):
    """Within the context the encoder's `ops` calls are appended to `calls` instead of launched."""
    real = {name: getattr(ops, name) for name in (*STANDINS, "spconv_packed_supported", "spconv_plan_kind")}
    serial = _Serials()

    def standin(name):
        sig = inspect.signature(real[name])

        def fn(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append(dict(op=name, args={p: _describe(v, serial) for p, v in bound.arguments.items()}))
            return STANDINS[name](*a, **k)
        fn.__name__ = name
        return fn
    try:
        for name in STANDINS:
            setattr(ops, name, standin(name))
        ops.spconv_packed_supported, ops.spconv_plan_kind = _packed_supported, _plan_kind
        yield serial
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)


def encoder(config):
    """The sparse encoder of `config` as workloads builds it."""
    from srfdet3d_amd import workloads
    from srfdet3d_amd.compat.registry import build_middle_encoder
    return build_middle_encoder(workloads.model_cfg(config)["pts_middle_encoder"])


def strided_keys(enc):
    from srfdet3d_amd.sparse import _SparseConv
    return [m.indice_key for m in enc.modules() if isinstance(m, _SparseConv) and not m.subm]


def static_caps(enc, rows):
    """{indice_key: the eager size of its level + HEADROOM, "__rows__": a device count}."""
    caps = {}
    for key in strided_keys(enc):
        rows = live_rows(rows)
        caps[key] = rows + HEADROOM
    return dict(caps, __rows__=_i32(1))


def sorted_input(enc, rows, batch, caps=None):
    """The encoder's input on a bitmap level, as `SparseEncoderCustom.forward` makes it on the GPU."""
    from srfdet3d_amd.sparse import SparseConvTensor
    return SparseConvTensor.sorted_by_bitmap(torch.zeros(rows, enc.in_channels), _i32(rows, 4), enc.sparse_shape, batch, caps)


def run(enc, route, rows, serial, calls):
    """One forward of `enc` on `rows` voxels.  CPU coordinates take the hash route in `forward`, so the eager bitmap route is entered
    the way `forward` enters it on the GPU; the static route goes through `forward`, where CPU tensors keep it on one stream."""
    if route == "hash":
        enc.spatial_sort = False
        enc(torch.zeros(rows, enc.in_channels), _i32(rows, 4), 2)
    elif route == "bitmap":
        enc._layers(sorted_input(enc, rows, 2)).dense_bev()
    else:
        _, counts = enc(torch.zeros(rows, enc.in_channels), _i32(rows, 4), 1, static_caps=static_caps(enc, rows))
        calls.append(dict(op="-- counts --", args=[[k, _describe(n, serial), cap] for k, n, cap in counts]))


def record(ops, cases=CASES):
    """{case: [call records]} of the sparse encoder over the `ops` module it uses."""
    out = {}
    for name in cases:
        config, route, rows, *train = name.split("/")
        torch.manual_seed(0)
        enc = encoder(config).train(bool(train)).requires_grad_(bool(train))
        calls = []
        with recording(ops, calls) as serial, torch.set_grad_enabled(bool(train)):
            run(enc, route, int(rows), serial, calls)
        out[name] = calls
    return out


def index_calls(calls):
    """The index calls of a case with their storages renumbered in order of first appearance among them."""
    seen = {}

    def renumber(v):
        if isinstance(v, dict):
            return {k: (seen.setdefault(e, len(seen)) if k in ("storage", "bitmap", "table") else renumber(e)) for k, e in v.items()}
        return [renumber(e) for e in v] if isinstance(v, list) else v
    return [renumber(c) for c in calls if c["op"] not in NOT_INDEX]


def brief(call):
    """A call as the fixture holds it: the op and a digest of its full record."""
    return f"{call['op']} " + hashlib.sha256(json.dumps(call, sort_keys=True).encode()).hexdigest()[:10]


def dump(rec, f, line=brief):
    """One call per line."""
    f.write("{\n")
    for i, (name, calls) in enumerate(sorted(rec.items())):
        f.write(f" {json.dumps(name)}: [\n")
        f.write(",\n".join("  " + json.dumps(line(c), sort_keys=True) for c in calls))
        f.write("\n ]" + ("," if i + 1 < len(rec) else "") + "\n")
    f.write("}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="root of the checkout whose srfdet3d_amd/sparse.py is recorded")
    ap.add_argument("--full", metavar="FILE", help="also write the records in full, one call per line, to compare two trees call by call")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from srfdet3d_amd import ops, sparse
    assert os.path.abspath(sparse.__file__).startswith(os.path.abspath(a.tree) + os.sep), sparse.__file__
    rec = record(ops)
    with open(OUT, "w") as f:
        dump(rec, f)
    if a.full:
        with open(a.full, "w") as f:
            dump(rec, f, line=lambda c: c)
    print("wrote", OUT, "from", sparse.__file__, {k: len(v) for k, v in rec.items()})


if __name__ == "__main__":
    main()
