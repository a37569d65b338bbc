"""Return codes of the entry points of csrc/rulebook.hip -- coordinate tables, hash-route and bitmap-route rulebooks -- and their host
queries.  The library decides every refusal on the host before it enqueues anything, so it answers on a machine without a GPU.

Every pointer handed in is a made-up address that no kernel may ever see: each call below is the entry point's VALID call (which is never
made) with exactly one thing wrong, and `refusal` will not make a call with nothing wrong.  The geometry rows come from the case table
of tests/rulebook_ref.py: every (shape, geometry) pair that the definition calls invalid must be SRF_EINVAL at every entry point that takes a
geometry -- a window larger than the padded grid with a stride >= 2 included, where C's truncating division yields an extent of 1."""
import ctypes

import numpy as np
import pytest

import rulebook_ref as R
from srfdet3d_amd import _lib
from srfdet3d_amd._lib import hi

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
PTR = ctypes.c_void_p(0x10000)       # never dereferenced: not a device address
BIG = 1 << 30                        # a workspace size no check objects to
SHAPE, BATCH, A = [5, 7, 9], 3, 100
KS, ST, PD = [3, 3, 3], [2, 2, 2], [1, 1, 1]
GRID_2_32 = [2048, 2048, 1024]       # 2^32 cells
K_28, K_32 = [28, 1, 1], [4, 4, 2]

# entry point -> (argument names in ABI order without the stream, the valid call)
ENTRIES = {
    "srf_coord_table_build": ("indices A shape batch table capacity", dict(indices=PTR, A=A, shape=SHAPE, batch=BATCH, table=PTR, capacity=1024)),
    "srf_rulebook_subm": ("indices A shape ksize table capacity nbr pair_counts",
                          dict(indices=PTR, A=A, shape=SHAPE, ksize=KS, table=PTR, capacity=1024, nbr=PTR, pair_counts=PTR)),
    "srf_rulebook_strided_outputs": ("indices A shape batch ksize stride pad out_indices num_out out_table out_capacity workspace workspace_bytes",
                                     dict(indices=PTR, A=A, shape=SHAPE, batch=BATCH, ksize=KS, stride=ST, pad=PD, out_indices=PTR, num_out=PTR,
                                          out_table=PTR, out_capacity=1024, workspace=PTR, workspace_bytes=BIG)),
    "srf_rulebook_strided_pairs": ("A ksize out_table out_capacity workspace num_out_host nbr pair_counts",
                                   dict(A=A, ksize=KS, out_table=PTR, out_capacity=1024, workspace=PTR, num_out_host=50, nbr=PTR, pair_counts=PTR)),
    "srf_bitmap_build": ("indices A shape batch bitmap prefix order sorted_indices workspace workspace_bytes",
                         dict(indices=PTR, A=A, shape=SHAPE, batch=BATCH, bitmap=PTR, prefix=PTR, order=PTR, sorted_indices=PTR, workspace=PTR,
                              workspace_bytes=BIG)),
    "srf_bitmap_rulebook_subm": ("sorted_indices A shape batch ksize bitmap prefix nbr pair_counts",
                                 dict(sorted_indices=PTR, A=A, shape=SHAPE, batch=BATCH, ksize=KS, bitmap=PTR, prefix=PTR, nbr=PTR, pair_counts=PTR)),
    "srf_bitmap_strided_outputs": ("indices A shape batch ksize stride pad out_bitmap out_prefix out_indices out_capacity num_out workspace workspace_bytes",
                                   dict(indices=PTR, A=A, shape=SHAPE, batch=BATCH, ksize=KS, stride=ST, pad=PD, out_bitmap=PTR, out_prefix=PTR,
                                        out_indices=PTR, out_capacity=200, num_out=PTR, workspace=PTR, workspace_bytes=BIG)),
    "srf_bitmap_strided_pairs": ("out_indices num_out max_out shape batch ksize stride pad in_bitmap in_prefix in_rows nbr nbr_stride fill_tail pair_counts",
                                 dict(out_indices=PTR, num_out=PTR, max_out=200, shape=SHAPE, batch=BATCH, ksize=KS, stride=ST, pad=PD, in_bitmap=PTR,
                                      in_prefix=PTR, in_rows=A, nbr=PTR, nbr_stride=200, fill_tail=1, pair_counts=PTR)),
}
ENTRIES["srf_bitmap_build_padded"] = ENTRIES["srf_bitmap_build"]
ENTRIES["srf_bitmap_strided_outputs_static"] = ENTRIES["srf_bitmap_strided_outputs"]
HOST_ARRAYS = ("shape", "ksize", "stride", "pad")
STRIDED = ("srf_rulebook_strided_outputs", "srf_bitmap_strided_outputs", "srf_bitmap_strided_outputs_static", "srf_bitmap_strided_pairs")


def refusal(entry, **wrong):
    """the code of the valid call of `entry` with `wrong` put in its place"""
    names, valid = ENTRIES[entry]
    kw = dict(valid, **wrong)
    assert set(kw) == set(valid) and any(v is None or v != valid[k] for k, v in wrong.items()), (entry, wrong)
    args = [hi(kw[n]) if n in HOST_ARRAYS and kw[n] is not None else kw[n] for n in names.split()]
    return getattr(_lib.lib(), entry)(*args, None)


def rows(entry):
    """(what is wrong, code) for `entry`: the rows every entry point with that argument shares, then its own"""
    names, valid = ENTRIES[entry]
    names = names.split()
    out = []
    # null pointers: everything but an optional output
    optional = {"srf_bitmap_build": ("order", "sorted_indices"), "srf_bitmap_build_padded": ("order", "sorted_indices"),
                "srf_bitmap_rulebook_subm": ("pair_counts",), "srf_bitmap_strided_pairs": ("pair_counts",)}.get(entry, ())
    out += [({n: None}, EINVAL) for n in names if (valid[n] is PTR or n in HOST_ARRAYS) and n not in optional]
    out += [({n: -1}, EINVAL) for n in ("A", "num_out_host", "max_out", "in_rows") if n in names]
    if "shape" in names:
        out += [(dict(shape=s), EINVAL) for s in ([0, 7, 9], [5, -1, 9], [5, 7, 0], GRID_2_32)]
    if "batch" in names and "bitmap" in " ".join(names) and entry != "srf_bitmap_rulebook_subm" and entry != "srf_bitmap_strided_pairs":
        out += [(dict(batch=0), EINVAL), (dict(batch=-2), EINVAL)]
    if "ksize" in names:
        out += [(dict(ksize=k), EINVAL) for k in (K_28, K_32, [0, 3, 3], [3, -3, -3], [1 << 16, 1 << 16, 1])]
    if "stride" in names:
        out += [(dict(stride=[2, 0, 2]), EINVAL), (dict(stride=[-1, 2, 2]), EINVAL), (dict(pad=[1, -1, 1]), EINVAL)]
    for n in ("capacity", "out_capacity"):
        if n in names and valid[n] == 1024:                          # a hash table: a power of two, >= 1024, >= 2 * rows
            out += [({n: c}, EINVAL) for c in (0, -1024, 512, 1000, 1025, 3 << 10)]
    if entry in ("srf_coord_table_build", "srf_rulebook_subm"):
        out += [(dict(A=513), EINVAL), (dict(A=1025, capacity=2048), EINVAL)]
    if entry == "srf_rulebook_strided_outputs":
        # bound = min(1000 * 8, 20 * 32 * 32) = 8000 outputs want a table of 16384
        out += [(dict(shape=[40, 64, 64], batch=1, A=1000, out_capacity=8192), EINVAL)]
        need = _lib.lib().srf_rulebook_strided_workspace_bytes(A, hi(KS), 1024)
        assert need > 0
        out += [(dict(workspace_bytes=need - 1), EWORKSPACE), (dict(workspace_bytes=0), EWORKSPACE)]
    if entry.startswith("srf_bitmap_build") or entry.startswith("srf_bitmap_strided_outputs"):
        out += [(dict(workspace_bytes=_lib.lib().srf_bitmap_workspace_bytes(1) - 1), EWORKSPACE), (dict(workspace_bytes=0), EWORKSPACE)]
    if entry.startswith("srf_bitmap_strided_outputs"):
        out += [(dict(out_capacity=-1), EINVAL)]
    if entry == "srf_bitmap_rulebook_subm":
        out += [(dict(ksize=k), EUNSUPPORTED) for k in ([2, 2, 2], [3, 3, 2], [2, 1, 1], [1, 4, 1])]
    if entry == "srf_bitmap_strided_pairs":
        out += [(dict(nbr_stride=199), EINVAL), (dict(nbr_stride=0), EINVAL)]
    return out


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals(entry):
    table = rows(entry)
    assert len(table) >= 8
    for wrong, code in table:
        assert refusal(entry, **wrong) == code, (entry, wrong)


INVALID = [(shape, g) for shape, _ in R.SHAPES for g in R.GEOMS if not R.valid_geometry(shape, *g)]
VALID = [(shape, batch, g) for shape, batch in R.SHAPES for g in R.GEOMS if R.valid_geometry(shape, *g)]


def test_every_invalid_pair_of_the_table_is_einval():
    L = _lib.lib()
    assert len(INVALID) == len(R.SHAPES) * len(R.GEOMS) - len(VALID) >= 5
    truncating = [(s, g) for s, g in INVALID if any(s[d] + 2 * g[2][d] < g[0][d] and g[1][d] >= 2 for d in range(3))]
    assert truncating                                                # ... where (-1) / 2 + 1 = 1 in C
    for shape, (ks, st, pd) in INVALID:
        assert L.srf_strided_max_outputs(A, 2, hi(shape), hi(ks), hi(st), hi(pd)) == EINVAL, (shape, ks, st, pd)
        for entry in STRIDED:
            assert refusal(entry, shape=shape, ksize=ks, stride=st, pad=pd) == EINVAL, (entry, shape, ks, st, pd)
    # the geometry the defect was first seen at, and its neighbours on either side of the rule
    assert L.srf_strided_max_outputs(A, 1, hi([2, 8, 8]), hi([3, 3, 3]), hi([2, 2, 2]), hi([0, 1, 1])) == EINVAL
    assert L.srf_strided_max_outputs(A, 1, hi([2, 8, 8]), hi([3, 3, 3]), hi([1, 1, 1]), hi([0, 1, 1])) == EINVAL
    assert L.srf_strided_max_outputs(A, 1, hi([3, 8, 8]), hi([3, 3, 3]), hi([2, 2, 2]), hi([0, 1, 1])) == min(A * 8, 1 * 4 * 4)
    assert L.srf_strided_max_outputs(A, 1, hi([1, 8, 8]), hi([3, 3, 3]), hi([2, 2, 2]), hi([1, 1, 1])) == min(A * 8, 1 * 4 * 4)


def test_strided_max_outputs_codes_and_value():
    L = _lib.lib()
    for kw in (dict(A=-1), dict(shape=None), dict(ksize=None), dict(ksize=K_28), dict(ksize=K_32), dict(stride=[2, 0, 2]), dict(pad=[0, -1, 0]),
               dict(shape=GRID_2_32), dict(shape=[0, 7, 9])):
        a = dict(dict(A=A, batch=BATCH, shape=SHAPE, ksize=KS, stride=ST, pad=PD), **kw)
        h = lambda v: hi(v) if v is not None else None
        assert L.srf_strided_max_outputs(a["A"], a["batch"], h(a["shape"]), h(a["ksize"]), h(a["stride"]), h(a["pad"])) == EINVAL, kw
    for shape, batch, (ks, st, pd) in VALID:
        per = int(np.prod([-(-ks[d] // st[d]) for d in range(3)]))
        vol = batch * int(np.prod(R.out_shape(shape, ks, st, pd)))
        for rows_ in (0, 1, 7, vol // per, vol // per + 1, 5000):
            assert L.srf_strided_max_outputs(rows_, batch, hi(shape), hi(ks), hi(st), hi(pd)) == min(rows_ * per, vol), (shape, batch, ks, st, pd, rows_)
    assert 13 * 41 * 1472 * 1472 < (1 << 32) - 1                     # a legal grid whose bound does not fit the 2^30 rows of a table
    assert L.srf_strided_max_outputs(1 << 30, 13, hi([41, 1472, 1472]), hi(KS), hi([1, 1, 1]), hi(PD)) == EINVAL


def test_bitmap_words_and_table_capacity():
    L = _lib.lib()
    for shape, batch in R.SHAPES + [([4, 256, 256], 1), ([4, 256, 257], 1), ([8, 64, 67], 2), ([41, 1472, 1472], 2)]:
        assert L.srf_bitmap_words(hi(shape), batch) == -(-batch * int(np.prod(shape)) // 32), (shape, batch)
    assert L.srf_bitmap_words(hi([4, 256, 256]), 1) == 8192 and L.srf_bitmap_words(hi([4, 256, 257]), 1) == 8224
    for shape, batch in ((GRID_2_32, 1), ([2048, 2048, 512], 2), ([0, 4, 4], 1), ([4, 4, 4], 0)):
        assert L.srf_bitmap_words(hi(shape), batch) == 0, (shape, batch)
    assert L.srf_bitmap_words(None, 1) == 0
    for n in (0, 1, 303, 511, 512, 513, 1023, 1024, 1025, 4096, 4097, 20000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 28, 1 << 29):
        want = 1024
        while want < 2 * n:
            want *= 2
        assert L.srf_coord_table_capacity(n) == want, n
        assert L.srf_coord_table_bytes(want) == 8 * want
