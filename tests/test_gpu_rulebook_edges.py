"""The producers of the sparse index tables (csrc/rulebook.hip: coordinate hash tables, occupancy bitmaps with their popcount prefixes,
sorted active sets, nbr[K][A_out] rulebooks) against the C oracle, exactly, on the case table of tests/rulebook_ref.py -- grids whose
samples end inside a bitmap word, geometries no encoder uses -- and at the seams of the implementation: 8192 elements of the device scan,
a hash table at half load, more workgroups than pair-count replicas, an output capacity at and below the count.

The oracle numbers strided outputs in first-seen order (the hash route); the bitmap route's answer is that result under the stable sort by
cell, which tests/test_rulebook_ref.py proves equal to the output-stationary definition.  No test here hands the library a coordinate
outside its grid or a duplicate row: both break the ABI's preconditions."""
import numpy as np
import pytest
import torch

import rulebook_ref as R
from oracle import oracle as O
from srfdet3d_amd import _lib, ops
from srfdet3d_amd._lib import hi

pytestmark = pytest.mark.gpu

CASES = {name: (shape, batch, density, idx) for name, shape, batch, density, idx in R.cases()}
BY_SHAPE = [[n for n, c in CASES.items() if c[0] == shape] for shape, _ in R.SHAPES]
IDS = ["x".join(map(str, shape)) + f"b{batch}" for shape, batch in R.SHAPES]
EUNSUPPORTED = -3
S333, G_S2 = [3, 3, 3], ([3, 3, 3], [2, 2, 2], [1, 1, 1])
GUARD, SENT = 64, 0x5A5A5A5A                                         # guard words behind a buffer, and what they (and garbage) hold


def valid_geoms(shape):
    return [g for g in R.GEOMS if R.valid_geometry(shape, *g)]


def _key(*a):
    return tuple(tuple(x) if isinstance(x, list) else x for x in a)


_memo = {}


def strided_ref(idx, shape, geom, tag):
    """oracle, first-seen: out_indices, nbr, counts, out_shape; computed once per (tag, geometry) -- `tag` names the active set"""
    k = ("strided", tag, _key(*geom))
    if k not in _memo:
        _memo[k] = O.rulebook_strided(idx, shape, *geom)
    return _memo[k]


def sorted_ref(idx, shape, geom, tag):
    """the same under the stable sort by cell: what the bitmap route emits"""
    k = ("sorted", tag, _key(*geom))
    if k not in _memo:
        oi, nbr, cnt, osh = strided_ref(idx, shape, geom, tag)
        perm = R.sort_order(oi, osh)
        _memo[k] = (oi[perm], nbr[:, perm], cnt, osh)
    return _memo[k]


def subm_ref(idx, shape, ks, tag):
    k = ("subm", tag, _key(ks))
    if k not in _memo:
        _memo[k] = O.rulebook_subm(idx, shape, ks)
    return _memo[k]


def np_(t):
    return t.cpu().numpy()


def same(got, want, what):
    got = np_(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), what


def level_is(lvl, idx, shape, batch, what):
    words, prefix = R.bitmap(idx, shape, batch)
    same(np_(lvl.bitmap).view(np.uint32), words, (what, "bitmap"))
    same(lvl.prefix, prefix, (what, "prefix"))


def second_geom(oshape, geom):
    return geom if R.valid_geometry(oshape, *geom) else G_S2         # 3x3x3 / 2 / 1 fits every grid


# ------------------------------------------------------------------------------------------------------------------ hash route
@pytest.mark.parametrize("names", BY_SHAPE, ids=IDS)
def test_hash_route(dev, names):
    for name in names:
        shape, batch, density, idx = CASES[name]
        t_idx = torch.from_numpy(idx).to(dev)
        table = ops.coord_table_build(t_idx, shape, batch)
        for ks in R.SUBM_KSIZES + R.SUBM_KSIZES_HASH_ONLY:
            nbr, cnt = ops.rulebook_subm(t_idx, shape, ks, table)
            w_nbr, w_cnt = subm_ref(idx, shape, ks, name)
            same(nbr, w_nbr, (name, ks, "subm nbr"))
            same(cnt, w_cnt, (name, ks, "subm counts"))
        for geom in valid_geoms(shape):
            oi, nbr, cnt, otable, osh = ops.rulebook_strided(t_idx, shape, batch, *geom)
            w_oi, w_nbr, w_cnt, w_osh = strided_ref(idx, shape, geom, name)
            assert osh == w_osh == R.out_shape(shape, *geom), (name, geom)
            same(oi, w_oi, (name, geom, "out_indices"))
            same(nbr, w_nbr, (name, geom, "nbr"))
            same(cnt, w_cnt, (name, geom, "pair_counts"))
            # the table the strided step returns serves the produced level
            s_nbr, s_cnt = ops.rulebook_subm(oi, osh, S333, otable)
            w_s_nbr, w_s_cnt = subm_ref(w_oi, osh, S333, (name, _key(*geom), "first-seen"))
            same(s_nbr, w_s_nbr, (name, geom, "subm on the produced level"))
            same(s_cnt, w_s_cnt, (name, geom, "subm counts on the produced level"))


# ---------------------------------------------------------------------------------------------------------------- bitmap route
@pytest.mark.parametrize("names", BY_SHAPE, ids=IDS)
def test_bitmap_route(dev, names):
    for name in names:
        shape, batch, density, idx = CASES[name]
        order = R.sort_order(idx, shape)
        sidx = idx[order]
        lvl, g_order, g_sidx = ops.bitmap_build(torch.from_numpy(idx).to(dev), shape, batch)
        same(g_order, order, (name, "order"))
        same(g_sidx, sidx, (name, "sorted indices"))
        level_is(lvl, idx, shape, batch, name)
        tag = (name, "sorted")
        for ks in R.SUBM_KSIZES:
            nbr, cnt = ops.rulebook_subm_bitmap(g_sidx, lvl, ks)
            w_nbr, w_cnt = subm_ref(sidx, shape, ks, tag)
            same(nbr, w_nbr, (name, ks, "subm nbr"))
            same(cnt, w_cnt, (name, ks, "subm counts"))
        for ks in R.SUBM_KSIZES_HASH_ONLY:
            rc = _lib.lib().srf_bitmap_rulebook_subm(ops._ptr(g_sidx), len(sidx), hi(shape), batch, hi(ks), ops._ptr(lvl.bitmap), ops._ptr(lvl.prefix),
                                                     ops._ptr(g_order), None, ops._stream())   # refused on the host: g_order is not written
            assert rc == EUNSUPPORTED, (name, ks)
        for geom in valid_geoms(shape):
            oi, nbr, cnt, olvl, osh = ops.rulebook_strided_bitmap(g_sidx, lvl, *geom)
            w_oi, w_nbr, w_cnt, w_osh = sorted_ref(sidx, shape, geom, tag)
            assert osh == w_osh, (name, geom)
            same(oi, w_oi, (name, geom, "out_indices"))
            same(nbr, w_nbr, (name, geom, "nbr"))
            same(cnt, w_cnt, (name, geom, "pair_counts"))
            level_is(olvl, w_oi, osh, batch, (name, geom, "output level"))
            # a two-level chain on odd extents: SubM on the output level, then a strided step from it
            tag2 = (name, _key(*geom), "sorted")
            s_nbr, s_cnt = ops.rulebook_subm_bitmap(oi, olvl, S333)
            same(s_nbr, subm_ref(w_oi, osh, S333, tag2)[0], (name, geom, "subm on the output level"))
            same(s_cnt, subm_ref(w_oi, osh, S333, tag2)[1], (name, geom, "subm counts on the output level"))
            g2 = second_geom(osh, geom)
            oi2, nbr2, cnt2, olvl2, osh2 = ops.rulebook_strided_bitmap(oi, olvl, *g2)
            w2_oi, w2_nbr, w2_cnt, w2_osh = sorted_ref(w_oi, osh, g2, tag2)
            assert osh2 == w2_osh, (name, geom, g2)
            same(oi2, w2_oi, (name, geom, g2, "second step out_indices"))
            same(nbr2, w2_nbr, (name, geom, g2, "second step nbr"))
            same(cnt2, w2_cnt, (name, geom, g2, "second step pair_counts"))
            level_is(olvl2, w2_oi, osh2, batch, (name, geom, g2, "second output level"))


# ----------------------------------------------------------------------------------------------------------------------- seams
def both_routes(dev, idx, shape, batch, tag, geoms=(G_S2,), subm=(S333,)):
    t_idx = torch.from_numpy(idx).to(dev)
    table = ops.coord_table_build(t_idx, shape, batch)
    assert table.capacity == _lib.lib().srf_coord_table_capacity(len(idx))
    for ks in subm:
        nbr, cnt = ops.rulebook_subm(t_idx, shape, ks, table)
        same(nbr, subm_ref(idx, shape, ks, tag)[0], (tag, ks, "hash subm"))
        same(cnt, subm_ref(idx, shape, ks, tag)[1], (tag, ks, "hash subm counts"))
    for geom in geoms:
        oi, nbr, cnt, otable, osh = ops.rulebook_strided(t_idx, shape, batch, *geom)
        w_oi, w_nbr, w_cnt, w_osh = strided_ref(idx, shape, geom, tag)
        same(oi, w_oi, (tag, geom, "hash out_indices"))
        same(nbr, w_nbr, (tag, geom, "hash nbr"))
        same(cnt, w_cnt, (tag, geom, "hash pair_counts"))
    order = R.sort_order(idx, shape)
    sidx = idx[order]
    lvl, g_order, g_sidx = ops.bitmap_build(t_idx, shape, batch)
    same(g_order, order, (tag, "order"))
    same(g_sidx, sidx, (tag, "sorted indices"))
    level_is(lvl, idx, shape, batch, tag)
    stag = (tag, "sorted")
    for ks in subm:
        nbr, cnt = ops.rulebook_subm_bitmap(g_sidx, lvl, ks)
        same(nbr, subm_ref(sidx, shape, ks, stag)[0], (tag, ks, "bitmap subm"))
        same(cnt, subm_ref(sidx, shape, ks, stag)[1], (tag, ks, "bitmap subm counts"))
    for geom in geoms:
        oi, nbr, cnt, olvl, osh = ops.rulebook_strided_bitmap(g_sidx, lvl, *geom)
        w_oi, w_nbr, w_cnt, w_osh = sorted_ref(sidx, shape, geom, stag)
        same(oi, w_oi, (tag, geom, "bitmap out_indices"))
        same(nbr, w_nbr, (tag, geom, "bitmap nbr"))
        same(cnt, w_cnt, (tag, geom, "bitmap pair_counts"))
        level_is(olvl, w_oi, osh, batch, (tag, geom, "output level"))


@pytest.mark.parametrize("shape,words", [([4, 256, 256], 8192), ([4, 256, 257], 8224)], ids=["8192w", "8224w"])
def test_scan_switch_at_8192_bitmap_words(dev, shape, words):
    """one 1024-thread workgroup up to 8192 elements, three launches above"""
    assert _lib.lib().srf_bitmap_words(hi(shape), 1) == words
    idx = R.active_set(shape, 1, 0.02, 7)
    # a stride-1 geometry as well: its OUTPUT bitmap has the same word count, so the scan that emits the rows sits at the seam too
    both_routes(dev, idx, shape, 1, ("seam", words), geoms=(G_S2, ([3, 3, 3], [1, 1, 1], [1, 1, 1])))


@pytest.mark.parametrize("A", [303, 304, 512, 513])
def test_hash_route_at_its_scan_switch_and_at_half_load(dev, A):
    """A * K = 8181 | 8208 candidates on either side of the scan switch; 512 | 513 rows: a table of 1024 slots half full, and the first of 2048"""
    shape, batch, _, idx = CASES["[41, 6, 5]x2@0.3"]
    assert len(idx) >= 513 and 303 * 27 <= 8192 < 304 * 27
    assert [_lib.lib().srf_coord_table_capacity(n) for n in (512, 513)] == [1024, 2048]
    both_routes(dev, np.ascontiguousarray(idx[:A]), shape, batch, ("truncated", A),
                geoms=(G_S2, ([3, 3, 3], [3, 3, 3], [1, 1, 1]), ([3, 3, 3], [1, 1, 1], [0, 0, 0])))


def test_pair_counts_through_the_replicas(dev):
    """~20 k rows: 80 workgroups per offset add into 32 replicated counters"""
    shape, batch = [8, 64, 67], 2
    idx = R.active_set(shape, batch, 0.3, 11)
    assert len(idx) > 32 * 256 * 2
    both_routes(dev, idx, shape, batch, "replicas", geoms=(G_S2, ([3, 3, 3], [2, 2, 2], [0, 1, 1])), subm=(S333, [1, 3, 3]))


# ------------------------------------------------------------------------------------------------------- static and padded forms
def garbage(n, dev):
    return torch.full((max(n, 1),), SENT, dtype=torch.int32, device=dev)


def padded_build(dev, rows, shape, batch):
    """srf_bitmap_build_padded through the C ABI into buffers full of garbage -> level, order, sorted_indices (all A slots)"""
    L = _lib.lib()
    A = len(rows)
    t = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
    lvl = ops.BitmapLevel(shape, batch, dev)
    lvl.bitmap.fill_(SENT)
    lvl.prefix.fill_(SENT)
    order, sidx = garbage(A + GUARD, dev), garbage(4 * A + GUARD, dev)
    ws, nbytes = lvl.workspace()
    _lib.check(L.srf_bitmap_build_padded(ops._ptr(t), A, hi(shape), batch, ops._ptr(lvl.bitmap), ops._ptr(lvl.prefix), ops._ptr(order), ops._ptr(sidx),
                                         ops._ptr(ws), nbytes, ops._stream()), "bitmap_build_padded")
    assert (np_(order[A:]) == SENT).all() and (np_(sidx[4 * A:]) == SENT).all()
    return lvl, np_(order[:A]), np_(sidx[:4 * A]).reshape(A, 4)


@pytest.mark.parametrize("names", BY_SHAPE[:4], ids=IDS[:4])
def test_padded_build_with_padding_between_the_live_rows(dev, names):
    rng = np.random.default_rng(5)
    for name in names:
        shape, batch, density, idx = CASES[name]
        n = len(idx)
        want_lvl, want_order, want_sidx = ops.bitmap_build(torch.from_numpy(idx).to(dev), shape, batch)
        same(want_sidx, idx[R.sort_order(idx, shape)], name)
        pad = n // 2 + 3
        for how in ("tail", "interleaved", "all padding"):
            rows = np.full((n + pad, 4), -1, np.int32)
            at = np.arange(n) if how == "tail" else np.sort(rng.choice(n + pad, n, replace=False))
            if how != "all padding":
                rows[at] = idx
            live = 0 if how == "all padding" else n
            lvl, order, sidx = padded_build(dev, rows, shape, batch)
            if live:
                assert torch.equal(lvl.bitmap, want_lvl.bitmap) and torch.equal(lvl.prefix, want_lvl.prefix), (name, how)
                same(order[:n], at[np_(want_order)], (name, how, "order"))
                same(sidx[:n], np_(want_sidx), (name, how, "sorted indices"))
            else:
                assert not lvl.bitmap.any() and not lvl.prefix.any(), (name, how)
            assert (order[live:] == 0).all() and (sidx[live:] == -1).all(), (name, how)


def static_step(dev, g_sidx, lvl, geom, cap):
    """srf_bitmap_strided_outputs_static + srf_bitmap_strided_pairs(fill_tail = 1) through the C ABI with `cap` rows, guard words behind
    out_indices and nbr -> out_indices (cap, 4), nbr (K, cap), counts (K,), the true count, the output level; asserts the guards"""
    L = _lib.lib()
    A, K = g_sidx.shape[0], int(np.prod(geom[0]))
    osh = ops.out_spatial_shape(lvl.shape, *geom)
    olvl = ops.BitmapLevel(osh, lvl.batch, dev)
    out_idx, nbr, num = garbage(4 * cap + GUARD, dev), garbage(K * cap + GUARD, dev), garbage(1, dev)
    counts = garbage(L.srf_bitmap_pair_count_ints(), dev)
    ws, nbytes = olvl.workspace()
    _lib.check(L.srf_bitmap_strided_outputs_static(ops._ptr(g_sidx), A, hi(lvl.shape), lvl.batch, hi(geom[0]), hi(geom[1]), hi(geom[2]),
                                                   ops._ptr(olvl.bitmap), ops._ptr(olvl.prefix), ops._ptr(out_idx), cap, ops._ptr(num), ops._ptr(ws),
                                                   nbytes, ops._stream()), "bitmap_strided_outputs_static")
    _lib.check(L.srf_bitmap_strided_pairs(ops._ptr(out_idx), ops._ptr(num), cap, hi(lvl.shape), lvl.batch, hi(geom[0]), hi(geom[1]), hi(geom[2]),
                                          ops._ptr(lvl.bitmap), ops._ptr(lvl.prefix), A, ops._ptr(nbr), cap, 1, ops._ptr(counts), ops._stream()),
               "bitmap_strided_pairs")
    assert (np_(out_idx[4 * cap:]) == SENT).all() and (np_(nbr[K * cap:]) == SENT).all(), "guard words"
    return out_idx[:4 * cap].view(cap, 4), nbr[:K * cap].view(K, cap), counts[:K], int(num.item()), olvl


@pytest.mark.parametrize("names", BY_SHAPE, ids=IDS)
def test_static_capacity_at_above_and_below_the_count(dev, names):
    """capacity == count and count + 1: every row written, tails -1.  count - 1 and count // 2: writes stay inside the capacity, *num_out is
    the true count, rows and columns [0, cap) are the head of the sorted answer, and the consumers of that level read ranks >= cap as -1"""
    name = names[1]                                                  # density 0.3
    shape, batch, density, idx = CASES[name]
    sidx = idx[R.sort_order(idx, shape)]
    tag = (name, "sorted")
    lvl, _, g_sidx = ops.bitmap_build(torch.from_numpy(idx).to(dev), shape, batch)
    for geom in R.overflow_geoms(shape):
        ref = sorted_ref(sidx, shape, geom, tag)
        w_oi, w_nbr, w_cnt, osh = ref
        n, K = len(w_oi), len(w_nbr)
        assert n >= 4, (name, geom)
        tag2 = (name, _key(*geom), "sorted")
        full_subm = subm_ref(w_oi, osh, S333, tag2)[0]
        for cap in (n, n + 1, n - 1, n // 2):
            oi, nbr, cnt, num, olvl = static_step(dev, g_sidx, lvl, geom, cap)
            assert num == n, (name, geom, cap)                       # never clamped
            level_is(olvl, w_oi, osh, batch, (name, geom, cap, "output level"))   # the level's bitmap is complete whatever the capacity
            m = min(cap, n)
            e_oi, e_nbr = R.overflowed(ref[:3], cap, len(sidx))
            same(oi[:m], e_oi, (name, geom, cap, "out_indices"))
            same(nbr[:, :m], e_nbr, (name, geom, cap, "nbr"))
            assert (np_(oi[m:]) == -1).all() and (np_(nbr[:, m:]) == -1).all(), (name, geom, cap, "tails")
            same(cnt, (e_nbr >= 0).sum(1), (name, geom, cap, "pair_counts"))
            if cap > n:
                continue
            # consumers of the level with A = cap: SubM, and a strided step with in_rows = cap
            head = oi[:cap].contiguous()
            s_nbr, s_cnt = ops.rulebook_subm_bitmap(head, olvl, S333)
            e_s = R.clip_rows(full_subm[:, :cap], cap)
            same(s_nbr, e_s, (name, geom, cap, "subm on the overflowed level"))
            same(s_cnt, (e_s >= 0).sum(1), (name, geom, cap, "subm counts on the overflowed level"))
            g2 = second_geom(osh, geom)
            oi2, nbr2, cnt2, olvl2, osh2 = ops.rulebook_strided_bitmap(head, olvl, *g2)
            # the input bitmap holds all n sites, the rows only cap of them: a rank >= cap reads as absent, which is the definition on the head
            w2_oi, w2_nbr, w2_cnt, _ = sorted_ref(w_oi[:cap], osh, g2, (tag2, cap))
            same(oi2, w2_oi, (name, geom, cap, g2, "strided step from the overflowed level"))
            same(nbr2, w2_nbr, (name, geom, cap, g2, "its nbr"))
            same(cnt2, w2_cnt, (name, geom, cap, g2, "its pair_counts"))


def test_empty_sets(dev):
    shape, batch = R.SHAPES[0]
    none = torch.zeros((0, 4), dtype=torch.int32, device=dev)
    table = ops.coord_table_build(none, shape, batch)
    assert table.capacity == 1024 and (np_(table.buf) == -1).all()
    for ks in R.SUBM_KSIZES + R.SUBM_KSIZES_HASH_ONLY:
        nbr, cnt = ops.rulebook_subm(none, shape, ks, table)
        assert nbr.shape == (int(np.prod(ks)), 0) and not cnt.any()
    lvl, order, sidx = ops.bitmap_build(none, shape, batch)
    assert order.shape == (0,) and sidx.shape == (0, 4) and not lvl.bitmap.any() and not lvl.prefix.any()
    plvl, porder, psidx = ops.bitmap_build(none, shape, batch, padded=True)
    assert porder.shape == (0,) and not plvl.bitmap.any() and not plvl.prefix.any()
    for ks in R.SUBM_KSIZES:
        nbr, cnt = ops.rulebook_subm_bitmap(sidx, lvl, ks)
        assert nbr.shape == (int(np.prod(ks)), 0) and not cnt.any()
    for geom in valid_geoms(shape):
        K = int(np.prod(geom[0]))
        oi, nbr, cnt, otable, osh = ops.rulebook_strided(none, shape, batch, *geom)
        assert oi.shape == (0, 4) and nbr.shape == (K, 0) and not cnt.any() and osh == R.out_shape(shape, *geom)
        assert (np_(otable.buf) == -1).all()
        oi, nbr, cnt, olvl, osh = ops.rulebook_strided_bitmap(sidx, lvl, *geom)
        assert oi.shape == (0, 4) and nbr.shape == (K, 0) and not cnt.any() and osh == R.out_shape(shape, *geom)
        assert not olvl.bitmap.any() and not olvl.prefix.any()
        s_oi, s_nbr, _, s_lvl, _, s_num = ops.rulebook_strided_bitmap(sidx, lvl, *geom, out_capacity=5)
        assert int(s_num.item()) == 0 and (np_(s_oi) == -1).all() and (np_(s_nbr) == -1).all() and not s_lvl.bitmap.any()
