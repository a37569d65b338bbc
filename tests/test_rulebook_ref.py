"""tests/rulebook_ref.py (the definition of the sparse index tables, numpy) against the C oracle over the whole case table, the two
output orders against each other, the bitmap against its decoding -- and the table against itself: it must hold the cases that tell a
right kernel from a wrong one, so each of seven wrong definitions has to differ from the right one at a case that is named.  CPU only."""
import numpy as np
import pytest

import rulebook_ref as R
from oracle import oracle as O

CASES = list(R.cases())
BY_SHAPE = [[c for c in CASES if c[1] == shape] for shape, _ in R.SHAPES]
IDS = ["x".join(map(str, shape)) + f"b{batch}" for shape, batch in R.SHAPES]


def valid_geoms(shape):
    return [g for g in R.GEOMS if R.valid_geometry(shape, *g)]


def test_the_table_is_the_one_the_oracle_was_checked_on():
    assert sum(len(valid_geoms(shape)) for _, shape, *_ in CASES) == 261
    assert sum(s[0] * s[1] * s[2] % 32 != 0 for s, _ in R.SHAPES) == len(R.SHAPES) - 1
    assert {1, 2, 31, 32, 33, 41} <= {s[0] for s, _ in R.SHAPES} and any(s[1] == 1 for s, _ in R.SHAPES)


@pytest.mark.parametrize("group", BY_SHAPE, ids=IDS)
def test_oracle_equals_the_definition(group):
    for name, shape, batch, density, idx in group:
        for ks in R.SUBM_KSIZES + R.SUBM_KSIZES_HASH_ONLY:
            nbr, cnt = O.rulebook_subm(idx, shape, ks)
            want_nbr, want_cnt = R.subm(idx, shape, ks)
            assert np.array_equal(nbr, want_nbr) and np.array_equal(cnt, want_cnt), (name, ks)
        for ks, st, pd in valid_geoms(shape):
            oi, nbr, cnt, osh = O.rulebook_strided(idx, shape, ks, st, pd)
            w_oi, w_nbr, w_cnt = R.strided_first_seen(idx, shape, ks, st, pd)
            assert osh == R.out_shape(shape, ks, st, pd), (name, ks, st, pd)
            assert np.array_equal(oi, w_oi) and np.array_equal(nbr, w_nbr) and np.array_equal(cnt, w_cnt), (name, ks, st, pd)
            assert len(oi) >= 1, (name, ks, st, pd)                                # every valid case has an output row
            assert len(oi) <= min(len(idx) * int(np.prod([-(-ks[d] // st[d]) for d in range(3)])), batch * int(np.prod(osh)))
            if density == 0.3:                                                     # ... and says something in both directions
                # (K = 1 cannot: an output exists because its ONE offset has an input, so its nbr holds no -1 on any grid)
                assert (nbr >= 0).any() and ((nbr < 0).any() or int(np.prod(ks)) == 1), (name, ks, st, pd)
                assert not (int(np.prod(ks)) == 1 and (nbr < 0).any())
        if density == 0.3:
            for ks in R.SUBM_KSIZES:
                nbr = R.subm(idx, shape, ks)[0]
                assert (nbr >= 0).any() and ((nbr < 0).any() or ks == [1, 1, 1]), (name, ks)


@pytest.mark.parametrize("group", BY_SHAPE, ids=IDS)
def test_sorted_form_is_the_first_seen_form_under_the_stable_sort(group):
    for name, shape, batch, density, idx in group:
        for ks, st, pd in valid_geoms(shape):
            f_oi, f_nbr, f_cnt = R.strided_first_seen(idx, shape, ks, st, pd)
            s_oi, s_nbr, s_cnt = R.strided_sorted(idx, shape, ks, st, pd)
            perm = R.sort_order(f_oi, R.out_shape(shape, ks, st, pd))
            assert np.array_equal(s_oi, f_oi[perm]) and np.array_equal(s_nbr, f_nbr[:, perm]) and np.array_equal(s_cnt, f_cnt), (name, ks, st, pd)
            assert (np.diff(R.cells(s_oi, R.out_shape(shape, ks, st, pd))) > 0).all()


def test_bitmap_and_decode_round_trip_every_active_set():
    for name, shape, batch, density, idx in CASES:
        words, prefix = R.bitmap(idx, shape, batch)
        assert words.dtype == np.uint32 and len(words) == -(-batch * int(np.prod(shape)) // 32) == len(prefix)
        order = R.sort_order(idx, shape)
        live = R.set_cells(words)
        assert np.array_equal(R.decode(live, shape), idx[order]), name
        assert np.array_equal(live, R.cells(idx[order], shape))
        rank = prefix[live >> 5] + np.array([bin(int(words[c >> 5]) & ((1 << (c & 31)) - 1)).count("1") for c in live], np.int64)
        assert np.array_equal(rank, np.arange(len(idx))), name                     # the prefix ranks every site at its sorted row


def test_every_rejection_clause_fires_and_a_word_straddles_two_samples():
    fired = np.zeros(3, np.int64)
    for name, shape, batch, density, idx in CASES:
        for g in valid_geoms(shape):
            fired += np.array(R.candidates(idx, shape, *g)[3])
    assert (fired > 0).all(), dict(zip(("t < 0", "t % stride != 0", "q >= out_shape"), fired))
    straddling = []
    for name, shape, batch, density, idx in CASES:
        per = int(np.prod(shape))
        words, _ = R.bitmap(idx, shape, batch)
        for b in range(1, batch):
            w, bit = divmod(b * per, 32)
            if bit and int(words[w]) & ((1 << bit) - 1) and int(words[w]) >> bit:
                straddling.append((name, b, w))
    assert straddling
    # on the output side too: a strided level whose words straddle samples, with bits on both sides (what srf_bm_emit_k walks)
    out_side = 0
    for name, shape, batch, density, idx in CASES:
        for g in valid_geoms(shape):
            osh = R.out_shape(shape, *g)
            oi = R.strided_sorted(idx, shape, *g)[0]
            words, _ = R.bitmap(oi, osh, batch)
            w, bit = divmod(int(np.prod(osh)), 32)
            out_side += bool(bit and int(words[w]) & ((1 << bit) - 1) and int(words[w]) >> bit)
    assert out_side > 20


def test_overflow_prediction_is_the_definition_on_the_first_rows():
    """a level of which only the first `cap` sorted rows exist: its own tables are the head of the full ones, and what a consumer reads
    through the full bitmap with ranks >= cap as -1 is what the definition gives on the truncated set"""
    for name, shape, batch, density, idx in CASES:
        if density != 0.3:
            continue
        idx = idx[R.sort_order(idx, shape)]
        clipped = 0
        for g in R.overflow_geoms(shape):
            osh = R.out_shape(shape, *g)
            ref = R.strided_sorted(idx, shape, *g)
            n = len(ref[0])
            assert n >= 4, (name, g)
            full = R.subm(ref[0], osh, [3, 3, 3])[0]
            g2 = g if R.valid_geometry(osh, *g) else R.GEOMS[0]
            full2 = R.strided_sorted(ref[0], osh, *g2)
            for cap in (n - 1, n // 2):
                oi, nbr = R.overflowed(ref, cap, len(idx))
                assert len(oi) == cap and nbr.shape[1] == cap and np.array_equal(nbr, ref[1][:, :cap])
                assert np.array_equal(R.clip_rows(full[:, :cap], cap), R.subm(oi, osh, [3, 3, 3])[0]), (name, g, cap)
                clipped += int((full[:, :cap] >= cap).any())
                # a strided step from the head: its outputs are among the full step's, and their columns are the full ones clipped
                head2 = R.strided_sorted(oi, osh, *g2)
                pos = np.searchsorted(R.cells(full2[0], R.out_shape(osh, *g2)), R.cells(head2[0], R.out_shape(osh, *g2)))
                assert np.array_equal(full2[0][pos], head2[0]) and np.array_equal(R.clip_rows(full2[1][:, pos], cap), head2[1]), (name, g, g2, cap)
        assert clipped >= 2, name                                    # the capacity tests show something at this shape
        assert np.array_equal(R.overflowed(ref, n, 3)[1], np.where(ref[1] >= 3, -1, ref[1]))


# ---------------------------------------------------------------------------------------------------------------- sensitivity
class SortedByBZYX(R.Rules):
    @staticmethod
    def sort_key(b, z, y, x, shape):
        return ((b * shape[0] + z) * shape[1] + y) * shape[2] + x


class NoDivisibilityOffPowersOfTwo(R.Rules):
    @staticmethod
    def divisible(t, stride):
        return np.where(stride & (stride - 1), True, t % stride == 0)


class NoUpperBound(R.Rules):
    @staticmethod
    def inside(q, oshape):
        return np.ones(np.broadcast(q, oshape).shape, bool)


class CentreOne(R.Rules):
    @staticmethod
    def centre(ks):
        return 1


class NoBatchInKey(R.Rules):
    @staticmethod
    def lookup_key(b, z, y, x, shape):
        return (z * shape[1] + y) * shape[2] + x


class SamplesInWholeWords(R.Rules):
    @staticmethod
    def sample_cells(shape):
        return -(-shape[0] * shape[1] * shape[2] // 32) * 32


class TruncatingDivision(R.Rules):
    """C's division, and the window rule left to the extent it gives: (-1) / 2 + 1 = 1 passes for an output that does not exist"""
    @staticmethod
    def div(a, b):
        return int(a / b)

    @staticmethod
    def fits(padded, ks):
        return True


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _detect(wrong):
    """the first case of the table at which the wrong rules give another answer than the right ones, as text; None if there is none"""
    for name, shape, batch, density, idx in CASES:
        for g in R.GEOMS:
            if R.valid_geometry(shape, *g) != R.valid_geometry(shape, *g, rules=wrong):
                return f"{name} {g}: valid_geometry"
            if not R.valid_geometry(shape, *g):
                continue
            if not _same(R.strided_first_seen(idx, shape, *g), R.strided_first_seen(idx, shape, *g, rules=wrong)):
                return f"{name} {g}: strided_first_seen"
            if not _same(R.strided_sorted(idx, shape, *g), R.strided_sorted(idx, shape, *g, rules=wrong)):
                return f"{name} {g}: strided_sorted"
        for ks in R.SUBM_KSIZES + R.SUBM_KSIZES_HASH_ONLY:
            if not _same(R.subm(idx, shape, ks), R.subm(idx, shape, ks, rules=wrong)):
                return f"{name} {ks}: subm"
        if not np.array_equal(R.sort_order(idx, shape), R.sort_order(idx, shape, rules=wrong)):
            return f"{name}: sort_order"
        live = R.set_cells(R.bitmap(idx, shape, batch)[0])
        if not np.array_equal(R.decode(live, shape), R.decode(live, shape, rules=wrong)):
            return f"{name}: decode"
    return None


@pytest.mark.parametrize("wrong", [SortedByBZYX, NoDivisibilityOffPowersOfTwo, NoUpperBound, CentreOne, NoBatchInKey, SamplesInWholeWords,
                                   TruncatingDivision], ids=lambda c: c.__name__)
def test_the_table_tells_each_wrong_definition_from_the_right_one(wrong):
    case = _detect(wrong())
    print(f"{wrong.__name__}: detected at {case}")
    assert case is not None
    if wrong is TruncatingDivision:
        assert case.endswith("valid_geometry")
