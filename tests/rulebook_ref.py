"""The sparse index tables of csrc/rulebook.hip as their DEFINITION, in numpy and plain Python (no library, no torch), and the table
of cases that tests/test_rulebook_ref.py (CPU), tests/test_rulebook_args.py (return codes) and tests/test_gpu_rulebook_edges.py share.

Conventions (include/srfdet3d.h, K4 and the bitmap section): an active set is `indices` (A, 4) int32 rows (b, z, y, x), distinct, inside
the grid `shape` = [D, H, W].  A rulebook is nbr (K, A_out) int32, nbr[k][o] = the input row that output row o reads through kernel
offset k = (kz*KH + ky)*KW + kx, or -1; counts[k] = entries of nbr[k] that are >= 0.
  SubM     nbr[k][o] = row of (b, z + kz - ks0//2, y + ky - ks1//2, x + kx - ks2//2)
  strided  input p feeds output q through k  <=>  t = p + pad - k >= 0,  t % stride == 0,  q = t / stride < out_shape   (per dimension)
           hash route: outputs numbered in first-seen order over (input row, k) ascending; bitmap route: sorted by cell
  cell(b, z, y, x) = ((b*H + y)*W + x)*D + z;  bitmap word = cell >> 5, bit = cell & 31;  prefix[w] = set bits of the words before w

Every rule a kernel could get wrong is one method of `Rules`; a wrong definition (tests/test_rulebook_ref.py, sensitivity) overrides one
method, and every function here takes the rules it is to follow."""
import numpy as np

# (shape [D, H, W], batch): all but [32, 4, 4] have D*H*W % 32 != 0, so a bitmap word straddles two samples; D in {1, 2, 7, 5, 31, 32, 33, 41}
SHAPES = [([5, 7, 9], 3), ([2, 3, 50], 2), ([41, 6, 5], 2), ([33, 4, 4], 3), ([32, 4, 4], 2), ([31, 5, 3], 2), ([1, 9, 37], 2), ([7, 1, 11], 3)]
DENSITIES = [0.05, 0.3, 1.0]
# (ksize, stride, pad): the encoders' own three, then what the ABI accepts and no encoder uses
GEOMS = [
    ([3, 3, 3], [2, 2, 2], [1, 1, 1]),
    ([3, 3, 3], [2, 2, 2], [0, 1, 1]),
    ([3, 1, 1], [2, 1, 1], [0, 0, 0]),
    ([1, 1, 1], [1, 1, 1], [0, 0, 0]),
    ([2, 2, 2], [2, 2, 2], [0, 0, 0]),
    ([3, 3, 3], [3, 3, 3], [1, 1, 1]),   # the stride that is no power of two
    ([3, 3, 3], [1, 1, 1], [0, 0, 0]),
    ([3, 3, 3], [1, 1, 1], [2, 2, 2]),   # pad > ks/2: the output grid is larger than the input grid
    ([1, 3, 3], [1, 2, 2], [0, 1, 1]),
    ([5, 1, 1], [2, 1, 1], [2, 0, 0]),
    ([3, 3, 3], [4, 4, 4], [1, 1, 1]),   # stride > ksize: some inputs reach no output
    ([1, 1, 1], [2, 2, 2], [0, 0, 0]),
]
SUBM_KSIZES = [[3, 3, 3], [1, 1, 1], [5, 1, 1], [1, 3, 3], [3, 1, 3]]
SUBM_KSIZES_HASH_ONLY = [[2, 2, 2]]      # the bitmap route answers SRF_EUNSUPPORTED
MAX_K = 27


class Rules:
    """the definition; each method is one rule"""

    @staticmethod
    def div(a, b):                        # the division of out_shape
        return a // b

    @staticmethod
    def fits(padded, ks):                 # the window fits the padded grid (with floor division: the same as an output extent >= 1)
        return padded >= ks

    @staticmethod
    def centre(ks):                       # SubM: offset of the kernel's centre
        return ks // 2

    @staticmethod
    def divisible(t, stride):             # strided: t is a whole number of strides
        return t % stride == 0

    @staticmethod
    def inside(q, oshape):                # strided: the output lies in the output grid
        return q < oshape

    @staticmethod
    def lookup_key(b, z, y, x, shape):    # what identifies a site when a row is looked up
        return ((b * shape[0] + z) * shape[1] + y) * shape[2] + x

    @staticmethod
    def sort_key(b, z, y, x, shape):      # the order of a sorted active set: (b, y, x, z)
        return ((b * shape[1] + y) * shape[2] + x) * shape[0] + z

    @staticmethod
    def sample_cells(shape):              # cells between the first cell of sample b and of sample b + 1
        return shape[0] * shape[1] * shape[2]


RULES = Rules()


def out_shape(shape, ksize, stride, pad, rules=RULES):
    return [int(rules.div(shape[d] + 2 * pad[d] - ksize[d], stride[d])) + 1 for d in range(3)]


def valid_geometry(shape, ksize, stride, pad, rules=RULES):
    """all extents >= 1, the window fits the padded grid in every dimension, K <= 27"""
    if min(shape) < 1 or min(ksize) < 1 or min(stride) < 1 or min(pad) < 0 or int(np.prod(ksize)) > MAX_K:
        return False
    return all(o >= 1 for o in out_shape(shape, ksize, stride, pad, rules)) and all(rules.fits(shape[d] + 2 * pad[d], ksize[d]) for d in range(3))


def overflow_geoms(shape):
    """the geometries the capacity tests run at: the first three valid ones of the table and the stride that is no power of two"""
    valid = [g for g in GEOMS if valid_geometry(shape, *g)]
    return valid[:3] + [g for g in GEOMS[5:6] if g not in valid[:3]]


def active_set(shape, batch, density, seed):
    """distinct sites of a (batch, D, H, W) grid, each with probability `density`, rows shuffled; never empty"""
    rng = np.random.default_rng(seed)
    occ = rng.random((batch, *shape)) < density
    if not occ.any():
        occ.flat[rng.integers(occ.size)] = True
    idx = np.argwhere(occ).astype(np.int32)
    return np.ascontiguousarray(idx[rng.permutation(len(idx))])


def cases():
    """(name, shape, batch, density, indices) over SHAPES x DENSITIES; the seed depends on the case alone"""
    for si, (shape, batch) in enumerate(SHAPES):
        for di, density in enumerate(DENSITIES):
            yield f"{shape}x{batch}@{density}", shape, batch, density, active_set(shape, batch, density, 100 * si + di)


def offsets(ksize):
    """(K, 3) kernel offsets (kz, ky, kx) in the order of k"""
    return np.array([(kz, ky, kx) for kz in range(ksize[0]) for ky in range(ksize[1]) for kx in range(ksize[2])], np.int64).reshape(-1, 3)


def _cols(indices):
    i = np.asarray(indices, np.int64).reshape(-1, 4)
    return i[:, 0], i[:, 1], i[:, 2], i[:, 3]


def cells(indices, shape, rules=RULES):
    return rules.sort_key(*_cols(indices), shape)


def _row_lookup(indices, shape, rules):
    """site -> row as a function of coordinate arrays (sites outside the grid and inactive sites give -1)"""
    b, z, y, x = _cols(indices)
    nb = int(b.max()) + 1 if len(b) else 1
    table = np.full(nb * shape[0] * shape[1] * shape[2], -1, np.int64)
    table[rules.lookup_key(b, z, y, x, shape)] = np.arange(len(b))

    def find(qb, qz, qy, qx):
        ok = (qz >= 0) & (qz < shape[0]) & (qy >= 0) & (qy < shape[1]) & (qx >= 0) & (qx < shape[2])
        key = np.where(ok, rules.lookup_key(qb, qz, qy, qx, shape), 0)
        return np.where(ok, table[key], -1)

    return find


def _counts(nbr):
    return (nbr >= 0).sum(1).astype(np.int32)


def subm(indices, shape, ksize, rules=RULES):
    """-> nbr (K, A), counts (K,)"""
    b, z, y, x = _cols(indices)
    find = _row_lookup(indices, shape, rules)
    off = offsets(ksize)
    nbr = np.full((len(off), len(b)), -1, np.int32)
    c = [rules.centre(int(k)) for k in ksize]
    for k, (kz, ky, kx) in enumerate(off):
        nbr[k] = find(b, z + kz - c[0], y + ky - c[1], x + kx - c[2])
    return nbr, _counts(nbr)


def candidates(indices, shape, ksize, stride, pad, rules=RULES):
    """every (input row i, offset k) that reaches an output, ascending in (i, k): -> i, k, the output sites (n, 4), and how many
    candidates each of the three rejection clauses turned down (t < 0, t % stride != 0, q >= out_shape, decided in this order)"""
    idx = np.asarray(indices, np.int64).reshape(-1, 4)
    osh = np.array(out_shape(shape, ksize, stride, pad, rules), np.int64)
    st = np.array(stride, np.int64)
    t = idx[:, None, 1:4] + np.array(pad, np.int64) - offsets(ksize)[None]           # (A, K, 3)
    neg = t < 0
    rem = ~neg & ~rules.divisible(t, st)
    q = np.where(neg, 0, t) // st
    far = ~neg & ~rem & ~rules.inside(q, osh)
    ok = ~(neg | rem | far).any(-1)
    i, k = np.nonzero(ok)                                                            # row-major: i*K + k ascending
    sites = np.concatenate([idx[i, :1], q[i, k]], 1)
    return i, k, sites, (int(neg.any(-1).sum()), int((~neg.any(-1) & rem.any(-1)).sum()), int((~(neg | rem).any(-1) & far.any(-1)).sum()))


def strided_first_seen(indices, shape, ksize, stride, pad, rules=RULES):
    """the hash route -> out_indices (A_out, 4), nbr (K, A_out), counts (K,)"""
    K = int(np.prod(ksize))
    i, k, sites, _ = candidates(indices, shape, ksize, stride, pad, rules)
    if len(i) == 0:
        return np.zeros((0, 4), np.int32), np.full((K, 0), -1, np.int32), np.zeros(K, np.int32)
    uniq, first, inv = np.unique(sites, axis=0, return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[by_first] = np.arange(len(uniq))
    nbr = np.full((K, len(uniq)), -1, np.int32)
    nbr[k, number[inv.ravel()]] = i
    return uniq[by_first].astype(np.int32), nbr, _counts(nbr)


def strided_sorted(indices, shape, ksize, stride, pad, rules=RULES):
    """the bitmap route, output-stationary: the reached output sites sorted by cell, and for each of them and each offset k the row of
    the input site q*stride - pad + k -> out_indices, nbr, counts"""
    K = int(np.prod(ksize))
    osh = out_shape(shape, ksize, stride, pad, rules)
    _, _, sites, _ = candidates(indices, shape, ksize, stride, pad, rules)
    if len(sites) == 0:
        return np.zeros((0, 4), np.int32), np.full((K, 0), -1, np.int32), np.zeros(K, np.int32)
    out = np.unique(sites, axis=0)
    out = out[np.argsort(cells(out, osh, rules), kind="stable")]
    find = _row_lookup(indices, shape, rules)
    nbr = np.full((K, len(out)), -1, np.int32)
    for k, (kz, ky, kx) in enumerate(offsets(ksize)):
        nbr[k] = find(out[:, 0], out[:, 1] * stride[0] - pad[0] + kz, out[:, 2] * stride[1] - pad[1] + ky, out[:, 3] * stride[2] - pad[2] + kx)
    return out.astype(np.int32), nbr, _counts(nbr)


def sort_order(indices, shape, rules=RULES):
    """order[r] = the row of `indices` that is row r of the sorted set"""
    return np.argsort(cells(indices, shape, rules), kind="stable").astype(np.int32)


def bitmap(indices, shape, batch, rules=RULES):
    """-> words (uint32, ceil(cells / 32)), prefix (int32, exclusive popcount prefix)"""
    c = cells(indices, shape, rules)
    words = np.zeros((batch * shape[0] * shape[1] * shape[2] + 31) // 32, np.uint32)
    np.bitwise_or.at(words, c >> 5, (np.uint32(1) << (c & 31).astype(np.uint32)))
    pop = np.array([bin(int(w)).count("1") for w in words], np.int64)
    return words, (np.cumsum(pop) - pop).astype(np.int32)


def set_cells(words):
    """the set bits of a bitmap, ascending"""
    w = np.asarray(words, np.uint32)
    bits = (w[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return np.flatnonzero(bits.ravel()).astype(np.int64)


def decode(cell, shape, rules=RULES):
    """cells -> (n, 4) int32 (b, z, y, x)"""
    c = np.asarray(cell, np.int64)
    b, c = c // rules.sample_cells(shape), c % rules.sample_cells(shape)
    z, c = c % shape[0], c // shape[0]
    x, y = c % shape[2], c // shape[2]
    return np.stack([b, z, y, x], 1).astype(np.int32)


def clip_rows(nbr, rows):
    """what a consumer sees of a level of which only `rows` rows exist: every row index >= rows is -1"""
    return np.where(nbr >= rows, -1, nbr).astype(np.int32)


def overflowed(ref, cap, in_rows):
    """what the contract predicts of a strided step (`ref` = strided_sorted(...)) whose output arrays hold only `cap` rows, over an input
    level of `in_rows` rows: the first `cap` sorted output rows and their nbr columns.  A consumer of that level then sees
    clip_rows(its own reference, cap)."""
    out_idx, nbr, _ = ref
    return out_idx[:cap], clip_rows(nbr[:, :cap], in_rows)
