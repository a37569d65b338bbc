"""Every kernel form of the sparse convolution (csrc/spconv.hip, csrc/spconv_bf16.hip) held to its definition, through the C ABI, over
the full product of

* the epilogue: alpha / beta, residual and ReLU each present or absent (8 combinations of csrc/spconv_frame.hpp's one epilogue);
* `rows_dev`: none, a live count inside a tile that is no multiple of 32, and 0;

and once per form a rulebook that is a column slice of a wider table (`nbr_stride > A_out`).  The bf16 forms also carry rulebook entries at
or above the input row count, which the header of csrc/spconv_bf16.hip defines as "no pair".

Comparators: the oracle's `spconv_fwd`, bit for bit, for the f32 forms (one fma chain per output: offset ascending, channel ascending);
tests/spconv_bf16_ref.py on small integers, where every partial sum is exact in any order, for the bf16 form (as
tests/test_gpu_spconv_bf16.py holds it).  The output is pre-filled: rows at or past `*rows_dev` are "skipped" (srf_spconv_fwd,
include/srfdet3d.h; srf_spconv_fwd_packed takes rows_dev "as in srf_spconv_fwd") / "not written" (srf_spconv_fwd_bf16), so they keep the
fill, and a live count of 0 leaves the whole output as it was.

Each form runs at the smallest shape that selects it: ~300 active sites for the 64- / 128-wide layers and ~700 for the narrower ones give
every form two full tiles and a partial one (the tallest tile is 256 rows); the LDS-weight 16-channel forms need the 70k rows of
tests/test_gpu_spconv.py to cross SRF_C16L_MIN_ROWS."""
import functools
import itertools

import numpy as np
import pytest
import torch

import spconv_bf16_ref as R
from oracle import oracle as O
from srfdet3d_amd import _lib, ops
from test_gpu_spconv import SHAPE1, _level1

pytestmark = pytest.mark.gpu
FILL = 12345.0
EPILOGUES = list(itertools.product((False, True), repeat=3))       # (alpha / beta, residual, relu)

# name: (Cin, Cout, K, rows, entry point, plan)
FORMS = {
    "c16_k<2>": (5, 16, 27, "mid", "fwd", None),
    "c16_k<4>": (16, 16, 27, "mid", "fwd", None),
    "c16l_k<2>": (5, 16, 27, "c16l", "fwd", None),
    "c16l_k<4>": (16, 16, 27, "c16l", "fwd", None),
    "mfma16_k K3": (16, 16, 3, "mid", "fwd", None),
    "mfma16_k Cin32": (32, 16, 27, "mid", "fwd", None),
    "mfma32_k<32>": (32, 32, 27, "mid", "fwd", None),
    "mfma32_k<64>": (48, 64, 27, "small", "fwd", None),
    "mfma32_k<128>": (64, 128, 27, "small", "fwd", None),
    "w32_k<16>": (16, 32, 27, "mid", "packed", None),
    "w32_k<16> order": (16, 32, 27, "mid", "packed", "order"),
    "w32_k<32>": (32, 32, 27, "mid", "packed", None),
    "w32_k<32> order": (32, 32, 27, "mid", "packed", "order"),
    "gsp_k<1,64>": (32, 64, 27, "small", "packed", None),
    "gsp_k<1,64> tiles": (32, 64, 27, "small", "packed", "tiles"),
    "gsp_k<2,64>": (64, 64, 27, "small", "packed", None),
    "gsp_k<2,64> tiles": (64, 64, 27, "small", "packed", "tiles"),
    "gsp_k<2,128>": (64, 128, 27, "small", "packed", None),
    "gsp_k<2,128> tiles": (64, 128, 27, "small", "packed", "tiles"),
    "gsp_k<4,128>": (128, 128, 27, "small", "packed", None),
    "gsp_k<4,128> tiles": (128, 128, 27, "small", "packed", "tiles"),
    "gsp_k<4,128> K3": (128, 128, 3, "small", "packed", None),
    "gsp_k<4,128> K3 tiles": (128, 128, 3, "small", "packed", "tiles"),
    "bf16_k<32,64>": (32, 64, 27, "small", "bf16", None),
    "bf16_k<64,64>": (64, 64, 27, "small", "bf16", None),
    "bf16_k<64,128>": (64, 128, 27, "small", "bf16", None),
    "bf16_k<128,128>": (128, 128, 27, "small", "bf16", None),
    "bf16_k<128,128> K3": (128, 128, 3, "small", "bf16", None),
}
# (grid, occupancy) of the random level behind a rulebook; the live count of the rows_dev case
LEVELS = {("small", 27): ([8, 12, 12], 0.27, 173), ("small", 3): ([8, 16, 16], 0.27, 173),
          ("mid", 27): ([9, 24, 20], 0.165, 397), ("mid", 3): ([9, 32, 32], 0.165, 397)}
TALLEST = {"small": 128, "mid": 256}


@functools.lru_cache(maxsize=None)
def _rulebook(rows, K):
    """(nbr (K, A_out), A_in, live count), read-only and shared by every form of that size"""
    if rows == "c16l":
        idx = _level1(n=30000, batch=3)
        nbr, _ = O.rulebook_subm(idx, SHAPE1, [3, 3, 3])
        assert nbr.shape[1] >= 60000
        live = 40013
    else:
        shape, p, live = LEVELS[rows, K]
        idx = np.argwhere(np.random.default_rng(7).random((1, *shape)) < p).astype(np.int32)
        if K == 27:
            nbr, _ = O.rulebook_subm(idx, shape, [3, 3, 3])
        else:
            _, nbr, _, _ = O.rulebook_strided(idx, shape, [3, 1, 1], [2, 1, 1], [0, 0, 0])
        tile = TALLEST[rows]
        assert nbr.shape[1] > 2 * tile and nbr.shape[1] % tile != 0       # two full tiles and a partial one
        assert tile < live < 2 * tile and live % 32 != 0                    # inside the second tile
    nbr.setflags(write=False)
    return nbr, len(idx), live


@functools.lru_cache(maxsize=None)
def _operands(name):
    """numpy operands and the eight references of a form (computed once, left unchanged)"""
    cin, cout, K, rows, entry, _ = FORMS[name]
    nbr, a_in, live = _rulebook(rows, K)
    rng = np.random.default_rng(cin * 1000 + cout * 10 + K)
    if entry == "bf16":            # small integers: 27 * 128 * 15 * 255 < 2^24, every partial sum and epilogue step is exact
        x = rng.integers(-15, 16, size=(a_in, cin)).astype(np.float32)
        W = rng.integers(-255, 256, size=(K, cin, cout)).astype(np.float32)
        alpha = rng.choice([0.5, 1.0, 2.0], size=cout).astype(np.float32)
        beta = rng.integers(-8, 9, size=cout).astype(np.float32)
        res = rng.integers(-8, 9, size=(nbr.shape[1], cout)).astype(np.float32)
        acc, mag, _ = R.conv(x, W, nbr)
        assert (mag * 2.0 + 16).max() < 2 ** 24
        ref = {e: R.epilogue(acc, alpha if e[0] else None, beta if e[0] else None, res if e[1] else None, e[2]).astype(np.float32)
               for e in EPILOGUES}
    else:
        x = rng.standard_normal((a_in, cin)).astype(np.float32)
        W = (rng.standard_normal((K, cin, cout)) / np.sqrt(cin * 3)).astype(np.float32)
        alpha = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        beta = rng.standard_normal(cout).astype(np.float32)
        res = rng.standard_normal((nbr.shape[1], cout)).astype(np.float32)
        ref = {e: O.spconv_fwd(x, W, nbr, alpha if e[0] else None, beta if e[0] else None, res if e[1] else None, e[2]) for e in EPILOGUES}
    for a in (x, W, alpha, beta, res, *ref.values()):
        a.setflags(write=False)
    return x, W, alpha, beta, res, ref


def _outside(nbr, a_in, seed):
    """the rulebook with a third of its empty entries at or above the input row count: the same pairs for a kernel that reads them as none"""
    rng = np.random.default_rng(seed)
    out = np.array(nbr)
    hit = (out < 0) & (rng.random(out.shape) < 0.33)
    out[hit] = rng.choice([a_in, a_in + 1, a_in + 1000, 2 ** 31 - 1], size=int(hit.sum()))
    assert hit.any()
    return out


def _run(dev, name, t, nbr, epi, rows_dev):
    """one launch through the C ABI into a pre-filled output"""
    cin, cout, K, _, entry, plan = FORMS[name]
    bn, rs, relu = epi
    A_out = nbr.shape[1]
    out = torch.full((A_out, cout), FILL, dtype=torch.float32, device=dev)
    L, p = _lib.lib(), ops._ptr
    tiles = None if plan is None else (ops.spconv_order if plan == "order" else ops.spconv_tiles)(nbr, rows_dev)
    head = (p(t["x"]), t["x"].shape[0], cin)
    tail = (K, p(nbr), nbr.stride(0), A_out, cout, p(t["alpha"]) if bn else None, p(t["beta"]) if bn else None, p(t["res"]) if rs else None,
            int(relu), p(out), p(rows_dev))
    if entry == "fwd":
        _lib.check(L.srf_spconv_fwd(*head, p(t["W"]), *tail, ops._stream()), "spconv_fwd")
    elif entry == "packed":
        _lib.check(L.srf_spconv_fwd_packed(*head, p(t["packed"]), *tail, p(tiles), ops._stream()), "spconv_fwd_packed")
    else:
        _lib.check(L.srf_spconv_fwd_bf16(*head, p(t["packed"]), *tail, p(tiles), ops._stream()), "spconv_fwd_bf16")
    return out.cpu().numpy()


def _device_operands(dev, name):
    cin, cout, K, _, entry, _ = FORMS[name]
    x, W, alpha, beta, res, _ = _operands(name)
    t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in dict(x=x, W=W, alpha=alpha, beta=beta, res=res).items()}
    if entry == "packed":
        assert ops.spconv_packed_supported(K, cin, cout)
        t["packed"] = ops.pack_spconv_weights(t["W"])
    elif entry == "bf16":
        assert ops.spconv_bf16_supported(K, cin, cout)
        t["packed"] = ops.pack_spconv_bf16_weights(t["W"])
    else:
        assert FORMS[name][5] is None
    return t


@pytest.mark.parametrize("name", list(FORMS))
def test_form_over_epilogues_and_live_rows(dev, name):
    cin, cout, K, rows, entry, _ = FORMS[name]
    nbr, a_in, live = _rulebook(rows, K)
    ref = _operands(name)[5]
    t = _device_operands(dev, name)
    t_nbr = torch.from_numpy(_outside(nbr, a_in, 1) if entry == "bf16" else np.array(nbr)).to(dev)
    A_out = nbr.shape[1]
    for n_live in (None, live, 0):
        rows_dev = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=dev)
        n = A_out if n_live is None else n_live
        for epi in EPILOGUES:
            got = _run(dev, name, t, t_nbr, epi, rows_dev)
            assert np.array_equal(got[:n], ref[epi][:n]), (n_live, epi, np.abs(got[:n] - ref[epi][:n]).max())
            assert (got[n:] == FILL).all(), (n_live, epi)           # rows at or past the live count are not written


@pytest.mark.parametrize("name", list(FORMS))
def test_form_on_a_column_slice_of_a_wider_table(dev, name):
    cin, cout, K, rows, entry, _ = FORMS[name]
    nbr, a_in, _ = _rulebook(rows, K)
    ref = _operands(name)[5]
    t = _device_operands(dev, name)
    A_out = nbr.shape[1]
    wide = np.random.default_rng(3).integers(0, a_in, size=(K, A_out + 37)).astype(np.int32)   # other valid pairs beside the slice
    wide[:, 3:3 + A_out] = _outside(nbr, a_in, 2) if entry == "bf16" else nbr
    t_nbr = torch.from_numpy(wide).to(dev)[:, 3:3 + A_out]
    assert t_nbr.stride(0) == A_out + 37 and t_nbr.stride(1) == 1
    epi = (True, True, True)
    got = _run(dev, name, t, t_nbr, epi, None)
    assert np.array_equal(got, ref[epi]), np.abs(got - ref[epi]).max()
