"""srf_spconv_fwd_bf16 (csrc/spconv_bf16.hip) against its definition tests/spconv_bf16_ref.py:

* exact where the answer is exact (small integers: every partial sum in any order is an integer below 2^24) on hand-built rulebooks
  that hold every bookkeeping edge, and on the real rulebooks of a 6 000-point sweep;
* random data against float64 of the ROUNDED operands: <= 2 x the error of the f32 kernel on the same pre-rounded operands + 1e-7 of the
  summed magnitudes, and under the derivable cap n 2^-23 sum |a b| + one f32 rounding per epilogue operation; against the UNROUNDED
  float64 within (2^-7 + 2^-16) sum |a b| + the same accumulation term;
* bit for bit: the row plan, the capacity, the live row count and the tile a row sits in change nothing; a non-finite input row reaches
  exactly the outputs that gather it;
* the domain lines of the file header (values that round to a bf16 infinity, bf16 subnormals; non-finite weights are outside the domain);
* the routing of `sparse.mfma_dtype`."""
import functools

import numpy as np
import pytest
import torch

import spconv_bf16_ref as R
from bf16_ref import BF16_MAX, FLT_MIN, bf16_round
from oracle import oracle as O
from srfdet3d_amd import _lib, derived, ops, sparse, synthetic as S

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SHAPES = [(27, 32, 64), (27, 64, 64), (27, 64, 128), (27, 128, 128), (3, 128, 128)]
VS, RANGE, SHAPE1 = [0.075, 0.075, 0.2], list(S.NUSC_RANGE), [41, 1472, 1472]
TILE = 128      # output rows of a workgroup (SB_ROWS of csrc/spconv_bf16.hip)


@functools.lru_cache(maxsize=None)
def _sweep():
    """(indices (A, 4), SubM rulebook (27, A), conv_out rulebook (3, A_out)) of a 6 000-point sweep, as tests/test_gpu_spconv.py."""
    _, c, _ = O.hard_voxelize(S.nuscenes_sweep(2000, 6000), VS, RANGE, 10, 160000)
    idx = np.concatenate([np.zeros((len(c), 1), np.int32), c], 1).astype(np.int32)
    subm, _ = O.rulebook_subm(idx, SHAPE1, [3, 3, 3])
    _, down, _, _ = O.rulebook_strided(idx, SHAPE1, [3, 1, 1], [2, 1, 1], [0, 0, 0])
    for a in (idx, subm, down):
        a.setflags(write=False)
    return idx, subm, down


def _real_rulebook(K):
    idx, subm, down = _sweep()
    return (subm if K == 27 else down), len(idx)


def _launch(dev, x, W, nbr, alpha=None, beta=None, res=None, relu=False, rows_dev=None, tiles=None, out=None, packed=None):
    """numpy / torch operands -> the kernel's output (torch, on the device), through the C ABI so that `out` can be pre-filled."""
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(dev)
    x, W, nbr, alpha, beta, res = t(x), t(W), t(nbr), t(alpha), t(beta), t(res)
    K, Cin, Cout = W.shape
    packed = ops.pack_spconv_bf16_weights(W) if packed is None else packed
    A_out = nbr.shape[1]
    out = torch.empty((A_out, Cout), dtype=torch.float32, device=dev) if out is None else out
    p = ops._ptr
    _lib.check(_lib.lib().srf_spconv_fwd_bf16(p(x), x.shape[0], Cin, p(packed), K, p(nbr), nbr.stride(0), A_out, Cout, p(alpha), p(beta), p(res),
                                              int(relu), p(out), p(rows_dev), p(tiles), ops._stream()), "spconv_fwd_bf16")
    return out


# ------------------------------------------------------------------------------------------------------------------ exact
def _hand_rulebook(rng, K, A_in, A_out, counts):
    """nbr (K, A_out): offset k holds exactly counts[k] pairs (None: ~40 % of the rows); one output row (A_out >= 2) has no pair at all;
    input row 3 is gathered by every pair of the last random offset; the last input row is used."""
    nbr = np.full((K, A_out), -1, np.int32)
    empty = A_out // 2 if A_out >= 2 else -1
    rows = np.array([r for r in range(A_out) if r != empty])
    for k in range(K):
        n = counts[k]
        o = rows[rng.random(len(rows)) < 0.4] if n is None else rng.choice(rows, size=min(n, len(rows)), replace=False)
        nbr[k, o] = rng.integers(0, A_in, size=len(o))
    rnd = [k for k in range(K) if counts[k] is None]
    if rnd:
        nbr[rnd[-1]][nbr[rnd[-1]] >= 0] = 3
    k_any = next((k for k in range(K) if (nbr[k] >= 0).any()), None)
    if k_any is not None:
        nbr[k_any, np.nonzero(nbr[k_any] >= 0)[0][0]] = A_in - 1
    return nbr, empty


def _int_case(rng, K, Cin, Cout, A_in, nbr, epi):
    x = rng.integers(-15, 16, size=(A_in, Cin)).astype(np.float32)
    W = rng.integers(-255, 256, size=(K, Cin, Cout)).astype(np.float32)
    alpha = beta = res = None
    if epi:
        alpha = rng.choice([0.5, 1.0, 2.0], size=Cout).astype(np.float32)
        beta = rng.integers(-8, 9, size=Cout).astype(np.float32)
        res = rng.integers(-8, 9, size=(nbr.shape[1], Cout)).astype(np.float32)
    return x, W, alpha, beta, res


def _assert_exact(dev, x, W, nbr, alpha, beta, res, relu):
    acc, mag, _ = R.conv(x, W, nbr)
    assert 27 * 128 * 15 * 255 < 2 ** 24
    worst = mag * (1.0 if alpha is None else np.abs(alpha).max()) + (0.0 if beta is None else np.abs(beta).max() + np.abs(res).max())
    assert worst.max() < 2 ** 24            # every partial sum, in any order, and every epilogue step is an exactly representable number
    want = torch.from_numpy(R.epilogue(acc, alpha, beta, res, relu))
    got = _launch(dev, x, W, nbr, alpha, beta, res, relu).cpu()
    assert torch.equal(got.double(), want), (got.double() - want).abs().max()
    return acc, want


@pytest.mark.parametrize("K,Cin,Cout", SHAPES)
def test_exact_on_hand_built_rulebooks(dev, K, Cin, Cout):
    rng = np.random.default_rng(K * 100000 + Cin * 1000 + Cout)
    if K == 27:
        variants = [[0, 1, 15, 16, 17, 33] + [None] * 21]      # offset 0: no row uses it
    else:
        variants = [[0, 1, 15], [16, 17, 33], [None, 0, None]]
    A_in = 77
    for A_out in (1, 15, 16, 17, TILE, TILE + 1):
        for counts in variants:
            nbr, empty = _hand_rulebook(rng, K, A_in, A_out, counts)
            assert ((nbr == A_in - 1).any() or not (nbr >= 0).any()) and all(c is None or (nbr[k] >= 0).sum() == min(c, A_out - (A_out >= 2)) for k, c in enumerate(counts))
            for epi in (False, True):
                x, W, alpha, beta, res = _int_case(rng, K, Cin, Cout, A_in, nbr, epi)
                acc, want = _assert_exact(dev, x, W, nbr, alpha, beta, res, relu=epi)
                if empty >= 0:              # a row without a pair is epilogue(0)
                    assert not acc[empty].any()
                    assert torch.equal(want[empty], torch.from_numpy(R.epilogue(np.zeros(Cout), alpha, beta, None if res is None else res[empty], epi)))
    # no pair in the whole rulebook
    nbr = np.full((K, 40), -1, np.int32)
    x, W, alpha, beta, res = _int_case(rng, K, Cin, Cout, A_in, nbr, True)
    _assert_exact(dev, x, W, nbr, alpha, beta, res, relu=False)


@pytest.mark.parametrize("K,Cin,Cout", SHAPES)
def test_exact_on_the_rulebooks_of_a_sweep(dev, K, Cin, Cout):
    rng = np.random.default_rng(K * 100000 + Cin * 1000 + Cout + 1)
    nbr, A_in = _real_rulebook(K)
    assert nbr.shape[1] > 4 * TILE and nbr.shape[1] % TILE != 0 and (K == 27) == (nbr.shape[1] == A_in)
    x, W, alpha, beta, res = _int_case(rng, K, Cin, Cout, A_in, nbr, True)
    acc, _ = _assert_exact(dev, x, W, nbr, alpha, beta, res, relu=True)
    assert np.abs(acc).max() > 1000
    _assert_exact(dev, x, W, nbr, None, None, None, relu=False)


# ------------------------------------------------------------------------------------------------------------------ random data
@pytest.mark.parametrize("K,Cin,Cout", SHAPES)
def test_random_data_against_float64(dev, K, Cin, Cout):
    rng = np.random.default_rng(K * 100000 + Cin * 1000 + Cout + 2)
    nbr, A_in = _real_rulebook(K)
    A_out = nbr.shape[1]
    x = np.maximum(rng.standard_normal((A_in, Cin)) * 1.5 + 0.2, 0).astype(np.float32)          # post-ReLU-like
    W = (rng.standard_normal((K, Cin, Cout)) / np.sqrt(Cin * 3)).astype(np.float32)
    alpha = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    beta = rng.standard_normal(Cout).astype(np.float32)
    res = rng.standard_normal((A_out, Cout)).astype(np.float32)
    xr, Wr = bf16_round(x), bf16_round(W)
    acc, mag, terms = R.conv(x, W, nbr)
    acc_u, mag_u, _ = R.conv(x, W, nbr, rounded=False)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    packed32 = ops.pack_spconv_weights(t(Wr))
    assert packed32 is not None
    for bn, rs, relu in ((False, False, False), (True, False, True), (True, True, True), (False, True, False)):
        a, b = (alpha, beta) if bn else (None, None)
        r = res if rs else None
        ref, ref_u = R.epilogue(acc, a, b, r, relu), R.epilogue(acc_u, a, b, r, relu)
        got = _launch(dev, x, W, nbr, a, b, r, relu).cpu().double().numpy()
        f32 = ops.spconv_fwd(t(xr), t(Wr), t(nbr), t(a), t(b), t(r), relu, packed=packed32).cpu().double().numpy()
        plain = ops.spconv_fwd(t(x), t(W), t(nbr), t(a), t(b), t(r), relu).cpu().double().numpy()
        sc = 1.0 if a is None else np.abs(a.astype(np.float64))
        # 1. the yardstick is the f32 kernel on the same pre-rounded operands; D = the summed magnitudes of every term of an output
        D = np.maximum(mag * sc + (0.0 if b is None else np.abs(b)) + (0.0 if r is None else np.abs(r)), 1e-30)
        e, e32 = (np.abs(got - ref) / D).max(), (np.abs(f32 - ref) / D).max()
        # 2. the derivable cap: n terms summed in f32 in any order, one rounding for the fma and one for the residual add
        y1 = acc if a is None else acc * a + b
        y2 = y1 if r is None else y1 + r
        epi = (0.0 if a is None else 2.0 ** -24 * np.abs(y1)) + (0.0 if r is None else 2.0 ** -24 * np.abs(y2))
        acc_term = (terms[:, None] * 2.0 ** -23 * mag * sc + epi) * (1 + 2.0 ** -20)
        # (ReLU is 1-Lipschitz: both bounds hold behind it as they do in front of it)
        ratio_cap = (np.abs(got - ref) / np.maximum(acc_term, 1e-300)).max()
        bound_u = (2.0 ** -7 + 2.0 ** -16) * mag_u * sc + acc_term
        ratio_u = (np.abs(got - ref_u) / np.maximum(bound_u, 1e-300)).max()
        print(f"\n[{Cin}->{Cout} k{K} bn={bn} res={rs} relu={relu}] err / D: bf16 kernel {e:.3g}, f32 kernel on the rounded operands {e32:.3g} "
              f"(ratio to 2 e32 + 1e-7: {e / (2 * e32 + 1e-7):.3g}); worst err / cap = {ratio_cap:.3g}; worst err / unrounded bound = {ratio_u:.3g}")
        assert e <= 2.0 * e32 + 1e-7, (e, e32)
        assert (np.abs(got - ref) <= acc_term).all(), ratio_cap
        assert (np.abs(got - ref_u) <= bound_u).all(), ratio_u
        assert not np.array_equal(got, plain)            # other values than the f32 route: the reduced-precision kernel really ran


# ------------------------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("K,Cin,Cout", [(27, 64, 64), (27, 128, 128), (3, 128, 128)])
def test_bits_do_not_depend_on_plan_capacity_or_live_count(dev, K, Cin, Cout):
    rng = np.random.default_rng(K + Cin)
    nbr, A_in = _real_rulebook(K)
    live = nbr.shape[1]
    x = rng.standard_normal((A_in, Cin)).astype(np.float32)
    W = (rng.standard_normal((K, Cin, Cout)) / np.sqrt(Cin * 3)).astype(np.float32)
    alpha, beta = rng.uniform(0.5, 1.5, Cout).astype(np.float32), rng.standard_normal(Cout).astype(np.float32)
    tn = torch.from_numpy(np.array(nbr)).to(dev)
    base = _launch(dev, x, W, tn, alpha, beta, None, True)
    assert torch.equal(base, _launch(dev, x, W, tn, alpha, beta, None, True))                      # two launches, equal bits
    assert torch.equal(base, _launch(dev, x, W, tn, alpha, beta, None, True, tiles=ops.spconv_tiles(tn)))
    cap = (live * 3 // 2 + 7) // 8 * 8
    pad = torch.full((K, cap), -1, dtype=torch.int32, device=dev)
    pad[:, :live] = tn
    rows_dev = torch.tensor([live], dtype=torch.int32, device=dev)
    for tiles in (None, ops.spconv_tiles(pad, rows_dev)):
        out = torch.full((cap, Cout), 7.0, dtype=torch.float32, device=dev)
        _launch(dev, x, W, pad, alpha, beta, None, True, rows_dev=rows_dev, tiles=tiles, out=out)
        assert torch.equal(out[:live], base)
        assert (out[live:] == 7.0).all()                                                         # rows past the live count are not written
    # which rows share a tile: the rulebook shifted by 5 rows gives the same rows 5 further on
    shift = torch.full((K, live + 5), -1, dtype=torch.int32, device=dev)
    shift[:, 5:] = tn
    assert torch.equal(_launch(dev, x, W, shift, alpha, beta, None, True)[5:], base)
    # a live count inside a tile
    part = live - TILE // 2 - 3
    rows_dev.fill_(part)
    out = torch.full((live, Cout), 7.0, dtype=torch.float32, device=dev)
    _launch(dev, x, W, tn, alpha, beta, None, True, rows_dev=rows_dev, out=out)
    assert torch.equal(out[:part], base[:part]) and (out[part:] == 7.0).all()


def test_a_non_finite_input_row_reaches_exactly_the_outputs_that_gather_it(dev):
    K, Cin, Cout = 27, 64, 128
    rng = np.random.default_rng(5)
    nbr, A_in = _real_rulebook(K)
    x = rng.standard_normal((A_in, Cin)).astype(np.float32)
    W = (rng.standard_normal((K, Cin, Cout)) / np.sqrt(Cin * 3)).astype(np.float32)
    clean = _launch(dev, x, W, nbr).cpu()
    i_nan, i_inf = int(np.bincount(nbr[nbr >= 0]).argmax()), A_in - 1        # the most gathered input row, and the last one
    x[i_nan], x[i_inf] = np.nan, np.inf
    hit = torch.from_numpy(((nbr == i_nan) | (nbr == i_inf)).any(0))
    assert 3 <= hit.sum() < nbr.shape[1] // 10
    got = _launch(dev, x, W, nbr).cpu()
    assert not torch.isfinite(got[hit]).any()
    assert torch.equal(got[~hit], clean[~hit]) and torch.isfinite(got[~hit]).all()


# ------------------------------------------------------------------------------------------------------------------ domain
def test_values_that_round_to_a_bf16_infinity(dev):
    """Finite in f32, infinite after the rounding (|x| > 0x1.FEFFFFp127), +-inf and NaN in ACTIVATIONS: IEEE arithmetic on the rounded
    operands of the row's own pairs.  (Non-finite weights are outside the domain: csrc/spconv_bf16.hip.)"""
    K, Cin, Cout, A_in, A_out = 27, 64, 64, 200, 70
    rng = np.random.default_rng(7)
    nbr, _ = _hand_rulebook(rng, K, A_in, A_out, [12] * K)      # ~5 pairs per output: most outputs gather no special row
    x = rng.standard_normal((A_in, Cin)).astype(np.float32)
    W = (rng.standard_normal((K, Cin, Cout)) * 2.0 ** -12).astype(np.float32)
    W[:, 1], W[:, 2] = np.abs(W[:, 1]) + 2.0 ** -20, np.abs(W[:, 2]) + 2.0 ** -20
    W[:, 7, 10:20] = 0.0                                                       # inf x 0 = NaN
    x[5, 7], x[6, 33], x[7, 60] = np.inf, -np.inf, np.nan
    x[20, 3], x[21, 40] = 3.40e38, -float.fromhex("0x1.FFp127")               # finite in f32, infinite after the rounding
    x[22, 9] = BF16_MAX                                                        # the largest bf16 itself stays finite
    x[30, 1], x[30, 2] = np.inf, -np.inf                                       # inf - inf inside a row, whatever the order
    nbr[0, :8] = [5, 6, 7, 20, 21, 22, 30, 3]
    acc, mag, _ = R.conv(x, W, nbr)
    got = _launch(dev, x, W, nbr).cpu().double().numpy()
    assert np.isnan(acc[0, 12]) and np.isinf(acc[0, 0]) and np.isinf(acc[3, 0]) and np.isnan(acc[6, 0]) and np.isnan(acc[2]).all()
    assert np.array_equal(np.isnan(got), np.isnan(acc))
    assert np.array_equal(np.isposinf(got), np.isposinf(acc)) and np.array_equal(np.isneginf(got), np.isneginf(acc))
    fin = np.isfinite(acc)
    assert fin.sum() > A_out * Cout // 2
    assert (np.abs(got[fin] - acc[fin]) <= K * Cin * 2.0 ** -23 * mag[fin]).all()


@pytest.mark.parametrize("tiny_side", ["activations", "weights"])
def test_operands_whose_rounding_is_subnormal(dev, tiny_side):
    """|x| < 2^-126 after the rounding: the conversion keeps them, the MFMA may flush its inputs.  Held to the derivable bound only, as
    tests/test_gpu_gemm_bf16.py: within sum over those terms of 2^-126 |partner| of the definition (plus the accumulation error)."""
    K, Cin, Cout, A_in, A_out = 27, 64, 64, 60, 90
    rng = np.random.default_rng(11)
    nbr, _ = _hand_rulebook(rng, K, A_in, A_out, [None] * K)

    def tiny(shape):
        kind = rng.integers(0, 3, size=shape)
        sub = rng.integers(1, 1 << 23, size=shape).astype(np.uint32).view(np.float32)              # f32 subnormals
        small = np.exp2(rng.integers(-133, -126, size=shape).astype(np.float64)).astype(np.float32)  # bf16 subnormals, exact
        v = np.where(kind == 0, sub, np.where(kind == 1, small, rng.standard_normal(shape).astype(np.float32)))
        return (v * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)

    other = lambda shape: rng.standard_normal(shape).astype(np.float32)
    x, W = (tiny((A_in, Cin)), other((K, Cin, Cout))) if tiny_side == "activations" else (other((A_in, Cin)), tiny((K, Cin, Cout)))
    acc, mag, terms = R.conv(x, W, nbr)
    xr, Wr = bf16_round(x).astype(np.float64), bf16_round(W).astype(np.float64)
    sx, sw = ((np.abs(xr) < FLT_MIN) & (xr != 0)).astype(np.float64), ((np.abs(Wr) < FLT_MIN) & (Wr != 0)).astype(np.float64)
    partner = np.zeros_like(acc)
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        partner[o] += (sx[nbr[k, o]] @ np.abs(Wr[k])) if tiny_side == "activations" else (np.abs(xr[nbr[k, o]]) @ sw[k])
    got = _launch(dev, x, W, nbr).cpu().double().numpy()
    tol = terms[:, None] * 2.0 ** -23 * mag + FLT_MIN * partner
    err = np.abs(got - acc)
    print(f"\n[{tiny_side}] worst err / bound = {(err / np.maximum(tol, 1e-300)).max():.3g}")
    assert np.isfinite(got).all() and partner.max() > 0
    assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------------------------ routing
def _level(dev, C, seed=3):
    idx, _, _ = _sweep()
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(idx), C, generator=g).to(dev)
    return sparse.SparseConvTensor(feats, torch.from_numpy(np.array(idx)).to(dev), SHAPE1, 1)


def test_routing_inside_and_outside_the_context(dev):
    torch.manual_seed(0)
    subm = sparse.SubMConv3d(64, 64, 3, padding=1, bias=False, indice_key="s").to(dev).eval()
    down = sparse.SparseConv3d(64, 128, 3, stride=2, padding=1, bias=False, indice_key="d").to(dev).eval()
    c16 = sparse.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="s").to(dev).eval()
    c32 = sparse.SubMConv3d(32, 32, 3, padding=1, bias=False, indice_key="s").to(dev).eval()
    with torch.no_grad():
        x64, x16, x32 = _level(dev, 64), _level(dev, 16), _level(dev, 32)
        before = [subm(x64).features.clone(), down(x64).features.clone(), c16(x16).features.clone(), c32(x32).features.clone()]
        assert all("spconv_bf16" not in derived.names(m) for m in (subm, down, c16, c32))
        routes = []
        with sparse.mfma_dtype(BF16, routes=routes) as mode:
            assert sparse.mfma_active()
            got = [subm(x64).features, down(x64).features, c16(x16).features, c32(x32).features]
            with sparse.mfma_dtype(None):
                assert not sparse.mfma_active()
                assert torch.equal(subm(x64).features, before[0])           # switched off inside
            assert sparse.mfma_active()
        assert not sparse.mfma_active()
        assert [r["route"] for r in routes] == ["bf16", "bf16", "f32", "f32"] and mode.launches == 2
        assert routes[0]["why"] is None and all(r["why"] for r in routes[2:]) and routes[0]["layer"].startswith("64->64 k27 subm")
        # the bf16 layers: the direct calls, bit for bit, and other values than the f32 route
        w = subm.weight.view(27, 64, 64)
        rb = x64.level.subm([3, 3, 3])
        assert torch.equal(got[0], ops.spconv_fwd_bf16(x64.features, w, rb.nbr, ops.pack_spconv_bf16_weights(w.detach())))
        w = down.weight.view(27, 64, 128)
        rb, out = x64.level.strided("d", [3, 3, 3], [2, 2, 2], [1, 1, 1])
        assert torch.equal(got[1], ops.spconv_fwd_bf16(x64.features, w, rb.nbr, ops.pack_spconv_bf16_weights(w.detach())))
        assert not torch.equal(got[0], before[0]) and not torch.equal(got[1], before[1])
        assert (got[0] - before[0]).abs().max() < 0.05 * before[0].abs().max()
        assert "spconv_bf16" in derived.names(subm) and "spconv_bf16" in derived.names(down)
        # the other layers keep their f32 bits and hold no bf16 pack
        assert torch.equal(got[2], before[2]) and torch.equal(got[3], before[3])
        assert "spconv_bf16" not in derived.names(c16) and "spconv_bf16" not in derived.names(c32)
        # outside the context: the f32 bits again
        after = [subm(x64).features, down(x64).features, c16(x16).features, c32(x32).features]
        assert all(torch.equal(a, b) for a, b in zip(after, before))
    with pytest.raises(ValueError):
        sparse.mfma_dtype(torch.float16)
    # a layer in training mode, or with gradients enabled, keeps its f32 route inside the context
    routes = []
    with sparse.mfma_dtype(BF16, routes=routes) as mode:
        y = subm(_level(dev, 64))
    assert routes[0]["route"] == "f32" and "gradients" in routes[0]["why"] and mode.launches == 0 and y.features.requires_grad
    with pytest.raises(RuntimeError):
        ops.spconv_fwd_bf16(x64.features, subm.weight.view(27, 64, 64), x64.level.subm([3, 3, 3]).nbr,
                            ops.pack_spconv_bf16_weights(subm.weight.detach().view(27, 64, 64)))


def test_pack_and_support_rules(dev):
    for K, cin, cout in SHAPES:
        assert ops.spconv_bf16_supported(K, cin, cout) and ops.spconv_bf16_why_not(K, cin, cout) in (None, "not faster (profiles/spconv_bf16_layer_bench.json)")
    W = torch.randn(27, 32, 64, device=dev)
    p = ops.pack_spconv_bf16_weights(W)
    assert p.dtype == torch.int16 and p.numel() == 27 * 32 * 64
    # the pack is a permutation of the rounded weights
    assert torch.equal(p.view(BF16).float().sort().values, W.bfloat16().float().flatten().sort().values)
    assert ops.pack_spconv_bf16_weights(torch.randn(27, 16, 32, device=dev)) is None
    assert not ops.spconv_bf16_supported(27, 32, 32) and "no bf16" in ops.spconv_bf16_why_not(27, 16, 16)
