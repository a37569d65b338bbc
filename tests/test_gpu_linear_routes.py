"""`srf_linear` (csrc/decoder.hip) over its whole dispatch map, at the smallest shapes that cross each edge, through
`decoder_ref.call_linear`: every operand a column slice of a wider NaN-filled buffer (ldx = K + 4, ldw = K + 8, ldr = N + 3), Y a column
slice of a sentinel-filled one (ldy = N + 5), the workspace NaN-filled; the contiguous layout once per route.  And `srf_ese_gate`.

The dispatch map (`route` below restates the host code; rows = a LayerNorm, the residual or relu2 is asked for):

    gemv       !rows and M <= 8            srf_linear_gemv_k: one wave per column, float4 fma chains, 6 shuffle adds; no split at any K
    plain      !rows, M > 8, K < 2048      srf_linear_k, bias / relu1 from the accumulators
    fused      rows, N <= 128, K < 2048    srf_linear_k, the row chain in the same launch (also at M <= 8)
    slab16     rows, N > 128, K < 2048     srf_linear_k -> one slab -> srf_rows_epilogue_k<16>
    split2     K >= 2048, N <= 128         ceil(K / 256) slabs -> srf_rows_epilogue_k<2>          (M > 8, or rows)
    split16    K >= 2048, 128 < N <= 1024  the same -> srf_rows_epilogue_k<16>
    splitcols  K >= 2048, N > 1024, !rows  the same -> srf_cols_epilogue_k (bias and relu1 are column-local)
    rows and N > 1024 is SRF_EUNSUPPORTED (tests/test_linear_args.py).

Two kinds of assertion.

Exact, on small-integer data (x in [-3, 3], w in [-2, 2], integer bias and residual: every partial sum is an integer below 6 * 2340 + 14,
far below 2^24, so ANY correct order of summation gives the float64 result exactly): every chain without a LayerNorm must equal the
reference bit for bit, leave the sentinel beyond column N of every row alone, and return the same bits when called again.  This is the
check of the tile, split, mask, pitch and unwritten-column bookkeeping and needs no tolerance.

Bounded, on float data (decoder_ref.linear_inputs), for every chain with a LayerNorm and one plain case per route: |y - y64| <= bound
elementwise, the bound counted from the kernel's operation order (u = 2^-24, gamma(k) = k u / (1 - k u)):

    product    every term x w of an element passes one product rounding (none under an fma) and the additions after it:
                 gemv    4 ceil(K / 256) fmas in the lane, then 6 shuffle additions                       depth 4 ceil(K / 256) + 6
                 MFMA    the K terms of a tile are accumulated one after the other                         depth min(K, 256) per slab
                 slabs   nsplit additions in slab order (the first onto 0)                                + nsplit
    bias       one addition on the finished sum                                                            + 1
               e0 = gamma(depth + 1) (sum |x| |w| + |bias|)
    LayerNorm  decoder_ref.layernorm_bound(step, e, adds): the incoming error propagated to first order -- at most
               |g_i| (E / s) (2 + |t_i| / s) for a row error E -- plus the step's own roundings: the two-pass mean and variance with their
               6 shuffles (adds = NV + 6: NV = 2 values per lane in srf_linear_k's fused chain and srf_rows_epilogue_k<2>, 16 in <16>),
               1 / sqrtf, the affine.
    ReLU       exact, and 1-Lipschitz
    residual   one addition                                                                                + u |v + residual|

Conditions on the inputs are checked with the reference alone in tests/test_decoder_ref.py: the largest bound of a case stays below 1e-3
of its largest |reference| entry, and a dropped K chunk or slab, a skipped bias, the unbiased variance, swapped eps and a residual added
before relu1 each exceed the bound wherever they apply."""
import numpy as np
import pytest
import torch

import decoder_ref as R
from srfdet3d_amd import ops

pytestmark = pytest.mark.gpu
U = R.U32
SENTINEL = 12345.0
FULL = "bias+ln1+relu1+res+ln2+relu2"
NOLN = "bias+relu1+res+relu2"          # every step of the chain that integer data keeps exact


def route(M, K, N, chain):
    """The host code of srf_linear, restated."""
    rows = any(s in chain for s in ("ln1", "ln2", "res", "relu2"))
    if rows and N > 1024:
        return "unsupported"
    if not rows and M <= 8:
        return "gemv"
    if K >= 2048:
        return "split2" if N <= 128 else ("splitcols" if N > 1024 else "split16")
    if rows:
        return "fused" if N <= 128 else "slab16"
    return "plain"


def _cases():
    c = []          # (name, route, M, K, N, chain, contiguous, bounded even without a LayerNorm)
    add = lambda rt, M, K, N, chain, contig=False, bounded=False: c.append(
        (f"{rt}-{M}x{K}x{N}-{chain or 'none'}" + ("-contig" if contig else ""), rt, M, K, N, chain, contig, bounded))
    # gemv: M in {1, 8}; K < 256 leaves lanes idle, K >= 2048 still takes no split; N % 4 != 0 leaves the last workgroup partly empty
    add("gemv", 1, 4, 3, "bias", contig=True)
    add("gemv", 8, 260, 5, "bias+relu1")
    add("gemv", 1, 2052, 1028, "", bounded=True)
    add("gemv", 8, 4, 1028, "bias+relu1")
    add("gemv", 1, 260, 3, "relu1")
    add("gemv", 8, 2052, 5, "bias", bounded=True)
    # one pass, plain: a partial K chunk (36) and the largest unsplit K (2044)
    add("plain", 9, 36, 130, "bias", contig=True)
    add("plain", 9, 2044, 1028, "bias+relu1", bounded=True)
    add("plain", 33, 2044, 130, "")
    add("plain", 33, 36, 1028, "relu1")
    add("plain", 37, 36, 64, "bias", bounded=True)       # N <= 128 without a row step: still the plain epilogue
    # one pass, fused rows: M = 8 with a row epilogue must not take the GEMV
    for N in (10, 64, 65, 128):
        for M in (8, 37):
            add("fused", M, 36, N, FULL)
            add("fused", M, 36, N, NOLN)
    add("fused", 8, 36, 10, "ln1")
    add("fused", 37, 132, 65, "ln1+relu1")
    add("fused", 8, 36, 64, "res")
    add("fused", 37, 36, 128, "ln2")
    add("fused", 8, 132, 65, "relu2")
    add("fused", 37, 132, 128, FULL, contig=True)
    add("fused", 37, 132, 65, NOLN, contig=True)
    # two pass, one slab
    for N in (129, 200, 1024):
        for M in (9, 5):
            add("slab16", M, 132, N, FULL)
            add("slab16", M, 132, N, NOLN)
    add("slab16", 9, 132, 129, "ln2")
    add("slab16", 5, 36, 200, "res", contig=True)
    add("slab16", 9, 36, 200, "ln1+relu1", contig=True)
    # split-K: 2048 = 8 slabs, 2052 = 9 with the last 4 wide (the second round of the reducer's slab loop), 2340 = 10 with the last 36 wide
    for K in (2048, 2052, 2340):
        for N in (10, 128):
            add("split2", 9, K, N, "bias+relu1", bounded=(K == 2340))
            add("split2", 9, K, N, FULL)
        for N in (129, 1024):
            add("split16", 9, K, N, "bias+relu1", bounded=(K == 2340))
            add("split16", 9, K, N, FULL)
    add("split2", 9, 2052, 128, NOLN, contig=True)
    add("split2", 5, 2340, 10, FULL, contig=True)        # M <= 8 with rows: split, not the GEMV
    add("split16", 9, 2052, 129, NOLN, contig=True)
    add("split16", 5, 2048, 200, FULL, contig=True)
    # split-K, plain, N > 1024: before srf_cols_epilogue_k these returned SRF_OK with Y[:, 1024:] unwritten
    add("splitcols", 9, 2048, 1028, "bias+relu1", bounded=True)
    add("splitcols", 9, 2048, 1100, "bias+relu1", contig=True)
    add("splitcols", 9, 2052, 1100, "bias")
    add("splitcols", 9, 2340, 1028, "relu1")
    return c


CASES = {c[0]: c[1:] for c in _cases()}
ROUTES = ("gemv", "plain", "fused", "slab16", "split2", "split16", "splitcols")
EXACT = sorted(n for n, c in CASES.items() if "ln" not in c[4])
BOUNDED = sorted(n for n, c in CASES.items() if "ln" in c[4] or c[6])
_REF = {}
RATIOS = {}     # route -> largest err / bound seen in this run (printed, and recorded in DESIGN.md)


def reference(name, integers):
    """(x, w, chain arguments, float64 reference) of a case, computed once and left unchanged."""
    key = (name, integers)
    if key not in _REF:
        _, M, K, N, chain, _, _ = CASES[name]
        x, w, kw = R.linear_inputs(M, K, N, chain, seed=sorted(CASES).index(name) + 101, integers=integers)
        _REF[key] = (x, w, kw, R.linear_ref(x, w, **kw))
    return _REF[key]


def depth(name):
    rt, M, K, N, _, _, _ = CASES[name]
    if rt == "gemv":
        return 4 * ((K + 255) // 256) + 6
    if K >= 2048:
        return 256 + (K + 255) // 256
    return K + (1 if rt == "slab16" else 0)


def bound(name):
    """The elementwise bound of the module text for the float data of a case."""
    ref = reference(name, False)[3]
    N = CASES[name][3]
    adds = (2 if N <= 128 else 16) + 6
    e = R.gamma(depth(name) + 1) * ref["mag"]
    if ref["ln1"] is not None:
        e = R.layernorm_bound(ref["ln1"], e, adds)
    if ref["residual"] is not None:
        e = e + U * np.abs(ref["res_in"] + ref["residual"])
    if ref["ln2"] is not None:
        e = R.layernorm_bound(ref["ln2"], e, adds)
    return e


def run(name, integers, dev):
    """-> (Y (M, N) of the first call as float64 numpy, whether the sentinel survived, whether a second call gave the same bits)."""
    _, M, K, N, chain, contig, _ = CASES[name]
    x, w, kw, _ = reference(name, integers)
    pad = (0, 0, 0, 0) if contig else (4, 8, 3, 5)

    def view(a, extra):
        buf = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), dtype=torch.float32, device=dev)
        buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
        return buf[:, :a.shape[1]]

    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    xv, wv = view(x, pad[0]), view(w, pad[1])
    rv = None if kw["residual"] is None else view(kw["residual"], pad[2])
    ln = lambda p: None if p is None else (t(p[0]), t(p[1]), p[2])
    args = dict(bias=t(kw["bias"]), ln1=ln(kw["ln1"]), relu1=kw["relu1"], residual=rv, ln2=ln(kw["ln2"]), relu2=kw["relu2"])
    outs = []
    for _ in range(2):
        ybuf = torch.full((M, N + pad[3]), SENTINEL, dtype=torch.float32, device=dev)
        rc, y, _ = R.call_linear(xv, wv, y=ybuf[:, :N], **args)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(ybuf)
    untouched = bool((outs[0][:, N:] == SENTINEL).all()) and bool((outs[1][:, N:] == SENTINEL).all())
    return outs[0][:, :N].double().cpu().numpy(), untouched, torch.equal(outs[0], outs[1])


def test_the_table_names_the_route_the_host_code_takes():
    for name, (rt, M, K, N, chain, _, _) in CASES.items():
        assert route(M, K, N, chain) == rt, name
    for rt in ROUTES:
        mine = [c for c in CASES.values() if c[0] == rt]
        assert any(c[5] for c in mine) and any(not c[5] for c in mine), rt          # contiguous once, pitched otherwise
        assert any("ln" in c[4] or c[6] for c in mine) and any("ln" not in c[4] for c in mine), rt


@pytest.mark.parametrize("name", EXACT)
def test_integer_data_is_exact(dev, name):
    _, _, _, ref = reference(name, True)
    got, untouched, same = run(name, True, dev)
    assert np.abs(ref["mag"]).max() + 14 < 2 ** 24
    bad = np.argwhere(got != ref["out"])
    assert bad.size == 0, f"{name}: {len(bad)} wrong elements, first at {bad[0]}: {got[tuple(bad[0])]} != {ref['out'][tuple(bad[0])]}"
    assert untouched, "written beyond column N"
    assert same, "a second call returned other bits"


@pytest.mark.parametrize("name", BOUNDED)
def test_float_data_within_the_counted_bound(dev, name):
    _, _, _, ref = reference(name, False)
    bd = bound(name)
    got, untouched, same = run(name, False, dev)
    assert np.isfinite(got).all()
    ratio = float((np.abs(got - ref["out"]) / bd).max())
    rt = CASES[name][0]
    RATIOS[rt] = max(RATIOS.get(rt, 0.0), ratio)
    print(f"{name}: max err {np.abs(got - ref['out']).max():.3e}  max bound {bd.max():.3e}  max err / bound {ratio:.3f}  "
          f"(route {rt} so far {RATIOS[rt]:.3f})")
    assert ratio <= 1.0
    assert untouched and same


def test_ops_linear_reaches_the_wide_split_route(dev):
    """`ops.linear` sizes the workspace itself and hands over a torch.empty Y: the N > 1024 split-K product through the wrapper."""
    x, w, kw, ref = reference("splitcols-9x2048x1100-bias+relu1-contig", True)
    t = lambda a: torch.from_numpy(a).to(dev)
    got = ops.linear(t(x), t(w), t(kw["bias"]), relu1=True)
    assert np.array_equal(got.double().cpu().numpy(), ref["out"])


# ------------------------------------------------------------------------------------------------------------------ eSE gate
@pytest.mark.parametrize("N,C", [(1, 4), (8, 4), (1, 260), (8, 260)])
def test_ese_gate_bit_for_bit(dev, N, C):
    """srf_ese_gate = the GEMV with relu6(v + 3) / 6 as its epilogue.  On multiples of 1/8 and 1/4 (integers, scaled so that the sums land
    inside the clamp as well as on both sides of it) every partial sum is exact in any order; the epilogue is __fadd_rn, clamp,
    __fdiv_rn: the same three float32 operations in numpy, bit for bit."""
    rng = np.random.default_rng(N * 1000 + C)
    mean = (rng.integers(-3, 4, (N, C)) / 8).astype(np.float32)
    w = (rng.integers(-2, 3, (C, C)) / 4).astype(np.float32)
    bias = (rng.integers(-4, 5, C) / 4).astype(np.float32)
    v = (mean.astype(np.float64) @ w.astype(np.float64).T + bias).astype(np.float32)
    assert (v.astype(np.float64) == mean.astype(np.float64) @ w.astype(np.float64).T + bias).all()
    want = np.clip(v + np.float32(3.0), np.float32(0.0), np.float32(6.0)) / np.float32(6.0)
    assert want.dtype == np.float32
    got = ops.ese_gate(torch.from_numpy(mean).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if C > 4:
        assert ((want > 0) & (want < 1)).any()
    no_bias = ops.ese_gate(torch.from_numpy(mean).to(dev), torch.from_numpy(w).to(dev), None).cpu().numpy()
    v0 = (mean.astype(np.float64) @ w.astype(np.float64).T).astype(np.float32)
    assert np.array_equal(no_bias.view(np.uint32), (np.clip(v0 + np.float32(3.0), np.float32(0.0), np.float32(6.0)) / np.float32(6.0)).view(np.uint32))
