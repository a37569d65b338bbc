"""`ops.msda_backward` (csrc/msda_bwd.hip) against the float64 definition of tests/msda_bwd_ref.py on the same float32 inputs cast up.

Bound, counted from the kernel's own operation order (u = 2^-24, gamma_k = k u / (1 - k u)); the magnitude sums M*, A*, the add count Nv,
max |px|, max |py| and the `kink` mask come from the reference (its module text defines them), the bound itself is `msda_bwd_ref.bounds`:

    |grad_value  - f64| <= gamma_(2 T + 25 + Nv) Mv + 6 u (max |px| + max |py| + 1) Av + 1e-30 Av
    |grad_offs   - f64| <= gamma_(2 T + 31) Mo      + 6 u (max |px| + max |py| + 1) Ao + 1e-30 Ao        (kink samples left out)
    |grad_logits - f64| <= gamma_(4 T + 71) Ml      + 6 u (max |px| + max |py| + 1) Al + 1e-30 Al

  softmax   as in tests/test_gpu_msda.py: t = l - m one rounding seen through exp (T u), expf 2 u, the sum of L P terms (15 additions on
            terms that carry T + 2 each), the reciprocal and the product: a carries (T + 2) + (T + 17) + 2 = 2 T + 21 roundings.  T is the
            largest |l - m| among the logits whose weight is not flushed; a flushed weight is under 1e-45 of the row's largest in float64:
            the 1e-30 terms.
  position  px = fma(ref_x, W, dx) - 0.5 is off by <= 2 u |px| + u / 2, lx = px - floor(px) by as much plus u, 1 - lx by one u more:
            every bilinear factor is off by <= 2 u |p| + 3 u in ABSOLUTE terms.  A corner weight (a product of two factors <= 1) moves
            by <= 2 u (|px| + |py|) + 6 u <= 6 u (|px| + |py| + 1); the x-derivative's factors (1 - ly, ly) by half of that.  t and the
            adds are continuous in the position, also across an integer and across the inside test, where the reference's A sums count
            the corners of the cell next door; the offset gradient is not, hence `kink`.
  grad_value  one add is (a g) (hy hx): 3 roundings and a's; Nv adds and the prefilled value summed in ANY order: gamma_Nv of the sum
            of magnitudes (Higham, gamma_(n-1) for n terms in any order); together 2 T + 24 + Nv, one spare.
  grad_offs   the corner difference (1 rounding, against |v01| + |v00|), hy *, the fma, g *, the butterfly over the head's channels
            (log2 32 = 5 additions at most), a *: 10, and a's: 2 T + 31.
  grad_logits t: the weight product, four fused multiply-adds, g *, the butterfly: 11.  a[j] t[j]: a's, t's, the subtraction, the
            product: 2 T + 34.  a[j] sum_i a[i] t[i]: a twice, t, 16 fused multiply-adds, the subtraction, the product: 4 T + 71, taken for
            both terms.
Conditions on the inputs (tests/test_msda_bwd_ref.py, on the CPU with the reference alone): every reference gradient is finite, the kink
samples are under 0.1 % of the samples, the bound stays below 1e-3 of each tensor's largest entry, and a swapped corner pair, a flipped
sign, a level start off by one row and a dropped softmax term each exceed it."""
import numpy as np
import pytest
import torch

import msda_bwd_ref as R
from srfdet3d_amd import ops

pytestmark = pytest.mark.gpu
KEYS = ("grad_value", "grad_offs", "grad_logits")


def inputs(name, dev):
    """The case's tensors on the GPU, laid out as its row of `R.CASES` says: value in a NaN-padded pitched buffer, offsets and logits as
    views of one buffer when shared."""
    case, _ = R.reference(name)
    heads, d, shapes, B, Q, P, value_ld, gout_ld, shared = R.CASES[name]
    ns = heads * len(shapes) * P
    rows, C = case["ref"].shape[0], heads * d
    vbuf = torch.full((case["value"].shape[0], value_ld), float("nan"), device=dev)
    vbuf[:, :C] = torch.from_numpy(case["value"]).to(dev)
    gbuf = torch.full((rows, gout_ld), float("nan"), device=dev)
    gbuf[:, :C] = torch.from_numpy(case["grad_out"]).to(dev)
    offs = torch.from_numpy(case["offs"]).reshape(rows, 2 * ns).to(dev)
    logits = torch.from_numpy(case["logits"]).reshape(rows, ns).to(dev)
    if shared:
        buf = torch.cat((offs, logits), dim=1).contiguous()
        offs, logits = buf[:, :2 * ns], buf[:, 2 * ns:]
    return dict(value=vbuf[:, :C], ref=torch.from_numpy(case["ref"]).to(dev), offs=offs, logits=logits, grad_out=gbuf[:, :C],
                shapes=shapes, heads=heads, P=P, ns=ns, rows=rows, C=C, shared=shared)


def run(x, need=(True, True, True), out=(None, None, None)):
    got = ops.msda_backward(x["value"], x["shapes"], x["ref"], x["offs"], x["logits"], x["heads"], x["P"], x["grad_out"], need=need, out=out)
    torch.cuda.synchronize()
    return got


_RUN = {}


def plain(name):
    """The three gradients of a case from freshly allocated outputs, computed once."""
    if name not in _RUN:
        _RUN[name] = run(inputs(name, torch.device("cuda")))
    return _RUN[name]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_meets_the_definition(name):
    _, ref = R.reference(name)
    bd = R.bounds(name)
    for key, g in zip(KEYS, plain(name)):
        got = g.double().cpu().numpy()
        keep = np.ones(got.shape, dtype=bool)
        if key == "grad_offs":
            keep = np.repeat(~ref["kink"].reshape(got.shape[0], -1), 2, axis=1)
        assert np.isfinite(got).all()
        err = np.abs(got - ref[key])
        ratio = np.where(bd[key] > 0, err / np.where(bd[key] > 0, bd[key], 1.0), np.where(err > 0, np.inf, 0.0))
        print(name, key, "T", bd["T"], "max |g - g64|", err[keep].max(), "max bound", bd[key][keep].max(), "max err / bound", ratio[keep].max(),
              "largest entry", np.abs(ref[key]).max(), "most adds", int(ref["Nv"].max()))
        assert (err[keep] <= bd[key][keep]).all()


@pytest.mark.parametrize("name", ["d16_pyramid", "d32_pyramid_pitched", "d16_two_levels_p3"])
def test_pitched_shared_and_prefilled_outputs(name):
    """Outputs as column slices of wider buffers (grad_offs and grad_logits of ONE buffer where the case shares its inputs): nothing is
    written beyond the rows' widths, grad_offs and grad_logits have the bits of the plain call, and grad_value is ADDED to what the
    buffer held."""
    dev = torch.device("cuda")
    x = inputs(name, dev)
    ns, C, rows = x["ns"], x["C"], x["rows"]
    nv = x["value"].shape[0]
    vbuf = torch.full((nv, C + 12), -7.0, device=dev)
    pre = torch.from_numpy(np.random.default_rng(5).standard_normal((nv, C)).astype(np.float32)).to(dev)
    vbuf[:, :C] = pre
    if x["shared"]:
        buf = torch.full((rows, 3 * ns + 4), -7.0, device=dev)
        d_offs, d_logits, pads = buf[:, :2 * ns], buf[:, 2 * ns:3 * ns], [buf[:, 3 * ns:]]
    else:
        bo, bl = torch.full((rows, 2 * ns + 8), -7.0, device=dev), torch.full((rows, ns + 4), -7.0, device=dev)
        d_offs, d_logits, pads = bo[:, :2 * ns], bl[:, :ns], [bo[:, 2 * ns:], bl[:, ns:]]
    got = run(x, out=(vbuf[:, :C], d_offs, d_logits))
    assert got[0].data_ptr() == vbuf.data_ptr() and got[1].data_ptr() == d_offs.data_ptr() and got[2].data_ptr() == d_logits.data_ptr()
    assert (vbuf[:, C:] == -7.0).all() and all((p == -7.0).all() for p in pads)
    base = plain(name)
    assert same_bits(d_offs, base[1]) and same_bits(d_logits, base[2])
    bd = R.bounds(name)["grad_value"]      # the bound's add count has room for the prefilled term
    _, ref = R.reference(name)
    err = np.abs(vbuf[:, :C].double().cpu().numpy() - pre.double().cpu().numpy() - ref["grad_value"])
    slack = 2.0 ** -24 * (np.abs(pre.double().cpu().numpy()) + ref["Mv"])      # the prefilled value rides through the sum: one u of it
    assert (err <= bd + slack).all()
    assert (vbuf[:, :C] - pre).abs().max() > 0.1


@pytest.mark.parametrize("name", ["d16_pyramid", "d32_one_map_q3"])
def test_null_outputs_skip_their_gradient(name):
    x = inputs(name, torch.device("cuda"))
    base = plain(name)
    bd = torch.from_numpy(R.bounds(name)["grad_value"]).to(base[0].device)
    for need in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, False, True)):
        got = run(x, need=need)
        assert [g is None for g in got] == [not n for n in need]
        if need[0]:
            assert ((got[0] - base[0]).double().abs() <= 2 * bd).all()
        for k in (1, 2):
            if need[k]:
                assert same_bits(got[k], base[k]), (need, KEYS[k])
    assert run(x, need=(False, False, False)) == (None, None, None)


@pytest.mark.parametrize("name", ["d16_pyramid", "d32_pyramid_pitched"])
def test_two_launches(name):
    """grad_offs and grad_logits: the same bits.  grad_value: float atomics, the two sums within the bound of each other (twice: each is
    within it of the exact sum)."""
    x = inputs(name, torch.device("cuda"))
    base, again = plain(name), run(x)
    assert same_bits(again[1], base[1]) and same_bits(again[2], base[2])
    bd = torch.from_numpy(R.bounds(name)["grad_value"]).to(base[0].device)
    diff = (again[0] - base[0]).double().abs()
    print(name, "grad_value elements that differ between two launches", int((diff > 0).sum()), "of", diff.numel(), "largest", diff.max().item())
    assert (diff <= 2 * bd).all()


@pytest.mark.parametrize("name", ["d16_pyramid", "d32_one_map_q3"])
def test_autograd_node_returns_the_direct_call(name):
    x = inputs(name, torch.device("cuda"))
    base = plain(name)
    value, offs, logits = (x[k].clone().requires_grad_() for k in ("value", "offs", "logits"))
    ref = x["ref"].clone().requires_grad_()
    out = ops.msda_autograd(value, x["shapes"], ref, offs, logits, x["heads"], x["P"])
    assert same_bits(out, ops.msda(x["value"], x["shapes"], x["ref"], x["offs"], x["logits"], x["heads"], x["P"]))
    out.backward(x["grad_out"])
    assert ref.grad is None
    bd = torch.from_numpy(R.bounds(name)["grad_value"]).to(out.device)
    assert ((value.grad - base[0]).double().abs() <= 2 * bd).all()
    assert same_bits(offs.grad, base[1]) and same_bits(logits.grad, base[2])
    # needs_input_grad selects the outputs: with only the logits wanted the other two gradients are not computed
    seen = []
    real = ops.msda_backward
    logits2 = x["logits"].clone().requires_grad_()
    try:
        ops.msda_backward = lambda *a, **k: (seen.append(a[8] if len(a) > 8 else k.get("need")), real(*a, **k))[1]
        ops.msda_autograd(x["value"], x["shapes"], x["ref"], x["offs"], logits2, x["heads"], x["P"]).backward(x["grad_out"])
    finally:
        ops.msda_backward = real
    assert seen == [(False, False, True)] and same_bits(logits2.grad, base[2])


def test_refusals_on_the_gpu():
    dev = torch.device("cuda")
    value, ref = torch.zeros(35, 128, device=dev), torch.zeros(35, 1, 2, device=dev)
    offs, logits, gout = torch.zeros(35, 64, device=dev), torch.zeros(35, 32, device=dev), torch.zeros(35, 128, device=dev)
    got = ops.msda_backward(value, [(5, 7)], ref, offs, logits, 8, 4, gout)
    assert [tuple(g.shape) for g in got] == [(35, 128), (35, 64), (35, 32)]
    with pytest.raises(RuntimeError, match="msda_supported"):
        ops.msda_backward(torch.zeros(35, 64, device=dev), [(5, 7)], ref, offs, logits, 8, 4, gout[:, :64])      # head_dim 8
    with pytest.raises(ValueError):
        ops.msda_backward(value, [(5, 7)], ref, offs, logits, 8, 4, gout[:30])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.msda_backward(value, [(5, 7)], ref, offs, logits, 8, 4, gout.cpu())
    empty = ops.msda_backward(value[:0], [(5, 7)], ref[:0], offs[:0], logits[:0], 8, 4, gout[:0])                  # nothing to do
    assert [tuple(g.shape) for g in empty] == [(0, 128), (0, 64), (0, 32)]
