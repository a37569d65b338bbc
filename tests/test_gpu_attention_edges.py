"""`srf_self_attention(_batched)` and `srf_dynconv_mid` (csrc/decoder.hip) against the float64 definitions of tests/decoder_ref.py at the
edges of their tilings, on the same float32 inputs cast up.

Attention.  One workgroup per (head, 16 queries, sample); the 16 lanes of a query take every 16th key of each 128-key tile, keep an online
softmax state (max, sum, o) and merge the 16 states in 4 shuffle steps.  P in {1, 15, 16, 17, 128, 129, 257}: fewer keys than lanes (some
lanes merge an empty state), a partial query block, both sides of the key tile, three tiles.  Data is unit-scale, or wide: q scaled until
the widest row has max |s - max s| = 60, and the last key planted along one row's query so that row's maximum moves at the very end.
Bound, counted from the kernel's operation order (u = 2^-24, gamma(k) = k u / (1 - k u)), D = sum_j a_j |v_j|:

    |out - out64| <= (gamma(6 T + 8 n + 3) + 2 gamma(d + 2) S) D          n = ceil(P / 16) + 4,  T = max |s - max s| of the (row, head)

  logits    q * (1 / sqrt(d)): the constant and the product round once each; d products and additions (no contraction): every logit is
            off by <= gamma(d + 2) sum_i |q_i| |k_i| / sqrt(d) <= gamma(d + 2) S.  A softmax weight moves by its own logit's error minus the
            weighted mean of all of them: relatively 2 gamma(d + 2) S.
  exp       a term's weight is __expf(s - m_1) __expf(m_1 - m_2) ... __expf(m_last - m): the running maximum only grows, so the
            arguments add up to s - m, at most T in magnitude.  Each argument is a rounded difference (u |x|), and __expf(x) =
            exp2(x log2 e) rounds the product and carries the constant's error (2 u |x|): 3 u T over the chain.  The exp2 itself is
            one ulp, 2 u, once per key the lane sees after this one and once per merge step: at most n times.            3 T + 2 n
  sums      v * p, then per later key and per merge step one product with the correction and one addition: 2 n + 1 for the numerator,
            2 n for the denominator.                                                                                        2 n + 1
  the denominator carries the same 3 T + 2 n + 2 n on each of its terms, so on the whole;  the division rounds once (counted 2)
  No weight that matters is flushed: T <= 60 < 87 keeps every exp above the smallest normal float32 (checked on the CPU).

DynamicConv.  S in {1, 15, 16, 17, 49, 64} (rows padded to 64: 16-row MFMA tiles on both sides of a tile edge, the workload's 49, no
padding at all), R in {1, 3}, both (C, D); every input tensor ends exactly at its last element, so the clamped reads of the padded rows
must stay inside proposal R - 1.  Bound, with the rules of tests/test_gpu_linear_routes.py:

    e0 = gamma(C) sum |f| |w1|                                 the C terms of product 1 accumulate one after the other on the MFMA
    e1 = layernorm_bound(LN_D, e0, adds = D / 4 + 2)           4 lanes per row: D / 4 values per lane, 2 shuffles;  ReLU is 1-Lipschitz
    e2 = e1 |w2| + gamma(D) sum x1 |w2|                        product 2: the incoming error through |W2|, and its own D terms
    e3 = layernorm_bound(LN_C, e2, adds = C / 16 + 4)          16 lanes per row: C / 16 accumulators per lane, 4 shuffles

Conditions on the inputs are checked with the references alone in tests/test_decoder_ref.py: every bound stays below 1e-3 of the largest
|reference| entry of its case and each listed mutation of the reference exceeds it."""
import numpy as np
import pytest
import torch

import decoder_ref as R
from srfdet3d_amd import _lib, ops

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0

# name: (B, P, E, H, wide)
ATT_CASES = {
    "p1_e128": (1, 1, 128, 8, False),
    "p1_e64_b3_wide": (3, 1, 64, 4, True),
    "p15_e128_b3_wide": (3, 15, 128, 8, True),
    "p15_e32": (1, 15, 32, 1, False),
    "p16_e256": (1, 16, 256, 8, False),
    "p16_e64_wide": (1, 16, 64, 4, True),
    "p17_e64_wide": (1, 17, 64, 4, True),
    "p17_e128_b3": (3, 17, 128, 8, False),
    "p128_e32_wide": (1, 128, 32, 1, True),
    "p128_e128": (1, 128, 128, 8, False),
    "p129_e256_wide": (1, 129, 256, 8, True),
    "p129_e64_b3": (3, 129, 64, 4, False),
    "p257_e128_wide": (1, 257, 128, 8, True),
    "p257_e32": (1, 257, 32, 1, False),
}
# name: (R, S, C, D)
DYN_CASES = {f"c{C}_s{S}_r{Rr}": (Rr, S, C, D)
             for (C, D), shapes in {(128, 32): [(1, 1), (3, 15), (1, 16), (3, 17), (3, 49), (1, 64)],
                                    (256, 64): [(3, 1), (1, 15), (3, 16), (1, 17), (1, 49), (3, 64)]}.items()
             for Rr, S in shapes}
_REF = {}
RATIOS = {}


def att_reference(name):
    """(qkv float32, float64 reference) of a case, computed once and left unchanged."""
    if ("att", name) not in _REF:
        B, P, E, H, wide = ATT_CASES[name]
        qkv = R.attention_inputs(B, P, E, H, wide, seed=sorted(ATT_CASES).index(name) + 301)
        _REF["att", name] = (qkv, R.attention_ref(qkv, B, P, E, H))
    return _REF["att", name]


def att_bound(name):
    B, P, E, H, _ = ATT_CASES[name]
    ref = att_reference(name)[1]
    d = E // H
    n = (P + 15) // 16 + 4
    rel = R.gamma(6 * ref["T"] + 8 * n + 3) + 2 * R.gamma(d + 2) * ref["S"]        # (B P, H)
    return np.repeat(rel, d, axis=1) * ref["D"]


def dyn_reference(name):
    if ("dyn", name) not in _REF:
        Rr, S, C, D = DYN_CASES[name]
        inp = R.dynconv_inputs(Rr, S, C, D, seed=sorted(DYN_CASES).index(name) + 501)
        _REF["dyn", name] = (inp, R.dynconv_mid_ref(*inp))
    return _REF["dyn", name]


def dyn_bound(name):
    Rr, S, C, D = DYN_CASES[name]
    ref = dyn_reference(name)[1]
    e0 = R.gamma(C) * ref["mag1"].reshape(Rr * S, D)
    e1 = R.layernorm_bound(ref["ln1"], e0, D // 4 + 2).reshape(Rr, S, D)
    e2 = e1 @ ref["w2_abs"] + R.gamma(D) * ref["mag2"]
    e3 = R.layernorm_bound(ref["ln2"], e2.reshape(Rr * S, C), C // 16 + 4)
    return e3.reshape(Rr, S, C)


def _record(kind, name, got, want, bd):
    err = np.abs(got - want)
    ratio = float((err / bd).max())                    # every bound is positive: sum a |v| > 0, and a LayerNorm adds u |out| and more
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)
    print(f"{kind} {name}: max err {err.max():.3e}  max bound {bd.max():.3e}  max err / bound {ratio:.3f}  (so far {RATIOS[kind]:.3f})")
    return ratio


@pytest.mark.parametrize("name", sorted(ATT_CASES))
def test_attention_within_the_counted_bound(dev, name):
    B, P, E, H, wide = ATT_CASES[name]
    qkv, ref = att_reference(name)
    buf = torch.full((B * P + 3, E), SENTINEL, dtype=torch.float32, device=dev)
    out = ops.self_attention(torch.from_numpy(qkv).to(dev), H, out=buf[:B * P], batch=B)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert (buf[B * P:] == SENTINEL).all()                       # the rows after the last query are not written
    got = buf[:B * P].double().cpu().numpy()
    assert np.isfinite(got).all()
    assert _record("attention_wide" if wide else "attention_unit", name, got, ref["out"], att_bound(name)) <= 1.0
    again = ops.self_attention(torch.from_numpy(qkv).to(dev), H, batch=B)
    assert torch.equal(again, buf[:B * P])


def test_batched_launch_equals_the_per_sample_launches_at_p17(dev):
    """A partial query block per sample: the second and third samples start in the middle of what would be a block of the flat rows."""
    B, P, E, H, _ = ATT_CASES["p17_e128_b3"]
    qkv = torch.from_numpy(att_reference("p17_e128_b3")[0]).to(dev)
    att = ops.self_attention(qkv, H, batch=B)
    for b in range(B):
        assert torch.equal(att[b * P:(b + 1) * P], ops.self_attention(qkv[b * P:(b + 1) * P].contiguous(), H))


@pytest.mark.parametrize("name", sorted(DYN_CASES))
def test_dynconv_mid_within_the_counted_bound(dev, name):
    Rr, S, C, D = DYN_CASES[name]
    (feats, params, ln1, ln2), ref = dyn_reference(name)

    def exact(a):                      # a tensor of its own, as long as its data and no longer
        t = torch.empty(a.size, dtype=torch.float32, device=dev)
        t.copy_(torch.from_numpy(a.reshape(-1)))
        return t

    f, p = exact(feats), exact(params)
    g1, b1, g2, b2 = exact(ln1[0]), exact(ln1[1]), exact(ln2[0]), exact(ln2[1])
    buf = torch.full((Rr * S + 2, C), SENTINEL, dtype=torch.float32, device=dev)
    rc = _lib.lib().srf_dynconv_mid(ops._ptr(f), ops._ptr(p), Rr, S, C, D, ops._ptr(g1), ops._ptr(b1), ln1[2], ops._ptr(g2), ops._ptr(b2),
                                    ln2[2], ops._ptr(buf), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (buf[Rr * S:] == SENTINEL).all()                      # the padded rows S..63 of the last proposal are not stored
    got = buf[:Rr * S].double().cpu().numpy().reshape(Rr, S, C)
    assert np.isfinite(got).all()
    assert _record(f"dynconv_{C}_{D}", name, got, ref["out"], dyn_bound(name)) <= 1.0
    via_ops = ops.dynconv_mid(f.view(Rr, S, C), p.view(Rr, -1), (g1, b1, ln1[2]), (g2, b2, ln2[2]))
    assert torch.equal(via_ops.reshape(Rr * S, C), buf[:Rr * S])
