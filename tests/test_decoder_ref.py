"""Conditions on the inputs of tests/test_gpu_linear_routes.py and tests/test_gpu_attention_edges.py, checked with the float64
references of tests/decoder_ref.py alone (no GPU): on every case the largest counted bound stays below 1e-3 of the largest |reference|
entry, and each deliberate defect of the reference moves at least one element by more than its bound -- so a kernel with that defect
cannot pass under the bound.  Also the references against torch's own float64 operators, and the tables against the host code's rules."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_ref as R
import test_gpu_attention_edges as A
import test_gpu_linear_routes as G


def exceeds(mut, ref, bd):
    return bool((np.abs(mut - ref) > bd).any())


# ------------------------------------------------------------------------------------------------------------------ references
def test_linear_ref_is_the_torch_chain():
    x, w, kw = R.linear_inputs(7, 36, 20, G.FULL, seed=1, integers=False)
    ref = R.linear_ref(x, w, **kw)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    v = F.linear(d(x), d(w), d(kw["bias"]))
    assert torch.allclose(d(ref["pre"]), v, rtol=0, atol=1e-13)
    v = F.relu(F.layer_norm(v, (20,), d(kw["ln1"][0]), d(kw["ln1"][1]), kw["ln1"][2])) + d(kw["residual"])
    v = F.relu(F.layer_norm(v, (20,), d(kw["ln2"][0]), d(kw["ln2"][1]), kw["ln2"][2]))
    assert torch.allclose(d(ref["out"]), v, rtol=0, atol=1e-12)
    assert np.allclose(ref["mag"], np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(kw["bias"]))
    assert np.allclose(ref["ln1"]["rstd"][:, 0], 1 / np.sqrt(ref["pre"].var(1) + 1e-5))
    assert np.allclose(ref["ln1"]["z"], (ref["pre"] - ref["pre"].mean(1, keepdims=True)) * ref["ln1"]["rstd"])


def test_attention_ref_is_torch_mha_core():
    B, P, E, H = 2, 19, 64, 4
    qkv = R.attention_inputs(B, P, E, H, False, seed=2)
    ref = R.attention_ref(qkv, B, P, E, H)
    t = torch.from_numpy(qkv).double().view(B, P, 3, H, E // H)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B * P, E)
    assert torch.allclose(torch.from_numpy(ref["out"]), want, rtol=0, atol=1e-12)
    assert (ref["D"] >= np.abs(ref["out"]) - 1e-12).all() and (ref["T"] >= 0).all()


def test_dynconv_ref_is_the_torch_chain():
    feats, params, ln1, ln2 = R.dynconv_inputs(2, 5, 128, 32, seed=3)
    ref = R.dynconv_mid_ref(feats, params, ln1, ln2)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    w1, w2 = d(params)[:, :128 * 32].view(2, 128, 32), d(params)[:, 128 * 32:].view(2, 32, 128)
    x = F.relu(F.layer_norm(torch.bmm(d(feats), w1), (32,), d(ln1[0]), d(ln1[1]), ln1[2]))
    want = F.relu(F.layer_norm(torch.bmm(x, w2), (128,), d(ln2[0]), d(ln2[1]), ln2[2]))
    assert torch.allclose(d(ref["out"]), want, rtol=0, atol=1e-12)


def test_layernorm_bound_is_at_most_the_row_max_form():
    """The elementwise propagation used is, term by term, at most |g_i| (E / s) (2 + |t_i| / s) for E = the row's largest error."""
    rng = np.random.default_rng(4)
    v = rng.standard_normal((6, 40))
    step = R.layernorm_ref(v, (rng.random(40) + 0.5, rng.standard_normal(40), 1e-5))
    e = rng.random((6, 40)) * 1e-4
    E = e.max(1, keepdims=True)
    t, s, g = np.abs(step["t"]), step["s"], step["g"]
    own = R.layernorm_bound(step, np.zeros_like(e), 8)
    assert (R.layernorm_bound(step, e, 8) - own <= g * (E / s) * (2 + t / s) * (1 + 1e-12)).all()
    # and it does bound a real perturbation of the row, to first order
    dv = e * rng.choice([-1.0, 1.0], e.shape)
    moved = R.layernorm_ref(v + dv, (step["g"], np.zeros(40), 1e-5))["out"] - R.layernorm_ref(v, (step["g"], np.zeros(40), 1e-5))["out"]
    assert (np.abs(moved) <= (R.layernorm_bound(step, e, 8) - own) * (1 + 1e-3)).all()


# ----------------------------------------------------------------------------------------------------------------------- linear
def test_the_linear_table_names_the_route_the_host_code_takes():
    G.test_the_table_names_the_route_the_host_code_takes()
    assert len(G.CASES) == len(G._cases())                                          # no two cases share a name


def test_the_linear_table_covers_the_required_edges():
    by = lambda rt: [c for c in G.CASES.values() if c[0] == rt]
    dims = lambda rt, i: {c[i] for c in by(rt)}
    assert dims("gemv", 1) == {1, 8} and dims("gemv", 2) == {4, 260, 2052} and dims("gemv", 3) == {3, 5, 1028}
    assert dims("plain", 1) >= {9, 33} and dims("plain", 2) >= {36, 2044} and dims("plain", 3) >= {130, 1028}
    assert dims("fused", 3) == {10, 64, 65, 128} and dims("fused", 1) == {8, 37}
    assert {c[4] for c in by("fused")} >= {"ln1", "ln1+relu1", "res", "ln2", "relu2", G.FULL}
    assert dims("slab16", 3) == {129, 200, 1024} and dims("slab16", 1) == {9, 5}
    for rt, ns in (("split2", {10, 128}), ("split16", {129, 1024})):
        for K in (2048, 2052, 2340):
            for N in ns:
                assert {c[4] for c in by(rt) if c[2] == K and c[3] == N} >= {"bias+relu1", G.FULL}
    assert {(c[1], c[2], c[3], c[4]) for c in by("splitcols")} >= {(9, 2048, 1028, "bias+relu1"), (9, 2048, 1100, "bias+relu1")}
    assert max(2 * c[1] * c[2] * c[3] for c in G.CASES.values()) < 50e6               # FLOP: the widest split-K case; every case is a blink


def test_integer_data_stays_exact_in_float32():
    for name in G.EXACT:
        x, w, kw, ref = G.reference(name, True)
        assert ref["mag"].max() + 14 < 2 ** 24 and (ref["out"] == np.round(ref["out"])).all()
        assert np.abs(x).max() <= 3 and np.abs(w).max() <= 2


@pytest.mark.parametrize("name", G.BOUNDED)
def test_linear_bound_is_tight_enough(name):
    _, _, _, ref = G.reference(name, False)
    bd = G.bound(name)
    top = np.abs(ref["out"]).max()
    print(f"{name}: max bound {bd.max():.3e}  max |ref| {top:.3f}  ratio {bd.max() / top:.2e}")
    assert top > 0.25 and bd.max() < 1e-3 * top
    for step in (ref["ln1"], ref["ln2"]):
        if step is not None:
            var = step["s"] ** 2
            assert 0.05 < var.min() and var.max() < 20                                 # row variances of order 1


@pytest.mark.parametrize("name", G.BOUNDED)
def test_linear_mutations_exceed_the_bound(name):
    rt, M, K, N, chain, _, _ = G.CASES[name]
    x, w, kw, ref = G.reference(name, False)
    bd = G.bound(name)
    muts = []
    if K > 32:
        muts += [("chunk", 0), ("chunk", (K - 1) // 32 * 32)]                          # the first chunk and the last (partial) one
    if K >= 2048:
        muts += [("slab", 0), ("slab", (K - 1) // 256)]
    if "bias" in chain:
        muts.append("bias")
    if "ln" in chain:
        muts += ["unbiased", "eps"]
    if "relu1" in chain and "res" in chain:
        muts.append("residual_first")
    for m in muts:
        mut = R.linear_ref(x, w, **kw, mutate=m)["out"]
        assert exceeds(mut, ref["out"], bd), (name, m, np.abs(mut - ref["out"]).max(), bd.max())


# -------------------------------------------------------------------------------------------------------------------- attention
def test_the_attention_table_covers_the_required_edges():
    c = list(A.ATT_CASES.values())
    assert {x[1] for x in c} == {1, 15, 16, 17, 128, 129, 257} and {x[0] for x in c} == {1, 3}
    assert {(x[2], x[3]) for x in c} == {(128, 8), (256, 8), (64, 4), (32, 1)}
    assert {x[4] for x in c} == {False, True} and len(c) <= 14
    d = {(Rr, S, C, D) for Rr, S, C, D in A.DYN_CASES.values()}
    for C, D in ((128, 32), (256, 64)):
        assert {S for Rr, S, c, _ in d if c == C} == {1, 15, 16, 17, 49, 64} and {Rr for Rr, S, c, _ in d if c == C} == {1, 3}


@pytest.mark.parametrize("name", sorted(A.ATT_CASES))
def test_attention_bound_is_tight_enough(name):
    B, P, E, H, wide = A.ATT_CASES[name]
    qkv, ref = A.att_reference(name)
    bd = A.att_bound(name)
    top = np.abs(ref["out"]).max()
    print(f"{name}: T {ref['T'].max():.1f}  S {ref['S'].max():.1f}  max bound {bd.max():.3e}  max |ref| {top:.3f}  ratio {bd.max() / top:.2e}")
    assert top > 0.25 and bd.max() < 1e-3 * top
    assert ref["T"].max() <= 60.0 + 1e-3                                               # no weight that matters is flushed
    if wide and P > 1:
        assert ref["T"].max() > 59.0
        # the planted row: its last key holds the maximum, by a margin that forces a real rescale of what came before
        q = qkv.astype(np.float64).reshape(B, P, 3, H, E // H)
        s = np.einsum("bhd,bkhd->bhk", q[:, P // 2, 0], q[:, :, 1]) / np.sqrt(E // H)
        assert (s.argmax(-1) == P - 1).all() and (s[..., -1] - np.sort(s, -1)[..., -2] > 1.0).all()


@pytest.mark.parametrize("name", sorted(A.ATT_CASES))
def test_attention_mutations_exceed_the_bound(name):
    B, P, E, H, _ = A.ATT_CASES[name]
    qkv, ref = A.att_reference(name)
    bd = A.att_bound(name)
    muts = ["first_twice"] + (["last_key", "scale"] if P > 1 else []) + (["heads"] if H > 1 else [])
    if P == 1:
        muts.remove("first_twice")          # one key: its weight is 1 however often it is counted, and the scale cannot matter
    for m in muts:
        mut = R.attention_ref(qkv, B, P, E, H, mutate=m)["out"]
        assert exceeds(mut, ref["out"], bd), (name, m)


# ------------------------------------------------------------------------------------------------------------------ DynamicConv
@pytest.mark.parametrize("name", sorted(A.DYN_CASES))
def test_dynconv_bound_is_tight_enough_and_mutations_exceed_it(name):
    Rr, S, C, D = A.DYN_CASES[name]
    inp, ref = A.dyn_reference(name)
    bd = A.dyn_bound(name)
    top = np.abs(ref["out"]).max()
    print(f"{name}: max bound {bd.max():.3e}  max |ref| {top:.3f}  ratio {bd.max() / top:.2e}")
    assert top > 0.25 and bd.max() < 1e-3 * top
    muts = ["transposed"] + (["ln1_rows"] if S > 48 else []) + (["neighbour"] if Rr > 1 else [])
    for m in muts:
        assert exceeds(R.dynconv_mid_ref(*inp, mutate=m)["out"], ref["out"], bd), (name, m)
