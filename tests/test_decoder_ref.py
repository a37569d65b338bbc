"""Conditions on the inputs of tests/test_gpu_linear_routes.py, tests/test_gpu_attention_edges.py and
tests/test_gpu_stage_tail_edges.py, checked with the float64 references of tests/decoder_ref.py alone (no GPU): on every case the
largest counted bound stays below 1e-3 of the largest |reference|
entry, and each deliberate defect of the reference moves at least one element by more than its bound -- so a kernel with that defect
cannot pass under the bound.  Also the references against torch's own float64 operators, and the tables against the host code's rules."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_ref as R
import test_gpu_attention_edges as A
import test_gpu_linear_routes as G
import test_gpu_stage_tail_edges as S


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


# ------------------------------------------------------------------------------------------- stage tail, apply_deltas, dpg_mix
def test_apply_deltas_ref_is_the_head_formulation():
    """plugin/heads.py::apply_deltas_lidar on float64 tensors, the planted rows included."""
    from srfdet3d_amd.plugin import heads
    from types import SimpleNamespace
    for geom in (R.GEOM, R.GEOM_SHIPPED):
        deltas, boxes = R.apply_deltas_inputs(9, 10, geom, seed=5)
        w, lo, ext, clamp = R.geom64(geom)
        st = SimpleNamespace(bbox_weights=list(w) + [1.0] * 4, pc_range_lidar=list(lo) + list(lo + ext), scale_clamp=clamp)
        want = heads._StageBase.apply_deltas_lidar(st, torch.from_numpy(deltas).double(), torch.from_numpy(boxes).double())
        ref = R.apply_deltas_ref(deltas, boxes, *geom)
        assert torch.allclose(torch.from_numpy(ref["out"]), want, rtol=0, atol=1e-12)
        assert (ref["n"] >= np.abs(ref["out"][:, :3]) - 1e-15).all()


def test_stage_tail_ref_is_the_module_chain():
    params, boxes = R.stage_tail_inputs(35, 256, 2, 1, 5, 9, seed=6)
    ref = R.stage_tail_ref(params, boxes, R.GEOM)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = d(params["obj"])
    x = F.layer_norm(x + F.linear(F.relu(F.linear(x, d(params["w1"]), d(params["b1"]))), d(params["w2"]), d(params["b2"])), (128,),
                     d(params["n3"][0]), d(params["n3"][1]), params["n3"][2])
    assert torch.allclose(d(ref["obj_out"]), x, rtol=0, atol=1e-12)
    c, r = x, x
    for l, (W, g, b) in enumerate(params["cls"]):
        c = F.relu(F.layer_norm(F.linear(c, d(W)), (128,), d(g), d(b), params["eps_cls"][l]))
    for l, (W, g, b) in enumerate(params["reg"]):
        r = F.relu(F.layer_norm(F.linear(r, d(W)), (128,), d(g), d(b), params["eps_reg"][l]))
    assert torch.allclose(d(ref["logits"]), F.linear(c, d(params["wl"]), d(params["bl"])), rtol=0, atol=1e-12)
    deltas = F.linear(r, d(params["wd"]), d(params["bd"]))
    assert torch.allclose(d(ref["deltas"]), deltas, rtol=0, atol=1e-12)
    assert np.allclose(ref["pred"], R.apply_deltas_ref(deltas.numpy(), boxes, *R.GEOM)["out"], rtol=0, atol=1e-12)
    assert (params["eps_cls"][0], params["eps_reg"][0], params["n3"][2]) == (1e-2, 1e-5, 1e-3)


def test_dpg_mix_ref_is_softmax_sum_sigmoid():
    B, E, P, D, C = 2, 5, 9, 10, 12
    for second in (False, True):
        wl, wi, bw, fw = R.dpg_mix_inputs(B, E, P, D, C, second, False, seed=7)
        ref = R.dpg_mix_ref(wl, wi, bw, fw, B, E, P)
        d = lambda a: torch.from_numpy(a).double()
        w = d(wl).reshape(B, E, P)
        if second:
            w = (w + d(wi).reshape(B, E, P)) / 2
        w = w.softmax(1).unsqueeze(-1)
        rb, rf = (w * d(bw).view(1, E, P, -1)).sum(1), (w * d(fw).view(1, E, P, -1)).sum(1)
        rb[..., :3] = rb[..., :3].sigmoid()
        assert torch.allclose(torch.from_numpy(ref["boxes"]), rb, rtol=0, atol=1e-13)
        assert torch.allclose(torch.from_numpy(ref["feats"]), rf, rtol=0, atol=1e-13)
        assert (ref["mag_f"] >= np.abs(ref["feats"]) - 1e-13).all() and (ref["T"] >= 0).all()


def test_the_stage_tail_tables_cover_the_required_edges():
    c = [v for v in S.TAIL_CASES.values() if v[5] == "asym"]
    assert [v[:5] for v in c] == [(1, 128, (0, 0), 1, 8), (31, 256, (0, 3), 3, 10), (32, 384, (4, 0), 10, 11), (33, 512, (1, 4), 31, 32),
                                  (37, 512, (2, 3), 10, 10), (65, 384, (4, 4), 32, 8), (200, 512, (2, 3), 10, 10), (200, 256, (1, 1), 32, 32)]
    assert all(v[6] == (True, False) for v in c) and len(S.TAIL_RUNS) == 16 + 1        # both FFN forms; the shipped geometry once
    assert {v[1] // 128 for v in c} == {1, 2, 3, 4}                                    # the slice sum: 1, 2, 3 single rounds, one round of four
    assert any(v[2][0] == 0 < v[2][1] for v in c) and any(v[2][1] == 0 < v[2][0] for v in c) and (0, 0) in {v[2] for v in c}
    assert {v[3] for v in c} >= {1, 31, 32} and {v[4] for v in c} >= {8, 11, 32} and {v[0] for v in c} >= {1, 31, 32, 33, 65}
    seeds = [list(S.TAIL_CASES).index(n) + 701 for n, v in S.TAIL_CASES.items() if v[0] >= 31 and v[5] == "asym"]
    assert {s % 2 for s in seeds} == {0, 1}                                            # both planted triples of size deltas
    assert {(v[0], v[1]) for v in S.AD_CASES.values() if v[2] == "asym"} == {(r, dd) for r in (1, 127, 128, 129, 300) for dd in (8, 10, 11, 32)}
    assert sum(v[2] == "shipped" for v in S.AD_CASES.values()) == 1
    assert list(S.DPG_CASES.values()) == [(1, 1, 1, 3, 1, False, False), (3, 3, 7, 10, 118, True, False), (1, 4, 7, 10, 119, False, False),
                                          (2, 4, 200, 10, 128, True, False), (1, 16, 33, 11, 300, True, False), (3, 16, 7, 8, 256, True, True)]


def test_the_planted_rows_sit_on_their_edges():
    """ds below, on, one float32 above and far above the clamp, ds = -20; centres on lo, on lo + ext and beyond each; log sizes -2 and 2."""
    for geom in (R.GEOM, R.GEOM_SHIPPED):
        w, lo, ext, clamp = R.geom64(geom)
        deltas, boxes = R.apply_deltas_inputs(300, 10, geom, seed=8)
        ref = R.apply_deltas_ref(deltas, boxes, *geom)
        dsA, dsB = deltas[-1, 3:6] / w[3:], deltas[-2, 3:6] / w[3:]
        assert dsA[0] < clamp and dsA[1] == clamp and dsA[2] == float(np.nextafter(np.float32(clamp), np.float32(np.inf)))
        assert dsB[0] == -20.0 and dsB[1] == 50.0 and 0 < dsB[2] < clamp
        n = (boxes[:, :3].astype(np.float64) - lo) / ext
        assert n[-1, 0] == 0.0 and n[-1, 1] == 1.0 and n[-1, 2] < 0 and n[-2, 0] > 1 and n[-2, 2] == 0.0
        assert (ref["out"][-1, :3] == [0, 1, 0]).all() and ref["out"][-2, 0] == 1 and ref["out"][-2, 2] == 0
        assert set(boxes[-2:, 3:5].ravel()) == {-2.0, 2.0}
    for name, (Rr, F_, towers, ncls, Dd, geom, _) in S.TAIL_CASES.items():
        if Rr < 31:
            continue
        params, boxes, g, ref = S.tail_reference(name)
        w, lo, ext, clamp = R.geom64(g)
        ds = ref["deltas"][:, 3:6] / w[3:]
        assert (ds == ds[0]).all() and (ref["deltas"][:, 1] == 0).all()               # zeroed head rows: the planted delta in every row
        even = (list(S.TAIL_CASES).index(name) + 701) % 2 == 0
        up = float(np.nextafter(np.float32(clamp), np.float32(np.inf)))
        assert list(ds[0]) == ([50.0, clamp, up] if even else [float(np.float32(0.9) * np.float32(clamp)), 50.0, -20.0])
        n = (ref["ad"]["ctr"] * np.sign(boxes[:, :3]) - lo)[:, 1] / ext[1]            # ctr_y = the box's y
        assert n[-1] == 0.0 and n[-2] == 1.0 and n[-3] < 0 and n[-4] > 1
        assert ref["pred"][-1, 0] == 0.0 and ref["pred"][-2, 0] == 1.0                 # x far outside, through a live head row


@pytest.mark.parametrize("name,split", S.TAIL_RUNS)
def test_stage_tail_bound_is_tight_enough(name, split):
    _, _, _, ref = S.tail_reference(name)
    bd = S.tail_bound(name, split)
    worst = {"obj_out": bd["obj_out"].max() / np.abs(ref["obj_out"]).max(), "logits": bd["logits"].max() / np.abs(ref["logits"]).max(),
             "deltas": bd["deltas"].max() / np.abs(ref["deltas"]).max(),
             "pred centres": bd["pred"][:, :3].max() / 1.0,                            # columns 0..2 are in [0, 1]: judged against 1
             "pred rest": bd["pred"][:, 3:].max() / np.abs(ref["pred"][:, 3:]).max()}
    print(f"{name} {'split' if split else 'in line'}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < 1e-3, worst
    assert np.abs(ref["obj_out"]).max() > 0.25 and np.abs(ref["logits"]).max() > 0.25
    for step in [ref["ffn"]["ln2"]] + [s["ln1"] for s in ref["cls"] + ref["reg"]]:
        var = step["s"] ** 2
        assert 0.05 < var.min() and var.max() < 50


@pytest.mark.parametrize("name", list(S.TAIL_CASES))
def test_stage_tail_mutations_exceed_the_bound(name):
    Rr, F_, (n_cls, n_reg), ncls, Dd, geom, forms = S.TAIL_CASES[name]
    params, boxes, g, ref = S.tail_reference(name)
    planted = slice(Rr - 4, Rr)
    # (mutation, applies, the output it must show in, the rows it is judged on)
    table = [("ffn_slice", F_ >= 256, "obj_out", None), ("no_residual", True, "obj_out", None), ("no_b2", True, "obj_out", None),
             ("unbiased", True, "obj_out", None), ("tower_ln", n_cls > 0 and n_reg > 0, "logits", None),
             ("eps_swapped", n_cls + n_reg > 0, "logits" if n_cls else "pred", None),
             ("tower_relu", n_cls + n_reg > 0, "logits" if n_cls else "pred", None), ("head_col", ncls > 1, "logits", None),
             ("tail_row", Rr >= 34, "obj_out", slice(32, 64)), ("tail_row", Rr >= 34, "logits", slice(32, 64)),
             ("tail_row", Rr >= 34, "pred", slice(32, 64)),
             ("row_shift", Rr > 1, "pred", None), ("weights_swapped", geom == "asym", "pred", None), ("axis", geom == "asym", "pred", None),
             ("no_clamp", Rr >= 31, "pred", planted), ("no_clip", Rr >= 31, "pred", planted)]
    for split in forms:
        bd = S.tail_bound(name, split)
        for m, applies, key, rows in table:
            if applies:
                mut = R.stage_tail_ref(params, boxes, g, mutate=m)
                rows = slice(None) if rows is None else rows
                assert exceeds(mut[key][rows], ref[key][rows], bd[key][rows]), (name, split, m, key)
    assert len(table) - 2 == len(R.TAIL_MUTATIONS)                                      # every mutation of the reference is in the table


@pytest.mark.parametrize("name", list(S.AD_CASES))
def test_apply_deltas_bound_is_tight_enough_and_mutations_exceed_it(name):
    Rr, Dd, geom = S.AD_CASES[name]
    deltas, boxes, g, ref = S.ad_reference(name)
    bd = S.ad_bound(ref, 0.0)
    assert bd[:, :3].max() < 1e-3 and bd[:, 3:6].max() < 1e-3 * np.abs(ref["out"][:, 3:6]).max() and (bd[:, 6:] == 0).all()
    planted = slice(max(Rr - 2, 0), Rr)
    muts = [("row_shift", slice(None))] if Rr > 1 else []
    muts += [("weights_swapped", slice(None))] if geom == "asym" else []
    muts += [("axis", slice(None))] if geom == "asym" and Rr > 1 else []           # R == 1 is a planted row: its y is on or beyond an edge of both axes
    A_row = Rr >= 2 or (list(S.AD_CASES).index(name) + 901) % 2 == 0
    muts += [("no_clip", planted)] + ([("no_clamp", planted)] if Rr >= 2 or not A_row else [])     # ds = 50 is in planted row B
    for m, rows in muts:
        mut = R.apply_deltas_ref(deltas, boxes, *g, mutate=m)["out"]
        assert exceeds(mut[rows], ref["out"][rows], bd[rows]), (name, m)


@pytest.mark.parametrize("name", list(S.DPG_CASES))
def test_dpg_mix_bound_is_tight_enough_and_mutations_exceed_it(name):
    B, E, P, D, C, second, wide = S.DPG_CASES[name]
    (wl, wi, bw, fw), ref = S.dpg_reference(name)
    bb, bf = S.dpg_bound(name)
    worst = max(bb[..., :3].max(), bb[..., 3:].max() / max(np.abs(ref["boxes"][..., 3:]).max(), 1e-300) if D > 3 else 0.0,
                bf.max() / np.abs(ref["feats"]).max())
    print(f"{name}: T {ref['T'].max():.1f}  worst bound / |ref| {worst:.2e}")
    assert worst < 1e-3 and ref["T"].max() <= 60.0 + 1e-3
    if wide:
        assert ref["T"].max() > 59.0
        v = wl.reshape(B, E, P)
        assert np.isinf(v).any() and np.isfinite(v).any(1).all()                       # some expert at -inf, never all of a (b, p)
    muts = (["expert_major"] if E > 1 and P > 1 else []) + (["no_half"] if second else []) + (["sigmoid_cols"] if D > 3 else []) + \
           (["first_expert_twice"] if E > 1 else [])
    for m in muts:
        mut = R.dpg_mix_ref(wl, wi, bw, fw, B, E, P, mutate=m)
        assert exceeds(mut["boxes"], ref["boxes"], bb), (name, m)
        if m != "sigmoid_cols":
            assert exceeds(mut["feats"], ref["feats"], bf), (name, m)
