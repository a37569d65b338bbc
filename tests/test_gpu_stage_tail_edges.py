"""`srf_stage_tail`, `srf_apply_deltas` and `srf_dpg_mix` (csrc/decoder.hip) against the float64 definitions of tests/decoder_ref.py at the
edges of their tilings, on the same float32 inputs cast up, each output held elementwise to a bound counted from the kernel's operation
order (u = 2^-24, gamma(k) = k u / (1 - k u); the build is -fno-fast-math -ffp-contract=off: no product is contracted into an fma; expf
and logf are counted as one ulp, 2 u relative, as tests/test_gpu_attention_edges.py counts them).

Stage tail.  Two kernels and two FFN forms: with a workspace `srf_stage_ffn_k` runs one workgroup per (32 rows, 128 hidden units) and
`srf_stage_tail_k` adds the F / 128 slices in slice order, four at a time and then one at a time (ns = 1, 2, 3, 4 take 1 | 2 | 3 single
rounds | one round of four); without one the tail kernel runs the FFN in line.  Two workgroups per 32-row tile, one per tower; towers of 0
to 4 layers; a head masked to ncls <= 32 / Dd <= 32 columns; the box refinement in the last lines.  TAIL_CASES holds the smallest shapes
that cross each edge (R = 1 | 31 | 32 | 33, three tiles, every F, each tower empty while the other is not, ncls 1 | 31 | 32, Dd 8 | 11 | 32),
each in both forms.  obj_in and boxes_m are the first R rows of NaN-filled buffers, every output the first R rows of a sentinel-filled one,
the workspace exactly as long as asked and NaN-filled (decoder_ref.call_stage_tail).  The bound, step by step:

    hidden     e_h = gamma(128 + 1) (sum |obj| |w1| + |b1|)                 128 terms one after the other on the MFMA, the bias;  ReLU 1-Lipschitz
    FFN        e_f = e_h |W2|^T + gamma(depth + 2) (sum |h| |w2| + |b2| + |obj|)
               split: depth = 128 + F / 128 (a 128-term chain per slice, then the slice adds);  in line: depth = F (one chain through acc2);
               + 2: the bias and the residual
    norm3      layernorm_bound(step, e_f, adds):  split: 8 lanes per row, 16 values per lane and 3 shuffles, adds = 19;
               in line: srf_row_epilogue_regs<2>, 2 values per lane and 6 shuffles, adds = 8                                   -> obj_out
    tower      per layer  e |W|^T + gamma(128) sum |x| |w|,  then layernorm_bound(step, ., 19) (srf_tail_ln_relu_to_image: the 8-lane form);  ReLU
    head       e |W|^T + gamma(128 + 1) (sum |x| |w| + |bias|)                                                              -> logits, deltas
    pred       the refinement below with e = the bound of the deltas

Refinement (`srf_apply_deltas`, and the last lines of the tail), with e the incoming error of a delta (0 stand-alone), q = d / w,
size = expf(b):
    centre     q rounds once, size is one ulp, the product rounds once: gamma(4) |q size|;  + b: u |ctr|
               |d ctr| <= (e / |w|) size + gamma(4) |q size| + u |ctr|
    normalised ctr - lo and the division round once each; ext = hi - lo is formed in float32 on the host, one more u (the reference keeps
               the exact difference):  |d n| <= (|d ctr| + u |ctr - lo|) / ext + gamma(2) |n|;  the clip is 1-Lipschitz and exact at its ends
    log size   ds = d / w rounds once (the clamp is 1-Lipschitz and exact);  expf(ds) one ulp, size one ulp, their product one rounding: 5 u
               relative under the logarithm, so 5 u absolute;  logf one ulp of the result
               |d| <= e / |w| + u |ds| + gamma(5) + gamma(2) |out|
    column 6+  e itself: stand-alone the copy is exact (`torch.equal`)
R in {1, 127, 128, 129, 300} (128 rows per workgroup) x Dd in {8, 10, 11, 32}; the planted rows of decoder_ref.planted_box_rows: ds below,
on, one float32 above and far above the clamp, ds = -20, centres on lo, on lo + ext and beyond each, log sizes -2 and 2.  The geometry is
asymmetric (weights 1.5, 2, 3, 0.5, 1, 4; range -54, -40, -5, 54, 62.4, 3) so that an axis or weight mix-up shows; the shipped values run once.
The fused kernel takes a delta only from its head, so there the exact values are reached per column (bd and a zeroed head row,
decoder_ref.stage_tail_inputs): ds on and one float32 above the clamp in the cases with an even seed, 50 and -20 in those with an odd one,
ds below the clamp from the live head row of column 3 in all of them.

dpg_mix.  One workgroup per (b, p), 128 threads over the C + D output columns; every operation an explicit __f*_rn:
    v = (wl + wi) / 2 rounds once (the halving is exact): u |v|, on the logit and on the maximum: 2 u V, V = max |v|        (with wi only)
    x = v - max rounds once: u T, T = max |v - max v|;  expf one ulp: a term is off by gamma(T + 2 V + 2) relatively, the sum of E of
    them by that and its E - 1 additions, the division rounds once;  w src rounds once, E additions
    |d out| <= gamma(2 T + 4 V [wi] + 2 E + 5) sum_e w |src|
    sigmoid columns 0..2: the incoming error times 1 / 4, plus expf (2 u), the addition and the division: gamma(4) |out|
An expert at -inf has the weight 0 exactly.  Cases: a single expert, C + D = 128 | 129 (the edge of the 128-thread column loop), the
workload, E = 16 (the ABI limit) at C + D = 311, and wide logits (T = 60, one expert at -inf in a few (b, p)).

Conditions on the inputs are checked with the references alone in tests/test_decoder_ref.py: every bound stays below 1e-3 of the largest
|reference| entry of its output and each listed mutation of a reference exceeds it.  The measured max err / bound of every output family
is printed and recorded in DESIGN.md, not asserted beyond <= 1."""
import numpy as np
import pytest
import torch

import decoder_ref as R
from srfdet3d_amd import _lib, ops

pytestmark = pytest.mark.gpu
U = R.U32
SENTINEL = 12345.0

# name: (R, F, (n_cls, n_reg), ncls, Dd, geometry, forms)
TAIL_CASES = {
    "one row, no towers": (1, 128, (0, 0), 1, 8, "asym", (True, False)),
    "last row of a tile missing": (31, 256, (0, 3), 3, 10, "asym", (True, False)),
    "exactly one tile": (32, 384, (4, 0), 10, 11, "asym", (True, False)),
    "one row into the second tile": (33, 512, (1, 4), 31, 32, "asym", (True, False)),
    "workload-like, odd": (37, 512, (2, 3), 10, 10, "asym", (True, False)),
    "three tiles, deepest": (65, 384, (4, 4), 32, 8, "asym", (True, False)),
    "nuScenes stage": (200, 512, (2, 3), 10, 10, "asym", (True, False)),
    "widest heads": (200, 256, (1, 1), 32, 32, "asym", (True, False)),
    "nuScenes stage, shipped geometry": (200, 512, (2, 3), 10, 10, "shipped", (True,)),
}
TAIL_RUNS = [(name, split) for name, c in TAIL_CASES.items() for split in c[6]]
GEOMS = {"asym": R.GEOM, "shipped": R.GEOM_SHIPPED}
AD_CASES = {f"r{Rr}_d{Dd}": (Rr, Dd, "asym") for Rr in (1, 127, 128, 129, 300) for Dd in (8, 10, 11, 32)}
AD_CASES["r129_d10_shipped"] = (129, 10, "shipped")
# name: (B, E, P, D, C, second logits, wide)
DPG_CASES = {
    "single expert": (1, 1, 1, 3, 1, False, False),
    "C + D == 128": (3, 3, 7, 10, 118, True, False),
    "C + D == 129": (1, 4, 7, 10, 119, False, False),
    "workload": (2, 4, 200, 10, 128, True, False),
    "widest": (1, 16, 33, 11, 300, True, False),
    "wide logits": (3, 16, 7, 8, 256, True, True),
}
_REF = {}
RATIOS = {}     # output family -> largest err / bound seen in this run (printed, and recorded in DESIGN.md)


def tail_reference(name):
    """(params, boxes, geometry, float64 reference) of a case, computed once and left unchanged."""
    if ("tail", name) not in _REF:
        Rr, F, (n_cls, n_reg), ncls, Dd, geom, _ = TAIL_CASES[name]
        params, boxes = R.stage_tail_inputs(Rr, F, n_cls, n_reg, ncls, Dd, seed=list(TAIL_CASES).index(name) + 701, geom=GEOMS[geom])
        _REF["tail", name] = (params, boxes, GEOMS[geom], R.stage_tail_ref(params, boxes, GEOMS[geom]))
    return _REF["tail", name]


def ad_bound(ad, e):
    """The refinement's bound of the module text; ad = apply_deltas_ref's dict, e (R, Dd) the incoming error of the deltas (or 0.0)."""
    e = np.zeros_like(ad["out"]) + e
    w = ad["w"]
    dctr = e[:, :3] / w[:3] * ad["size"] + R.gamma(4) * ad["qsize"] + U * ad["ctr"]
    dn = (dctr + U * ad["ctr_lo"]) / ad["ext"] + R.gamma(2) * ad["n"]
    dsz = e[:, 3:6] / w[3:] + U * ad["ds"] + R.gamma(5) + R.gamma(2) * np.abs(ad["out"][:, 3:6])
    return np.concatenate((dn, dsz, e[:, 6:]), 1)


def tail_bound(name, split):
    """The elementwise bounds of the module text -> dict(obj_out, logits, deltas, pred)."""
    params, _, _, ref = tail_reference(name)
    A = lambda a: np.abs(np.asarray(a, np.float64))
    F = params["w1"].shape[0]
    e_h = R.gamma(128 + 1) * ref["hid"]["mag"]
    depth = 128 + F // 128 if split else F
    e_f = e_h @ A(params["w2"]).T + R.gamma(depth + 2) * (ref["ffn"]["mag"] + A(params["obj"]))
    e_obj = R.layernorm_bound(ref["ffn"]["ln2"], e_f, 19 if split else 8)

    def tower(layers, steps, head, w_head):
        e = e_obj
        for (W, _, _), step in zip(layers, steps):
            e = R.layernorm_bound(step["ln1"], e @ A(W).T + R.gamma(128) * step["mag"], 19)
        return e @ A(w_head).T + R.gamma(128 + 1) * head["mag"]

    e_logits = tower(params["cls"], ref["cls"], ref["head_cls"], params["wl"])
    e_deltas = tower(params["reg"], ref["reg"], ref["head_reg"], params["wd"])
    return dict(obj_out=e_obj, logits=e_logits, deltas=e_deltas, pred=ad_bound(ref["ad"], e_deltas))


def ad_reference(name):
    if ("ad", name) not in _REF:
        Rr, Dd, geom = AD_CASES[name]
        deltas, boxes = R.apply_deltas_inputs(Rr, Dd, GEOMS[geom], seed=list(AD_CASES).index(name) + 901)
        _REF["ad", name] = (deltas, boxes, GEOMS[geom], R.apply_deltas_ref(deltas, boxes, *GEOMS[geom]))
    return _REF["ad", name]


def dpg_reference(name):
    if ("dpg", name) not in _REF:
        B, E, P, D, C, second, wide = DPG_CASES[name]
        inp = R.dpg_mix_inputs(B, E, P, D, C, second, wide, seed=list(DPG_CASES).index(name) + 1101)
        _REF["dpg", name] = (inp, R.dpg_mix_ref(*inp, B, E, P))
    return _REF["dpg", name]


def dpg_bound(name):
    """-> (bound of boxes (B, P, D), bound of feats (B, P, C))."""
    B, E, P, D, C, second, _ = DPG_CASES[name]
    ref = dpg_reference(name)[1]
    rel = R.gamma(2 * ref["T"] + (4 * ref["V"] if second else 0.0) + 2 * E + 5)[..., None]
    eb = rel * ref["mag_b"]
    eb[..., :3] = eb[..., :3] / 4 + R.gamma(4) * np.abs(ref["boxes"][..., :3])
    return eb, rel * ref["mag_f"]


def _record(kind, name, got, want, bd):
    err = np.abs(got - want)
    ratio = float(np.where(err > 0, err / np.maximum(bd, 1e-300), 0.0).max())     # a bound of 0 (an exact copy) passes only with err == 0
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), ratio)
    print(f"{kind} | {name}: max err {err.max():.3e}  max bound {bd.max():.3e}  max err / bound {ratio:.3f}  (so far {RATIOS[kind]:.3f})")
    return ratio


# ------------------------------------------------------------------------------------------------------------------ stage tail
@pytest.mark.parametrize("name,split", TAIL_RUNS)
def test_stage_tail_within_the_counted_bound(dev, name, split):
    Rr = TAIL_CASES[name][0]
    params, boxes, geom, ref = tail_reference(name)
    bd = tail_bound(name, split)
    d = R.stage_tail_device(params, boxes, dev)
    rc, *outs = R.call_stage_tail(d, geom, split, sentinel=SENTINEL)
    assert rc == 0
    form = "split" if split else "in line"
    ratios = {}
    for key, buf in zip(("obj_out", "logits", "pred"), outs):
        assert (buf[Rr:] == SENTINEL).all(), f"{key}: written beyond row R"
        got = buf[:Rr].double().cpu().numpy()
        assert np.isfinite(got).all(), f"{key}: a read beyond row R reached a result"
        ratios[key] = _record(f"{key} {form}", name, got, ref[key], bd[key])
    assert max(ratios.values()) <= 1.0, ratios
    rc2, *again = R.call_stage_tail(d, geom, split, sentinel=SENTINEL)
    assert rc2 == 0 and all(torch.equal(a, b) for a, b in zip(outs, again)), "a second call returned other bits"


@pytest.mark.parametrize("split", [True, False])
def test_stage_tail_nothing_to_do_writes_nothing(dev, split):
    params, boxes, geom, _ = tail_reference("one row, no towers")
    d = R.stage_tail_device(params, boxes, dev)
    rc, *outs = R.call_stage_tail(d, geom, split, R=0, sentinel=SENTINEL)
    assert rc == 0 and all((o == SENTINEL).all() for o in outs)


# ---------------------------------------------------------------------------------------------------------------- apply_deltas
@pytest.mark.parametrize("name", list(AD_CASES))
def test_apply_deltas_within_the_counted_bound(dev, name):
    Rr, Dd, _ = AD_CASES[name]
    deltas, boxes, geom, ref = ad_reference(name)
    t = lambda a: torch.from_numpy(a).to(dev)           # each as long as its data and no longer
    dt, bt = t(deltas), t(boxes)
    outs = []
    for _ in range(2):
        buf = torch.full((Rr + 3, Dd), SENTINEL, dtype=torch.float32, device=dev)
        rc = _lib.lib().srf_apply_deltas(ops._ptr(dt), ops._ptr(bt), Rr, Dd, _lib.hf(geom[0]), _lib.hf(geom[1]), float(geom[2]), ops._ptr(buf),
                                         ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(buf)
    buf = outs[0]
    assert (buf[Rr:] == SENTINEL).all()
    got = buf[:Rr].double().cpu().numpy()
    assert np.isfinite(got).all()
    assert torch.equal(buf[:Rr, 6:], dt[:, 6:])                                   # the copied columns, exactly
    assert _record("apply_deltas", name, got, ref["out"], ad_bound(ref, 0.0)) <= 1.0
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(ops.apply_deltas(dt, bt, *geom), buf[:Rr])


# --------------------------------------------------------------------------------------------------------------------- dpg_mix
@pytest.mark.parametrize("name", list(DPG_CASES))
def test_dpg_mix_within_the_counted_bound(dev, name):
    B, E, P, D, C, second, wide = DPG_CASES[name]
    (wl, wi, bw, fw), ref = dpg_reference(name)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    wl_t, wi_t, bw_t, fw_t = t(wl), t(wi), t(bw), t(fw)
    outs = []
    for _ in range(2):
        boxes = torch.full((B * P + 3, D), SENTINEL, dtype=torch.float32, device=dev)
        feats = torch.full((B * P + 3, C), SENTINEL, dtype=torch.float32, device=dev)
        rc = _lib.lib().srf_dpg_mix(ops._ptr(wl_t), ops._ptr(wi_t), B, E, P, ops._ptr(bw_t), D, ops._ptr(fw_t), C, ops._ptr(boxes),
                                    ops._ptr(feats), ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((boxes, feats))
    boxes, feats = outs[0]
    assert (boxes[B * P:] == SENTINEL).all() and (feats[B * P:] == SENTINEL).all()
    gb, gf = (a[:B * P].double().cpu().numpy().reshape(B, P, -1) for a in (boxes, feats))
    assert np.isfinite(gb).all() and np.isfinite(gf).all()
    bb, bf = dpg_bound(name)
    kind = "dpg_mix wide" if wide else "dpg_mix"
    assert max(_record(kind + " boxes", name, gb, ref["boxes"], bb), _record(kind + " feats", name, gf, ref["feats"], bf)) <= 1.0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ob, of = ops.dpg_mix(wl_t, wi_t, bw_t, fw_t, E, P)
    assert torch.equal(ob.reshape(B * P, D), boxes[:B * P]) and torch.equal(of.reshape(B * P, C), feats[:B * P])
