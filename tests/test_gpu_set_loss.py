"""The decoder losses of a step on the GPU (csrc/setloss.hip, `ops.set_loss`) against their definition in tests/set_loss_ref.py and against the
torch route of `SRFDetHead.loss_ota`.

(a) losses and gradients against the float64 definition, next to the f32 torch route (`loss_classification` / `loss_boxes` on the GPU) on the
    same inputs: per case the kernel's largest error is at most four times the torch route's largest error, and no tighter than one f32 ulp
    of the largest magnitude in that tensor -- the bar of tests/test_gpu_ota.py.  (The kernel computes every element in float64 and
    rounds it once, so its error is about half an ulp of the element; the torch route's is a few.)  Logits of +-30 and +-100 are in every
    case; there float64, not torch f32, is the yardstick and the kernel must stay finite.
(b) the exact pattern of the box gradient, a non-finite stage, out-of-range slots, equal bytes twice and no host synchronisation.
(c) `loss_ota` with SRF_SET_LOSS=1 against SRF_SET_LOSS=0 and against a float64 run of the torch losses on the CPU; unset = 0 bit for bit;
    the reference's recorded losses with the switch on; the launches of the loss stage on both routes."""
import warnings

import numpy as np
import pytest
import torch

import make_fixtures as mf
import make_fixtures_r2 as mf2
import set_loss_ref as R
from srfdet3d_amd import ops
from srfdet3d_amd.plugin import heads, training
from test_fixtures_r2 import check_loss_ota, ota_inputs

pytestmark = pytest.mark.gpu
S, B = 3, 2
KW = dict(alpha=0.25, w_cls=2.0, w_box=0.25)
# (name, P, C, (D, Dw, Dg), boxes of the two samples, matched rows of the two samples (None: a third of the rows), gamma).
# P: 1, 7, 64, 65 (one row past a 64-row tile), 300 (five workgroups a pair); C: 1, 3, 10; G: 0, 1, 5, 17; count = 0 beside count = P three times.
CASES = [("p1", 1, 1, (8, 8, 7), (1, 0), (1, 0), 2.0), ("p7", 7, 3, (10, 10, 9), (5, 17), None, 1.5), ("p64", 64, 10, (8, 8, 7), (17, 1), (64, 0), 2.0),
         ("p65", 65, 10, (10, 10, 9), (0, 5), (0, 65), 2.0), ("p300", 300, 10, (10, 10, 9), (17, 5), None, 2.0),
         ("p300g", 300, 3, (8, 8, 7), (1, 17), None, 1.5)]
_CACHE = {}


def ulp(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def inputs(name):
    """The numpy inputs of a case: `set_loss_ref.case` with saturated logits of +-30 and +-100 on matched and unmatched rows."""
    _, P, C, (D, Dw, Dg), ns, counts, _ = next(c for c in CASES if c[0] == name)
    c = R.case(200 + [x[0] for x in CASES].index(name), S, B, P, C, D, Dw, Dg, ns, counts)
    flat = c["logits"].reshape(S, -1)
    sat = np.array([30.0, -30.0, 100.0, -100.0], np.float32)
    for s in range(1 if P < 4 else S):                      # with fewer than four rows only stage 0: the other stages keep ordinary logits
        for b in range(B):
            k = int(c["count"][s, b])
            rows = list(c["pred_idx"][s, b, :min(k, 2)]) + [0, P - 1]           # matched rows first: their class column is among the C
            for i, p in enumerate(rows):
                c["logits"][s, b, p, :] = np.resize(np.roll(sat, i), C)
    assert flat.shape[1] == B * P * C
    return c


def on_device(c, dev):
    t = lambda k: torch.from_numpy(c[k]).to(dev)
    return dict(args=(t("logits"), t("boxes"), t("count"), t("pred_idx"), t("gt_idx"), t("gt"), t("labels"), t("cw")), num=c["num"].tolist())


def run_kernel(c, dev, gamma):
    d = on_device(c, dev)
    return [x.cpu().numpy() for x in ops.set_loss(*d["args"], d["num"], KW["alpha"], gamma, KW["w_cls"], KW["w_box"])]


def case(name, dev):
    """Inputs, the kernel's result, the float64 definition and the f32 torch route of a case, computed once and left unchanged."""
    if name not in _CACHE:
        gamma = next(c for c in CASES if c[0] == name)[6]
        c = inputs(name)
        _CACHE[name] = dict(c=c, gamma=gamma, got=run_kernel(c, dev, gamma), ref=R.ref(c, gamma=gamma, **KW),
                            torch=R.torch_route(c, gamma=gamma, dtype=torch.float32, device=dev, **KW))
    return _CACHE[name]


def hold_to_float64(tag, got, torch32, ref):
    """The 4 x / one-ulp bar on (loss, grad_logits, grad_boxes); prints the figures first.  -> the three ratios kernel / torch."""
    ratios = []
    for what, x, t, r in zip(("loss", "grad_logits", "grad_boxes"), got, torch32, ref):
        assert x.dtype == np.float32 and np.isfinite(x).all(), (tag, what)
        e_k = float(np.abs(x.astype(np.float64) - r).max())
        e_t = np.abs(t.astype(np.float64) - r).max()
        e_t = float("inf") if not np.isfinite(e_t) else float(e_t)             # a torch route that lost a value sets no bar
        floor = ulp(r)
        ratios.append(e_k / max(e_t, 1e-300))
        print(f"set_loss {tag} {what}: error kernel {e_k:.3e}, torch f32 {e_t:.3e}, one ulp of the largest {floor:.3e}, ratio {ratios[-1]:.3g}")
        assert e_k <= max(4 * e_t, floor), (tag, what, e_k, e_t, floor)
    return ratios


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_losses_and_gradients_meet_float64(dev, name):
    k = case(name, dev)
    hold_to_float64(name, k["got"], k["torch"], k["ref"][:3])
    matched, box_rows = k["ref"][3], k["ref"][4]
    gb = k["got"][2]
    Dw = len(k["c"]["cw"])
    assert (gb[~box_rows] == 0).all() and (gb[..., Dw:] == 0).all()
    assert (gb[box_rows][:, :Dw] != 0).all() and np.array_equal(np.sign(gb), np.sign(k["ref"][2]))
    if name in ("p1", "p64", "p65"):                       # count = P beside count = 0
        assert sorted(k["c"]["count"][0].tolist()) == [0, k["c"]["logits"].shape[2]]
        assert matched[0].reshape(B, -1).all(1).tolist() in ([True, False], [False, True])


def pattern_case(dev):
    """P 65, (10, 10, 9): sample 0 has a box with dx = 0, one with dx < 0 and a unit box at yaw 0 whose target is exact in every format;
    the prediction matched to it equals it; code weight 2 is zero."""
    if "pattern" not in _CACHE:
        c = R.case(300, S, B, 65, 10, 10, 10, 9, ns=(6, 5))
        c["gt"][0, 2, 3] = 0.0
        c["gt"][0, 3, 4] = -2.0
        c["gt"][0, 4] = [1.5, -2.25, 0.5, 1.0, 1.0, 1.0, 0.0, 0.75, -1.25]
        c["gt_idx"][:, 0, :6] = np.arange(6)
        c["gt_idx"][:, 0, 6:] = np.where(c["gt_idx"][:, 0, 6:] >= 0, 5, -1)
        c["cw"][2] = 0.0
        exact = int(c["pred_idx"][0, 0, 4])
        c["boxes"][0, 0, exact] = [1.5, -2.25, 0.5, 0.0, 0.0, 0.0, 0.0, 1.0, 0.75, -1.25]
        _CACHE["pattern"] = dict(c=c, exact=exact, got=run_kernel(c, dev, 2.0), ref=R.ref(c, gamma=2.0, **KW), ref32=R.ref(c, gamma=2.0, dtype=np.float32, **KW))
    return _CACHE["pattern"]


def test_exact_pattern_of_the_box_gradient(dev):
    k = pattern_case(dev)
    c, gb, (_, _, gb64, matched, box_rows) = k["c"], k["got"][2], k["ref"]
    assert (matched & ~box_rows).sum() == 2 * S                                  # the rows of dx = 0 and dx < 0: matched, no box loss
    zero = np.ones(gb.shape, bool)
    zero[box_rows] = False                                                        # unmatched rows and rows with a non-finite target
    zero[..., 2] = True                                                           # the zero weight
    zero[0, 0, k["exact"]] = True                                                 # pred == target
    assert box_rows[0, 0, k["exact"]]
    # everywhere else the float64 difference is far from zero, so the sign is decided
    rows = np.argwhere(box_rows)
    for s, b, p in rows:
        g = c["gt_idx"][s, b, list(c["pred_idx"][s, b]).index(p)]
        u = c["gt"][b, g].astype(np.float64)
        tn = np.concatenate([u[:3], np.log(u[3:6]), [np.sin(u[6]), np.cos(u[6])], u[7:]])
        df = c["boxes"][s, b, p].astype(np.float64) - tn
        assert (np.abs(df[~zero[s, b, p]]) > 1e-5).all()
    assert (gb[zero] == 0).all() and (gb[~zero] != 0).all()
    assert np.array_equal(np.sign(gb), np.sign(gb64))
    np.testing.assert_allclose(gb, k["ref32"][2], rtol=2.5e-7, atol=0)           # a constant times a sign


def test_a_non_finite_stage_has_its_nan_to_num_value_and_no_gradient(dev):
    k = pattern_case(dev)
    c = {n: v.copy() for n, v in k["c"].items()}
    c["boxes"][1, 0, c["pred_idx"][1, 0, 0], 1] = np.inf                          # slot 0 -> box 0: a finite target
    loss, gl, gb = run_kernel(c, dev, 2.0)
    assert loss[1, 1] == np.finfo(np.float32).max and not gb[1].any()
    base = k["got"]
    assert np.array_equal(gl, base[1]) and np.array_equal(gb[[0, 2]], base[2][[0, 2]])     # the other stages and the class loss: untouched
    keep = np.ones((S, 2), bool)
    keep[1, 1] = False
    assert np.array_equal(loss[keep], base[0][keep])
    c["logits"][2, 1, 3, 0] = np.nan
    loss, gl, gb = run_kernel(c, dev, 2.0)
    assert loss[2, 0] == 0.0 and not gl[2].any() and np.array_equal(gl[:2], base[1][:2]) and loss[1, 1] == np.finfo(np.float32).max
    ref = R.ref(c, gamma=2.0, **KW)
    assert np.array_equal(ref[0] == np.finfo(np.float32).max, loss == np.finfo(np.float32).max) and ref[0][2, 0] == 0.0
    assert not ref[1][2].any() and not ref[2][1].any()


def test_out_of_range_slots_are_skipped(dev):
    k = case("p65", dev)                                   # sample 0 has no match, sample 1 has count = P
    c = {n: v.copy() for n, v in k["c"].items()}
    P = c["logits"].shape[2]
    c["count"][0, 0], c["pred_idx"][0, 0, :3], c["gt_idx"][0, 0, :3] = 3, [P, -1, 5], [0, 0, 8]      # a row past the end, one before the start, a box at Gpad
    c["count"][1, 0] = P + 5                               # clamped to P, and the slots hold -1
    c["gt_idx"][2, 1, 7] = -1                              # one live slot of a full sample loses its box
    got = run_kernel(c, dev, k["gamma"])
    ref = R.ref(c, gamma=k["gamma"], **KW)
    clean = {n: v.copy() for n, v in k["c"].items()}
    clean["pred_idx"][2, 1, 7:-1], clean["gt_idx"][2, 1, 7:-1] = k["c"]["pred_idx"][2, 1, 8:], k["c"]["gt_idx"][2, 1, 8:]    # the same inputs with the slots removed
    clean["pred_idx"][2, 1, -1] = clean["gt_idx"][2, 1, -1] = -1
    clean["count"][2, 1] = P - 1
    assert not ref[3][0, 0].any() and ref[3][2, 1].sum() == P - 1
    for x, y in zip(ref, R.ref(clean, gamma=k["gamma"], **KW)):
        np.testing.assert_array_equal(x, y)
    hold_to_float64("out-of-range slots", got, R.torch_route(clean, gamma=k["gamma"], dtype=torch.float32, device=dev, **KW), ref[:3])
    for x, y in zip(got, run_kernel(clean, dev, k["gamma"])):
        assert x.tobytes() == y.tobytes()


def test_set_loss_does_not_synchronise_and_repeats_its_bytes(dev):
    k = case("p300", dev)
    d = on_device(k["c"], dev)
    call = lambda: ops.set_loss(*d["args"], d["num"], KW["alpha"], k["gamma"], KW["w_cls"], KW["w_box"])
    call()                                                 # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first, second = call(), call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for x, y, z in zip(first, second, k["got"]):
        assert x.dtype == torch.float32 and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == z.tobytes()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.set_loss(*[a.cpu() for a in d["args"]], d["num"], KW["alpha"], 2.0, KW["w_cls"], KW["w_box"])


def test_more_stages_than_one_pair_of_launches_takes(dev):
    """65 stages: the divisors of 64 travel with a pair of launches, the 65th stage is a second pair."""
    c = R.case(400, 65, 1, 3, 2, 8, 8, 7, ns=(2,))
    c["num"] = (1.0 + np.arange(130, dtype=np.float32).reshape(65, 2))           # every stage its own divisors
    got = run_kernel(c, dev, 2.0)
    hold_to_float64("65 stages", got, R.torch_route(c, gamma=2.0, dtype=torch.float32, device=dev, **KW), R.ref(c, gamma=2.0, **KW)[:3])


# ---- end to end
def head(assigner, dev, dtype=torch.float32):
    hd = object.__new__(heads.SRFDetHead)
    torch.nn.Module.__init__(hd)
    hd.assigner, hd.num_heads, hd.deep_supervision, hd.num_classes, hd.sync_cls_avg_factor = assigner, 6, True, 10, True
    hd.pc_range = mf.NUSC_RANGE
    hd.code_weights = torch.nn.Parameter(torch.tensor([1.0] * 8 + [0.2, 0.2], device=dev, dtype=dtype), requires_grad=False)
    hd.loss_cls = training.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="sum", loss_weight=2.0)
    hd.loss_bbox = training.L1Loss(reduction="sum", loss_weight=0.25)
    return hd


class Fixed:
    """An assigner that hands back a finished assignment."""

    def __init__(self, assigned):
        self.assigned = assigned

    def assign_layers(self, layers, gts, labels):
        return self.assigned


def run_loss_ota(hd, outs, gts, labels):
    """-> losses, leaf gradients, the host synchronisations of `loss_ota`, what the assigner returned"""
    leaves = [{k: v.clone().requires_grad_() for k, v in o.items()} for o in outs]
    kept = {}
    inner = hd.assigner.assign_layers
    hd.assigner.assign_layers = lambda *a: kept.setdefault("assigned", inner(*a))
    if gts[0].is_cuda:
        torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            losses = hd.loss_ota(dict(leaves[0], aux_outputs=leaves[1:]), [mf2._GtBoxes(g) for g in gts], labels)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            del hd.assigner.assign_layers
    syncs = [str(w.message) for w in seen if "called a synchronizing" in str(w.message)]
    sum(losses.values()).backward()
    return losses, [l[k].grad for l in leaves for k in ("pred_boxes", "pred_logits")], syncs, kept["assigned"]


def test_loss_ota_with_the_switch_on(dev, monkeypatch):
    outs, gts, labels = ota_inputs(dev)
    a = training.OTAssignerSRFDet(**mf2.OTA_KW)
    hd = head(a, dev)
    monkeypatch.setenv("SRF_SET_LOSS", "1")
    check_loss_ota(a, outs, gts, labels, rtol=1e-4)        # the reference's recorded numbers, with the switch on
    on, g_on, syncs_on, assigned = run_loss_ota(hd, outs, gts, labels)
    assert training.set_loss_route(hd, outs, assigned, gts)
    monkeypatch.setenv("SRF_SET_LOSS", "0")
    off, g_off, _, _ = run_loss_ota(hd, outs, gts, labels)
    monkeypatch.delenv("SRF_SET_LOSS")
    unset, g_unset, _, _ = run_loss_ota(hd, outs, gts, labels)
    assert list(on) == list(off) == list(unset)            # the same keys in the same order
    for k in off:                                          # unset is off, bit for bit
        assert torch.equal(off[k], unset[k])
    for x, y in zip(g_off, g_unset):
        assert torch.equal(x, y)
    print(f"loss_ota with SRF_SET_LOSS=1: host synchronisations {len(syncs_on)}")
    assert len(syncs_on) == 1, syncs_on                    # the matched counts
    # the yardstick: the torch losses in float64 on the CPU, on the assignment the GPU made
    cpu = [[training.Assigned(x[0].cpu(), x[1].cpu(), x.rows.cpu()) for x in stage] for stage in assigned]
    ref, g_ref, _, _ = run_loss_ota(head(Fixed(cpu), "cpu", torch.float64), [{k: v.double().cpu() for k, v in o.items()} for o in outs],
                                    [g.double().cpu() for g in gts], [l.cpu() for l in labels])
    to64 = lambda t: t.detach().cpu().double().numpy()
    for what, x, t, r in [(k, on[k], off[k], ref[k]) for k in ref] + [(f"leaf gradient {i}", x, t, r) for i, (x, t, r) in enumerate(zip(g_on, g_off, g_ref))]:
        x, t, r = to64(x), to64(t), to64(r)
        e_k, e_t, floor = float(np.abs(x - r).max()), float(np.abs(t - r).max()), ulp(r)
        print(f"loss_ota {what}: error SRF_SET_LOSS=1 {e_k:.3e}, =0 {e_t:.3e}, one ulp {floor:.3e}, ratio {e_k / max(e_t, 1e-300):.3g}")
        assert np.isfinite(x).all() and e_k <= max(4 * e_t, floor), (what, e_k, e_t, floor)


def kernel_count(fn):
    """What one call of fn() runs on the device, by the profiler: kernels and device-to-device copies alike (a `stack` of one tensor is a
    copy, of three a kernel: each is one launch-sized piece of work on the stream).  -> the names"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]


def test_the_launches_of_the_loss_stage_do_not_grow_with_the_stages(dev, monkeypatch):
    outs, gts, labels = ota_inputs(dev)
    a = training.OTAssignerSRFDet(**mf2.OTA_KW)
    hd = head(a, dev)
    counts = {}
    for n_stages in (1, 3):
        for switch in ("1", "0"):
            monkeypatch.setenv("SRF_SET_LOSS", switch)
            leaves = [{k: v.clone().requires_grad_() for k, v in o.items()} for o in outs[:n_stages]]
            layers = [(leaves[0], 6, "")] + [(l, i + 1, f"s.{i}.") for i, l in enumerate(leaves[1:])]
            assigned = a.assign_layers([(o, h) for o, h, _ in layers], gts, labels)
            assert training.set_loss_route(hd, leaves, assigned, gts) == (switch == "1")

            flat = [t for l in leaves for t in l.values()]
            one = torch.ones((), device=dev)

            def loss_stage():                              # autograd.grad: no accumulation into the leaves, which would be a launch per leaf
                values = list(hd.losses_of_assigned(layers, assigned, gts, labels).values())
                torch.autograd.grad(values, flat, [one] * len(values))

            counts[n_stages, switch] = kernel_count(loss_stage)
    print(f"loss stage, forward and backward, launches on the device: SRF_SET_LOSS=1 {len(counts[1, '1'])} (S = 1) / {len(counts[3, '1'])} (S = 3); "
          f"SRF_SET_LOSS=0 {len(counts[1, '0'])} / {len(counts[3, '0'])}")
    for n_stages in (1, 3):
        print(f"SRF_SET_LOSS=1, S = {n_stages}:", [n.replace("void at::native::", "").replace("(anonymous namespace)::", "")[:40] for n in counts[n_stages, "1"]])
    assert len(counts[1, "1"]) > 0 and len(counts[1, "1"]) == len(counts[3, "1"])
    assert sum("srf_set_loss" in n for n in counts[3, "1"]) == 2
