#!/usr/bin/env python3
"""Generate tests/golden/decoder_free.npz: the reference's five-stage decoder FREE-RUNNING on a damped, trained-like
fixture (run in the build container only, like make_fixtures.py, whose stand-ins and loader it reuses).

The reference's SRFDetHead is executed where it lies; only what it returns is stored.  Inputs and weights are regenerated
on both sides from names by the rule in detgen.py (free_param, lowpass_map, spread_proposal_boxes).  Unpinned parts are
the same as in make_fixtures.py: the ConvModule stand-in and the oracle's RoIAlign / SingleRoIExtractor.

The white-noise fixtures of make_fixtures.py make the loop chaotic, so they can only be compared stage by stage.  Here
the delta heads are damped, the feature maps are smooth and the proposals are spread over the range and over all four
pyramid levels, so a rounding difference does not grow and the loop can be held to the 1e-4 contract as a whole.

The generator REFUSES to write unless, on the reference's run alone, for every case
  * no BEV or image RoI of any stage lies within --margin (2e-4) of a level boundary in log2(scale / finest_scale);
  * every stage uses all four BEV levels with at least 1 % of the RoIs on the rarest;
  * the largest centre movement between consecutive stages is at least 0.1 m at every stage;
  * at least 3 centre coordinates sit on the [0, 1] clamp, and the samples of a bs = 2 case differ by more than 0.1 m;
  * sensitivity: the reference run again on inputs perturbed at rounding level (feature maps 1e-6 relative, camera
    matrices one float32 epsilon; four independent draws) stays within 5e-5 on the boxes of all five stages and on the
    pre-NMS pair.  This is the one condition that was added after the first run on a GPU, see DESIGN.md ("Free-running
    parity"): a box of tens of metres has corners within a metre of a camera's image plane, where the projected RoI
    moves by thousands of pixels per metre, and such a fixture turns an in-tolerance difference of stage 2 into 3e-4 at
    stage 3 for ANY second implementation.  The CPU gate below does not see it, because oracle/pipeline.py repeats the
    reference's float32 operations in the reference's order;
for each case it tries seed index k = 0, 1, 2, ... (part of every tensor name) and keeps the first that passes.  Then the
CPU gate (tests/test_oracle_pinned.py) is evaluated: oracle/pipeline.head_forward against the reference, boxes within 5e-5
at all five stages, logits within half the GPU tests' tolerance, the pre-NMS pair within 5e-5.  The damping factor is the
largest of detgen.FREE_DAMPINGS for which every case passes both.

usage:  python tests/golden/make_free_fixture.py [--ref /root/reference] [--margin 2e-4] [--out decoder_free.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import detgen  # noqa: E402
from make_fixtures import NUSC_RANGE, STAGE_KW, OraclePooler, install_stand_ins, load_reference  # noqa: E402
from detgen import free_metas, level_stats, repo_head  # noqa: E402

BOX_GATE = 5e-5                       # half the 1e-4 contract: the rest is left to the device arithmetic
LOGIT_GATE = {False: (5e-5, 1e-4), True: (5e-5, 1.5e-4)}   # (rtol, atol): half of the GPU tests' logit tolerances
DECODE_GATE = 5e-5                    # half of the GPU tests' 1e-4 on the pre-NMS boxes and scores
PERTURB = 1e-6                        # relative size of the rounding-level perturbation of the sensitivity gate
PERTURB_DRAWS = 4
MAX_SEEDS = 40
t = torch.from_numpy


def reference_head(head, P, fusion):
    hd = object.__new__(head.SRFDetHead)
    nn.Module.__init__(hd)
    hd.use_img, hd.with_lidar_encoder, hd.with_dpg, hd.deep_supervision, hd.is_kitti = fusion, False, True, True, False
    hd.num_dpg_exp, hd.num_proposals, hd.feat_channels_lidar = detgen.FREE_EXPERTS, P, 128
    hd.lidar_feat_lvls, hd.img_feat_lvls, hd.hidden_dim, hd.feat_channels_img = 4, 4, 128, 256
    hd.grid_size, hd.out_size_factor, hd.pc_range = [1472, 1472, 40], 8, NUSC_RANGE
    hd.code_weights = [1.0] * 8 + [0.2, 0.2]
    hd._build_dynamic_prop_gen()
    if fusion:
        hd.img_convs = nn.ModuleList([nn.Conv2d(256, 128, 3, padding=1) for _ in range(4)])
        hd.head_series_lidar = nn.ModuleList([head.SingleSRFDetHead(use_fusion=True, **STAGE_KW) for _ in range(5)])
    else:
        hd.head_series_lidar = nn.ModuleList([head.SingleSRFDetHeadLiDAR(**STAGE_KW) for _ in range(5)])
    # what get_bboxes reads (srfdet_head.py:1246-1293)
    hd.use_focal_loss, hd.use_fed_loss, hd.use_nms, hd.num_classes = True, False, True, 10

    class _Cfg(dict):
        def __getattr__(self, key):
            try:
                return self[key]
            except KeyError:
                raise AttributeError(key)

    hd.test_cfg = _Cfg(score_thr=0.1, max_per_img=300, post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0])
    return hd.eval()


def perturbed(maps, name, rel=PERTURB):
    """every map times (1 + rel * N(0,1)): what another correct float32 implementation's rounding does to an activation"""
    return [(f.astype(np.float64) * (1.0 + rel * detgen.det(f"{name}{i}", f.shape).astype(np.float64))).astype(np.float32)
            for i, f in enumerate(maps)]


def run_reference(head, case, k, damping, captured, perturb=None):
    P, bs, fusion = detgen.FREE_CASES[case]
    hd = detgen.load_free_params(reference_head(head, P, fusion), detgen.free_prefix(case, k), damping)
    bev, img = detgen.free_inputs(case, k)
    metas = free_metas(bs)
    if perturb is not None:
        pre = f"{detgen.free_prefix(case, k)}perturb{perturb}."
        bev = perturbed(bev, pre + "feat")
        img = perturbed(img, pre + "img") if fusion else None
        for b, m in enumerate(metas):   # the camera matrices by one float32 epsilon: another rounding of the projection
            m["lidar2img"] = perturbed(m["lidar2img"], f"{pre}l2i{b}.", rel=2.0 ** -23)
    hd.roi_extractor_lidar = OraclePooler([8, 16, 32, 64])
    if fusion:
        hd.roi_extractor_img = OraclePooler([4, 8, 16, 32])
    first_in = []
    box_arg = 2 if fusion else 1
    hd.head_series_lidar[0].register_forward_pre_hook(lambda mod, a: first_in.append(a[box_arg].detach().clone().numpy()))
    for m in metas:
        m["box_type_3d"] = captured["box_type"]
    with torch.no_grad():
        logits, boxes = hd([t(f) for f in img] if fusion else None, [t(f) for f in bev], metas)
        captured["boxes"], captured["scores"] = [], []
        hd.get_bboxes(logits, boxes.clone(), metas)
    out = dict(boxes=boxes.numpy(), logits=logits.numpy(),
               dec_boxes=np.stack(captured["boxes"]), dec_scores=np.stack(captured["scores"])[..., :hd.num_classes],
               rois_bev=np.stack(hd.roi_extractor_lidar.rois, 0))
    if fusion:
        out["rois_img"] = np.stack(hd.roi_extractor_img.rois, 0)
    lo = np.asarray(NUSC_RANGE[:3], np.float32)
    ext = np.asarray(NUSC_RANGE[3:], np.float32) - lo
    init_m = first_in[0].copy()
    init_m[..., :3] = init_m[..., :3] * ext + lo
    return out, init_m


def conditions(case, out, init_m, margin):
    """-> (list of violated conditions, meta dict) from the reference's run alone"""
    P, bs, fusion = detgen.FREE_CASES[case]
    bad, meta = [], {}
    margins, bev_levels, img_levels = [], [], []
    for s in range(5):
        cnt, mg = level_stats(out["rois_bev"][s])
        if cnt is None:
            return [f"stage {s + 1}: non-finite BEV RoI"], meta
        bev_levels.append(cnt)
        margins.append(mg)
        if cnt.min() < 0.01 * cnt.sum():
            bad.append(f"stage {s + 1}: BEV levels {cnt.tolist()} (rarest under 1 %)")
        if fusion:
            cnt, mg = level_stats(out["rois_img"][s])
            if cnt is None:
                return [f"stage {s + 1}: non-finite image RoI"], meta
            img_levels.append(cnt)
            margins.append(mg)
    if min(margins) < margin:
        bad.append(f"level margin {min(margins):.3e} < {margin:g}")
    chain = np.concatenate([init_m[None], out["boxes"]], 0)[..., :3]
    move = np.abs(chain[1:] - chain[:-1]).max(axis=(1, 2, 3))
    if move.min() < 0.1:
        bad.append(f"movement per stage {move.tolist()} (under 0.1 m)")
    lo, hi = np.asarray(NUSC_RANGE[:3], np.float32), np.asarray(NUSC_RANGE[3:], np.float32)
    clamped = int(((out["boxes"][..., :3] == lo) | (out["boxes"][..., :3] == hi)).sum())
    if clamped < 3:
        bad.append(f"{clamped} centre coordinates on the clamp")
    if bs > 1:
        apart = float(np.abs(out["boxes"][:, 0] - out["boxes"][:, 1]).max())
        meta["samples_apart"] = np.float32(apart)
        if apart < 0.1:
            bad.append(f"the samples differ by {apart:.3e} m only")
    meta.update(move=move.astype(np.float32), bev_levels=np.stack(bev_levels).astype(np.int32),
                margin=np.float32(min(margins)), clamped=np.int32(clamped))
    if fusion:
        # how much of the behind-camera geometry the case still exercises: image RoIs wider than 1e4 px, and (box, camera) pairs
        # whose eight corners lie on both sides of the camera's image plane, per stage
        from oracle import decoder_oracle as DO
        l2i = np.asarray(free_metas(bs)[0]["lidar2img"], np.float64)            # (n_cam, 4, 4)
        stage_in = np.concatenate([init_m[None], out["boxes"][:-1]], 0)          # centres in metres
        cor = np.stack([DO.corners3d(b) for b in stage_in]).astype(np.float64)   # (5, bs, P, 8, 3)
        depth = np.einsum("ck,sbpnk->scbpn", l2i[:, 2, :3], cor) + l2i[:, 2, 3][None, :, None, None, None]
        meta["img_rois_crossing"] = ((depth.min(-1) <= 1e-5) & (depth.max(-1) > 1e-5)).sum(axis=(1, 2, 3)).astype(np.int32)
        meta["img_rois_wide"] = np.array([int(((r[:, 3] - r[:, 1]) > 1e4).sum()) for r in out["rois_img"]], np.int32)
        meta["img_levels"] = np.stack(img_levels).astype(np.int32)
    return bad, meta


def _gate(fusion, out, boxes, logits, dec_boxes, dec_scores):
    """per-stage max differences of a second run against the reference's arrays, and whether they are within the gate"""
    dbox = np.abs(boxes - out["boxes"]).max(axis=(1, 2, 3))
    dlog = np.abs(logits - out["logits"])
    ddec = np.array([np.abs(dec_boxes - out["dec_boxes"]).max(), np.abs(dec_scores - out["dec_scores"]).max()])
    rtol, atol = LOGIT_GATE[fusion]
    ok = bool(dbox.max() <= BOX_GATE and (dlog <= atol + rtol * np.abs(out["logits"])).all() and ddec.max() <= DECODE_GATE)
    return ok, dbox.astype(np.float32), dlog.max(axis=(1, 2, 3)).astype(np.float32), ddec.astype(np.float32)


def cpu_gate(case, k, damping, out):
    """oracle/pipeline.head_forward free-running (+ the head's decode) against the reference"""
    from oracle import pipeline
    P, bs, fusion = detgen.FREE_CASES[case]
    bev, img = detgen.free_inputs(case, k)
    hd = repo_head(case, k, damping)
    lg, bx = pipeline.head_forward(hd, [t(f) for f in img] if fusion else None, [t(f) for f in bev], free_metas(bs))
    with torch.no_grad():
        sc, dec = hd.decode(lg, bx.clone())
    return _gate(fusion, out, bx.numpy(), lg.numpy(), dec.numpy(), sc.numpy())


def sensitivity_gate(head, case, k, damping, out, captured):
    """The reference against ITSELF with every feature map perturbed by 1e-6 relative and the camera matrices by one
    float32 epsilon (PERTURB_DRAWS independent draws, the worst counts).  The CPU gate cannot see how the
    fixture amplifies rounding, because oracle/pipeline.py follows the reference's float32 operation order almost bit for
    bit; a device kernel legitimately rounds otherwise (fused multiply-add, another summation order).  A fixture that
    turns such a perturbation into more than half the tolerance cannot carry the 1e-4 contract, whatever is compared."""
    worst = None
    for draw in range(PERTURB_DRAWS):
        pert, _ = run_reference(head, case, k, damping, captured, perturb=draw)
        g = _gate(detgen.FREE_CASES[case][2], out, pert["boxes"], pert["logits"], pert["dec_boxes"], pert["dec_scores"])
        worst = g if worst is None else (worst[0] and g[0],) + tuple(np.maximum(a, b) for a, b in zip(worst[1:], g[1:]))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--margin", type=float, default=2e-4)
    ap.add_argument("--out", default=os.path.join(HERE, "decoder_free.npz"))
    ap.add_argument("--dampings", type=float, nargs="*", default=list(detgen.FREE_DAMPINGS))
    args = ap.parse_args()
    install_stand_ins()
    _, head = load_reference(args.ref)
    captured = {}

    class _Boxes:
        def __init__(self, tensor, box_dim=9):
            self.tensor = tensor

        @property
        def bev(self):
            return self.tensor[:, [0, 1, 3, 4, 6]]

    def _nms(b, b_nms, scores, thr, mx, cfg):  # the capture of make_fixtures.py: the tensors handed to the NMS
        captured["boxes"].append(b.clone().numpy())
        captured["scores"].append(scores.clone().numpy())
        return b[:0], scores[:0, 0], scores[:0, 0].long()

    captured["box_type"] = _Boxes
    head.xywhr2xyxyr = lambda x: x
    head.box3d_multiclass_nms = _nms

    for damping in args.dampings:
        npz = {"meta.damping": np.float32(damping), "meta.margin_required": np.float32(args.margin)}
        passed = True
        for case in detgen.FREE_CASES:
            for k in range(MAX_SEEDS):
                out, init_m = run_reference(head, case, k, damping, captured)
                bad, meta = conditions(case, out, init_m, args.margin)
                if not bad:   # the second reference run is only worth its time on a fixture that met the cheap conditions
                    ok_s, sbox, slog, sdec = sensitivity_gate(head, case, k, damping, out, captured)
                    if not ok_s:
                        bad.append(f"sensitivity: perturbed run off by boxes {sbox.tolist()} logits {slog.tolist()} decode {sdec.tolist()}")
                print(f"damping {damping:g} case {case} k={k}: " + ("conditions met" if not bad else "; ".join(bad)), flush=True)
                if not bad:
                    break
            else:
                print(f"damping {damping:g} case {case}: no seed index below {MAX_SEEDS} meets the conditions")
                passed = False
                break
            ok, dbox, dlog, ddec = cpu_gate(case, k, damping, out)
            print(f"  perturbed reference: boxes {sbox.tolist()} logits {slog.tolist()} decode {sdec.tolist()}")
            print(f"  CPU gate: boxes {dbox.tolist()} logits {dlog.tolist()} decode {ddec.tolist()} -> {'ok' if ok else 'FAILS'}",
                  flush=True)
            if not ok:
                passed = False
                break
            meta.update(seed=np.int32(k), cpu_box_diff=dbox, cpu_logit_diff=dlog, cpu_decode_diff=ddec,
                        perturbed_box_diff=sbox, perturbed_logit_diff=slog, perturbed_decode_diff=sdec)
            for key, v in out.items():
                npz[f"{case}.{key}"] = v
            for key, v in meta.items():
                npz[f"meta.{case}.{key}"] = v
        if passed:
            np.savez_compressed(args.out, **npz)
            print("wrote", args.out, os.path.getsize(args.out), "bytes")
            return 0
    print("refused: no damping factor meets the conditions and the CPU gate in every case; nothing written")
    return 1


if __name__ == "__main__":
    sys.exit(main())
