"""Times the loss stage of a training step -- the focal and L1 losses of every decoder stage, forward and backward, from finished assignments
on -- on its HIP route (SRF_SET_LOSS=1: `ops.set_loss`, csrc/setloss.hip, one call under one autograd node) against the torch operators
(SRF_SET_LOSS=0, the default: `SRFDetHead.loss_classification` / `loss_boxes`, twelve losses one after the other), in one process, the
routes alternated.

Shapes: config 4's (`srfdet_voxel_nusc_LC`: S = 6 decoder stages, B = 2 samples, P = 900 proposals, C = 10 classes, D = 10, 32 + 38
boxes) and the same at P = 200.  The stage is `SRFDetHead.losses_of_assigned` on the result of one `assign_layers` call, the sum of the
twelve values and `backward()` down to the stages' predictions, with the config's loss settings.  The timer is the host clock around windows
of whole stages with the device synchronised at both ends.  Per route also: device kernels of one stage (torch profiler; null when the
profiler reports none) and its host synchronisations (torch's sync debug mode).

  python tools/bench_set_loss.py [--window 0.5] [--repeats 3] [--out profiles/set_loss_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ota import host_syncs, launches, scene, window  # noqa: E402
from srfdet3d_amd import workloads  # noqa: E402
from srfdet3d_amd.plugin import heads, training  # noqa: E402

SHAPES = [("config 4", 6, 2, 900, (32, 38)), ("P = 200", 6, 2, 200, (32, 38))]


def route(on):
    os.environ["SRF_SET_LOSS"] = "1" if on else "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_set_loss.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    cfg = workloads.model_cfg("srfdet_voxel_nusc_LC")
    head_cfg = cfg.bbox_head
    asg = training.OTAssignerSRFDet(**{k: v for k, v in cfg.train_cfg.assigner.items() if k != "type"})
    hd = object.__new__(heads.SRFDetHead)
    torch.nn.Module.__init__(hd)
    hd.assigner, hd.num_heads, hd.num_classes, hd.sync_cls_avg_factor, hd.pc_range = asg, 6, 10, True, None
    hd.code_weights = torch.nn.Parameter(torch.tensor(list(head_cfg.get("code_weights", [1.0] * 8 + [0.2, 0.2])), device=dev), requires_grad=False)
    hd.loss_cls = training.FocalLoss(**{k: v for k, v in head_cfg.loss_cls.items() if k != "type"})
    hd.loss_bbox = training.L1Loss(**{k: v for k, v in head_cfg.loss_bbox.items() if k != "type"})
    lines = [dict(stage="box", gpu=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip,
                  loss_cls=dict(gamma=hd.loss_cls.gamma, alpha=hd.loss_cls.alpha, reduction=hd.loss_cls.reduction, loss_weight=hd.loss_cls.loss_weight),
                  loss_bbox=dict(reduction=hd.loss_bbox.reduction, loss_weight=hd.loss_bbox.loss_weight))]
    print(json.dumps(lines[0]), flush=True)
    for tag, S, B, P, boxes in SHAPES:
        rng = np.random.default_rng(P)
        samples = [scene(rng, P, n, S, dev) for n in boxes]
        gts, labels = [s[1] for s in samples], [s[2] for s in samples]
        outs = [dict(pred_boxes=torch.from_numpy(np.stack([samples[b][0][s][0] for b in range(B)])).to(dev).requires_grad_(),
                     pred_logits=torch.from_numpy(np.stack([samples[b][0][s][1] for b in range(B)])).to(dev).requires_grad_()) for s in range(S)]
        layers = [(outs[0], S, "")] + [(o, i + 1, f"s.{i}.") for i, o in enumerate(outs[1:])]
        route(True)                                        # assigned with the switch on: the 9-column ground truth travels with it
        assigned = asg.assign_layers([(o, h) for o, h, _ in layers], gts, labels)
        assert training.set_loss_route(hd, outs, assigned, gts), "the HIP route refuses this shape"

        def stage():
            for o in outs:
                o["pred_boxes"].grad = o["pred_logits"].grad = None
            losses = hd.losses_of_assigned(layers, assigned, gts, labels)
            sum(losses.values()).backward()
            return losses

        vals, extra = {}, {}
        for name, r in (("hip", True), ("torch", False)):
            route(r)
            vals[name] = {k: float(v) for k, v in stage().items()}
            extra[name] = dict(launches=launches(stage), host_syncs=host_syncs(stage))
        t = {"hip": [], "torch": []}
        for _ in range(args.repeats):
            for name, r in (("hip", True), ("torch", False)):
                route(r)
                t[name].append(round(window(stage, args.window), 1))
        ln = dict(stage=f"loss stage, forward + backward ({tag})", S=S, B=B, P=P, C=10, D=10, boxes=list(boxes),
                  matched=[int(sum(a[1].numel() for a in x)) for x in assigned], hip_us=t["hip"], torch_us=t["torch"],
                  speedup=[round(y / x, 2) for x, y in zip(t["hip"], t["torch"])],
                  spread_us=dict(hip=round(max(t["hip"]) - min(t["hip"]), 1), torch=round(max(t["torch"]) - min(t["torch"]), 1)),
                  launches=dict(hip=extra["hip"]["launches"], torch=extra["torch"]["launches"]),
                  host_syncs=dict(hip=extra["hip"]["host_syncs"], torch=extra["torch"]["host_syncs"]),
                  largest_relative_difference_of_a_loss=max(abs(vals["hip"][k] - vals["torch"][k]) / max(abs(vals["torch"][k]), 1e-30) for k in vals["hip"]),
                  window_s=args.window, timer="host clock around windows of whole loss stages, device synchronised at both ends")
        print(json.dumps(ln), flush=True)
        lines.append(ln)
        if args.out:
            with open(args.out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")
    os.environ.pop("SRF_SET_LOSS", None)


if __name__ == "__main__":
    main()
