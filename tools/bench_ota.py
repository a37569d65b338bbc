"""Times the label-assignment stage of a training step on its HIP route (`ops.ota_assign`, csrc/ota.hip: one call, two launches, for every
decoder stage and sample) against the route it took before (SRF_OTA=0: `plugin/training.py` op by op in torch, once per stage and sample),
in one process, the routes alternated.

Shapes: config 4's (`srfdet_voxel_nusc_LC`: S = 6 decoder stages, B = 2 samples, P = 900 proposals, C = 10 classes, 20-40 boxes per sample)
and the same at P = 200.  The stage is `OTAssignerSRFDet.assign_layers` with the config's assigner settings: stacking the predictions,
padding the ground truth, the call, the one read-back and the index tensors the losses take -- on the torch route the S x B calls of
`single_assigner` that `loss_ota` made before.  It ends in host-known counts on both routes, so the timer is the host clock around windows
of whole calls with the device synchronised at both ends.
Per route also: kernel launches of one call (torch profiler; null when the profiler reports none) and the host synchronisations of one call
(torch's sync debug mode: every device-to-host copy and blocking wait counts one).

  python tools/bench_ota.py [--window 0.5] [--repeats 3] [--out profiles/ota_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import workloads  # noqa: E402
from srfdet3d_amd.plugin import training  # noqa: E402

SHAPES = [("config 4", 6, 2, 900), ("P = 200", 6, 2, 200)]


def route(on):
    if on:
        os.environ.pop("SRF_OTA", None)
    else:
        os.environ["SRF_OTA"] = "0"


def scene(rng, P, n_gt, stages, dev):
    """n_gt car-sized boxes over the range; per stage P predictions: six proposals per box within 0.4 m, the rest background."""
    xy, z = rng.uniform(-50, 50, (n_gt, 2)), rng.uniform(-2.5, -0.5, (n_gt, 1))
    size = rng.uniform([1.5, 3.5, 1.4], [2.2, 5.0, 2.0], (n_gt, 3))
    gt = np.concatenate([xy, z, size, rng.uniform(-np.pi, np.pi, (n_gt, 1)), rng.normal(0, 1, (n_gt, 2))], 1).astype(np.float32)
    labels = rng.integers(0, 10, n_gt)
    outs = []
    for _ in range(stages):
        boxes, logits = np.zeros((P, 10), np.float32), rng.standard_normal((P, 10)).astype(np.float32)
        k = min(P, 6 * n_gt)
        g = gt[np.arange(k) % n_gt]
        c = np.concatenate([g[:, :3] + rng.uniform(-0.4, 0.4, (k, 3)), rng.uniform([-54, -54, -4], [54, 54, 1], (P - k, 3))])
        s = np.concatenate([g[:, 3:6] * np.exp(rng.uniform(-0.1, 0.1, (k, 3))), rng.uniform(0.5, 6, (P - k, 3))])
        y = np.concatenate([g[:, 6] + rng.uniform(-0.1, 0.1, k), rng.uniform(-np.pi, np.pi, P - k)])
        boxes[:, :3], boxes[:, 3:6], boxes[:, 6], boxes[:, 7] = c, np.log(s), np.sin(y), np.cos(y)
        logits[np.arange(k), labels[np.arange(k) % n_gt]] += 3.0
        outs.append((boxes, logits))
    return outs, torch.from_numpy(gt).to(dev), torch.from_numpy(labels).to(dev)


def window(fn, min_s):
    """Mean host time of fn() in us over a window of at least min_s seconds, the device idle at both ends."""
    n = 2
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        if total >= min_s:
            return total / n * 1e6
        n = int(n * max(2.0, 1.2 * min_s / max(total, 1e-6)))


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name and "emset" not in e.name)
        return n or None
    except Exception:
        return None


def host_syncs(fn):
    fn()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum(1 for w in seen if "called a synchronizing" in str(w.message))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ota.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    cfg = workloads.model_cfg("srfdet_voxel_nusc_LC")
    asg = training.OTAssignerSRFDet(**{k: v for k, v in cfg.train_cfg.assigner.items() if k != "type"})
    lines = [dict(stage="box", gpu=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)]
    print(json.dumps(lines[0]), flush=True)
    for tag, S, B, P in SHAPES:
        rng = np.random.default_rng(P)
        samples = [scene(rng, P, int(rng.integers(20, 41)), S, dev) for _ in range(B)]
        gts, labels = [s[1] for s in samples], [s[2] for s in samples]
        layers = [(dict(pred_boxes=torch.from_numpy(np.stack([samples[b][0][s][0] for b in range(B)])).to(dev),
                        pred_logits=torch.from_numpy(np.stack([samples[b][0][s][1] for b in range(B)])).to(dev)), S if s == 0 else s)
                  for s in range(S)]
        call = lambda: asg.assign_layers(layers, gts, labels)
        route(True)
        assert asg.kernel_route(layers, gts, labels)
        on = call()
        route(False)
        off = call()
        same = sum(int(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])) for x, y in zip(on, off) for a, b in zip(x, y))
        extra = {}
        for name, r in (("hip", True), ("torch", False)):
            route(r)
            extra[name] = dict(launches=launches(call), host_syncs=host_syncs(call))
        t = {"hip": [], "torch": []}
        for _ in range(args.repeats):
            for name, r in (("hip", True), ("torch", False)):
                route(r)
                t[name].append(round(window(call, args.window), 1))
        route(True)
        ln = dict(stage=f"assignment ({tag})", S=S, B=B, P=P, C=10, boxes=[int(g.shape[0]) for g in gts], matched=[int(sum(a[1].numel() for a in x)) for x in on],
                  hip_us=t["hip"], torch_us=t["torch"], speedup=[round(y / x, 1) for x, y in zip(t["hip"], t["torch"])],
                  spread_us=dict(hip=round(max(t["hip"]) - min(t["hip"]), 1), torch=round(max(t["torch"]) - min(t["torch"]), 1)),
                  launches=dict(hip=extra["hip"]["launches"], torch=extra["torch"]["launches"]),
                  host_syncs=dict(hip=extra["hip"]["host_syncs"], torch=extra["torch"]["host_syncs"]),
                  pairs_with_equal_assignment=f"{same} of {S * B}", window_s=args.window,
                  timer="host clock around windows of whole assign_layers calls, device synchronised at both ends")
        print(json.dumps(ln), flush=True)
        lines.append(ln)
        if args.out:
            with open(args.out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")


if __name__ == "__main__":
    main()
