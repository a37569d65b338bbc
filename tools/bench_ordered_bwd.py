"""Times the fixed-order gradient kernels (SRF_DETERMINISTIC=1) against the float-atomic kernels they stand in for, by direct calls of
the entry points in one process, the two routes alternated: device events around windows of at least --window seconds, --repeats times.

  RoI gradient   srf_roi_extract_bwd_ordered against srf_roi_extract_bwd at config 4's shape: bs 2 x 6 cameras x 900 proposals = 10800
                 image RoIs out of `ops.box_rois` on the synthetic camera rig, C = 256, four levels of a 928 x 1600 image at strides
                 4 / 8 / 16 / 32, bin-major output gradient; channels-last and NCHW maps.  The zero-fill of the maps, which both routes
                 need, is not timed.
  sparse wgrad   srf_spconv_bwd_weight_ordered against srf_spconv_bwd_weight over the sparse convolutions of `srfdet_voxel_nusc_L` on a
                 30 k-point sweep and of `srfdet_dvoxel_waymo_L` on the 180 k-point sweep: the (input rows, weights, rulebook) of every
                 layer are taken from one training-mode forward of the model's point branch; a window is all of a model's layers in turn.

Per route: time, launches of one call (torch profiler) and, for the ordered route, the workspace bytes.

  python tools/bench_ordered_bwd.py [--window 0.5] [--repeats 3] [--out profiles/ordered_bwd_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import _lib, ops, synthetic, workloads  # noqa: E402
from srfdet3d_amd._lib import FeatMap  # noqa: E402


def window(fn, min_s):
    """Mean device time of fn() in us over a window of at least min_s seconds (events on the current stream)."""
    n = 2
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1) / 1e3
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
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name and "emset" not in e.name) or None
    except Exception:
        return None


def alternated(routes, min_s, repeats):
    """routes: {name: fn} -> {name: [us per call, one per repeat]}, the routes taking turns."""
    out = {k: [] for k in routes}
    for fn in routes.values():
        fn()
    for _ in range(repeats):
        for k, fn in routes.items():
            out[k].append(round(window(fn, min_s), 1))
    return out


def roi_case(dev, channels_last):
    bs, n_cam, P, C, pooled, sr = 2, 6, 900, 256, 7, 2
    strides, (h, w) = [4, 8, 16, 32], (928, 1600)
    rng = np.random.default_rng(0)
    yaw = rng.uniform(-np.pi, np.pi, (bs, P))
    boxes = np.concatenate([rng.uniform(0, 1, (bs, P, 3)), rng.uniform(np.log(0.4), np.log(6.0), (bs, P, 3)), np.sin(yaw)[..., None],
                            np.cos(yaw)[..., None], rng.standard_normal((bs, P, 2))], -1).astype(np.float32)
    l2i = torch.from_numpy(np.stack([synthetic.camera_rig()] * bs).astype(np.float32)).to(dev)
    _, rois = ops.box_rois(torch.from_numpy(boxes).to(dev), list(synthetic.NUSC_RANGE), [0.075, 0.075, 0.2], mutate_centres=False,
                           want_bev=False, lidar2img=l2i)
    R = rois.shape[0]
    grads = [torch.zeros(bs * n_cam, C, h // s, w // s, device=dev) for s in strides]
    if channels_last:
        grads = [g.contiguous(memory_format=torch.channels_last) for g in grads]
    gout = torch.randn(R, pooled * pooled, C, device=dev)
    L = _lib.lib()
    fm = (FeatMap * 4)(*[ops._featmap(g, 1.0 / s) for g, s in zip(grads, strides)])
    gp = (ctypes.c_void_p * 4)(*[g.data_ptr() for g in grads])
    need = L.srf_roi_extract_bwd_ordered_workspace_bytes(R, pooled, sr)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s3 = (pooled * pooled * C, 1, C)

    def ordered():
        _lib.check(L.srf_roi_extract_bwd_ordered(fm, gp, 4, C, rois.data_ptr(), R, pooled, sr, 56.0, gout.data_ptr(), *s3, ws.data_ptr(), need,
                                                 ops._stream()), "roi_extract_bwd_ordered")

    def atomic():
        _lib.check(L.srf_roi_extract_bwd(fm, gp, 4, C, rois.data_ptr(), R, pooled, sr, 56.0, gout.data_ptr(), *s3, ops._stream()),
                   "roi_extract_bwd")
    return dict(ordered=ordered, atomic=atomic), dict(rois=R, C=C, pooled=pooled, sampling_ratio=sr, records=R * pooled * pooled * sr * sr * 4,
                                                      maps="channels-last" if channels_last else "NCHW", workspace_bytes=need), (grads, gout, ws)


def sparse_layers(name, sweep, dev):
    """(feats, weight, rulebook) of every sparse convolution of the model's point branch, from one training-mode forward."""
    seen = []
    real = ops._SpconvFn

    class Shim:
        @staticmethod
        def apply(feats, weight, nbr, subm):
            seen.append((feats.detach().contiguous(), weight.detach(), nbr))
            return real.apply(feats, weight, nbr, subm)
    model = workloads.build(name, 64, train=True).to(dev).train()
    ops._SpconvFn = Shim
    try:
        model.extract_bev([torch.from_numpy(sweep).to(dev)])
    finally:
        ops._SpconvFn = real
    torch.cuda.synchronize()
    return seen


def sparse_case(name, sweep, dev):
    L = _lib.lib()
    layers, calls, table = sparse_layers(name, sweep, dev), {"ordered": [], "atomic": []}, []
    keep = []
    for f, w, nbr in layers:
        K, Cin, Cout = w.shape
        A_out = nbr.shape[1]
        g = torch.randn(A_out, Cout, device=dev)
        gw = torch.empty(K, Cin, Cout, device=dev)
        need = L.srf_spconv_bwd_weight_ordered_workspace_bytes(A_out, Cin, Cout, K)
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        ld = nbr.stride(0) if A_out > 0 else 0
        keep.append((g, gw, ws))
        calls["ordered"].append(lambda f=f, g=g, nbr=nbr, gw=gw, ws=ws, a=(A_out, Cin, Cout, K, ld, need): _lib.check(
            L.srf_spconv_bwd_weight_ordered(f.data_ptr(), f.shape[0], a[1], g.data_ptr(), a[0], a[2], nbr.data_ptr(), a[4], a[3], gw.data_ptr(),
                                            ws.data_ptr(), a[5], ops._stream()), "spconv_bwd_weight_ordered"))
        calls["atomic"].append(lambda f=f, g=g, nbr=nbr, gw=gw, a=(A_out, Cin, Cout, K, ld): _lib.check(
            L.srf_spconv_bwd_weight(f.data_ptr(), f.shape[0], a[1], g.data_ptr(), a[0], a[2], nbr.data_ptr(), a[4], a[3], gw.data_ptr(),
                                    ops._stream()), "spconv_bwd_weight"))
        table.append(dict(A_in=f.shape[0], A_out=A_out, Cin=Cin, Cout=Cout, K=K, row_ranges=-(-A_out // 2048), workspace_bytes=need))
    routes = {k: (lambda fns=fns: [fn() for fn in fns]) for k, fns in calls.items()}
    return routes, dict(model=name, points=int(sweep.shape[0]), layers=len(layers), workspace_bytes_largest=max(t["workspace_bytes"] for t in table),
                        workspace_bytes_sum=sum(t["workspace_bytes"] for t in table), layer_shapes=table), keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ordered_bwd.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    cases = [("RoI gradient, config 4", lambda: roi_case(dev, True)), ("RoI gradient, config 4", lambda: roi_case(dev, False)),
             ("sparse weight gradient, all layers", lambda: sparse_case("srfdet_voxel_nusc_L", synthetic.nuscenes_sweep(2000, 30000), dev)),
             ("sparse weight gradient, all layers", lambda: sparse_case("srfdet_dvoxel_waymo_L", synthetic.waymo_sweep(5000, 180000), dev))]
    for what, make in cases:
        routes, info, keep = make()
        us = alternated(routes, args.window, args.repeats)
        line = dict(what=what, **info, us_per_call=us, launches={k: launches(fn) for k, fn in routes.items()},
                    spread_us={k: round(max(v) - min(v), 1) for k, v in us.items()},
                    ordered_over_atomic=round(float(np.median(us["ordered"]) / np.median(us["atomic"])), 3))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del routes, keep
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
