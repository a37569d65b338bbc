"""Times the encoder of the dynamic-voxelization configs on its HIP route (`srf_dvfe_fwd`, csrc/dvfe.hip: two launches behind the voxel
map) against the route it took before (SRF_DVFE=0: `plugin/voxel_encoders.py` op by op in torch, with `srf_scatter_reduce` for the three
reduces), in one process, the routes alternated.

Stage mode (default), one row per sweep of `srfdet3d_amd/synthetic.py` through the encoder of its config:
  waymo   180 000 points   srfdet_dvoxel_waymo_L   (two layers, nf = 5)
  kitti    17 000 points   srfdet_voxel_kitti_L    (one layer,  nf = 4)
  nusc     30 000 points   srfdet_dvoxel_nusc_L    (two layers, nf = 5)
The encoder is timed BEHIND the voxel map (the map is cached on the coordinate tensor, so every timed call finds it); the map itself
(`ops.VoxelMap`, with its one read-back) is timed beside it.  Per route also: kernel launches of one call (torch profiler; null when the
profiler reports none) and the peak of allocated device memory over one call above what was allocated before it.
Per stage: warm-up of both routes, then `--repeats` alternated windows of >= `--window` seconds per route, device events around each window.
The first row, `tanh`, is T: twice the worst error of `torch.tanh` on this GPU, in float32 ulps against float64, over every argument the
position encoders of the three sweeps take a tanh at (at least 1): what tests/test_gpu_dvfe.py allows the kernel per tanh.

Frame mode (--frame): frames/s of srfdet_dvoxel_waymo_L and srfdet_voxel_kitti_L (num_proposals = 200, the sweeps of bench.py) through
`enable_hip_graphs()`, host clock, both routes alternated, one model copy (and so one set of captured graphs) per route.

  python tools/bench_dvfe.py [--stages | --frame] [--out profiles/dvfe_bench.json]      # neither flag: the stages, then the frames
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import ops, synthetic as S, workloads  # noqa: E402

SWEEPS = [("waymo", "srfdet_dvoxel_waymo_L", "waymo_sweep", 5000, 180000), ("kitti", "srfdet_voxel_kitti_L", "kitti_sweep", 1000, 17000),
          ("nusc", "srfdet_dvoxel_nusc_L", "nuscenes_sweep", 2000, 30000)]


def window(fn, min_s):
    """Mean time of fn() in us over a window of at least min_s seconds (device events around the whole window)."""
    n, total = 4, 0.0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total = e0.elapsed_time(e1) * 1e-3
        if total >= min_s:
            return total / n * 1e6
        n = int(n * max(2.0, 1.2 * min_s / max(total, 1e-6)))


def route(on):
    if on:
        os.environ.pop("SRF_DVFE", None)
    else:
        os.environ["SRF_DVFE"] = "0"


def alternate(fns, min_s, repeats, warm=10):
    """name -> [us per call, one per repeat]; `fns` is name -> (route, fn); the routes take turns within every repeat."""
    for on, fn in fns.values():
        route(on)
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (on, fn) in fns.items():
            route(on)
            out[k].append(round(window(fn, min_s), 1))
    route(True)
    return out


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return round(max(v) - min(v), 2)


def randomize_bn(module, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def launches(fn):
    """device kernels of one call, or None when the profiler saw none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def tanh_ulps(args):
    """worst error of torch.tanh on the GPU over float32 `args`, in float32 ulps of the float64 value"""
    true = torch.tanh(args.double().cpu()).numpy()
    got = torch.tanh(args).double().cpu().numpy()
    ulp = np.spacing(np.abs(true).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got - true) / ulp))


def stages(dev, min_s, repeats):
    rows, worst = [], 0.0
    for tag, config, sweep, seed, npts in SWEEPS:
        torch.manual_seed(0)
        model = workloads.build(config, 200).eval()
        randomize_bn(model)
        enc = model.pts_voxel_encoder.to(dev)
        with torch.no_grad():
            pts = torch.from_numpy(getattr(S, sweep)(seed, npts)).to(dev)
            p, coors = model.voxelize([pts])
            c32 = coors.int().contiguous()
            grid = enc.cluster_scatter.grid_zyx
            route(True)
            a, vc = enc(p, coors)                      # builds the voxel map and leaves it on `coors`
            route(False)
            seen = []
            hooks = [m.register_forward_pre_hook(lambda _m, x: seen.append(x[0].detach().float().flatten()))
                     for m in enc.cen2point_pos_enc if isinstance(m, torch.nn.Tanh)]
            b, _ = enc(p, coors)
            for h in hooks:
                h.remove()
            worst = max(worst, tanh_ulps(torch.cat(seen)))
            diff = ((a - b).abs().max() / b.abs().max()).item()
            call = lambda: enc(p, coors)
            extra = {}
            for name, on in (("hip", True), ("torch", False)):
                route(on)
                extra[name] = dict(launches=launches(call), peak_bytes=peak_bytes(call))
            t = alternate({"hip": (True, call), "torch": (False, call), "map": (True, lambda: ops.VoxelMap(c32, grid, 1))}, min_s, repeats)
        rows.append(dict(stage=f"encoder ({tag})", config=config, points=int(p.shape[0]), voxels=int(vc.shape[0]),
                         layers=[v.linear.out_features for v in enc.vfe_layers], hip_us=t["hip"], torch_us=t["torch"], voxel_map_us=t["map"],
                         speedup=[round(y / x, 1) for x, y in zip(t["hip"], t["torch"])],
                         spread_us=dict(hip=spread(t["hip"]), torch=spread(t["torch"])), launches=dict(hip=extra["hip"]["launches"],
                                                                                                       torch=extra["torch"]["launches"]),
                         peak_bytes=dict(hip=extra["hip"]["peak_bytes"], torch=extra["torch"]["peak_bytes"]),
                         routes_max_diff_over_max=float(f"{diff:.3e}"), window_s=min_s,
                         timer="device events around windows of whole calls, the voxel map already on the coordinate tensor"))
    yield dict(stage="tanh", worst_torch_tanh_error_ulp=round(worst, 4), T=round(max(1.0, 2.0 * worst), 4),
               note="T = max(1, 2 x worst float32-ulp error of torch.tanh on this GPU against float64) over the tanh arguments of the three sweeps")
    yield from rows


def frame(config, sweep, seed, npts, dev, min_s, repeats):
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    model = workloads.build(config, 200).eval()
    randomize_bn(model)
    model = model.to(dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    pts = torch.from_numpy(getattr(S, sweep)(seed, npts)).to(dev)
    with torch.no_grad():
        models = {}
        for name, on in (("hip", True), ("torch", False)):
            route(on)
            graphed = copy.deepcopy(model).enable_hip_graphs()
            for _ in range(3):
                graphed.simple_test(None, [pts], copy.deepcopy(metas))
            models[name] = graphed
        torch.cuda.synchronize()

        def fps(m, on):
            route(on)
            n, t0 = 0, time.perf_counter()
            while True:
                m.simple_test(None, [pts], copy.deepcopy(metas))
                n += 1
                if n % 4 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= min_s:
                        break
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        out = dict(stage="frame", config=config, num_proposals=200, points=int(pts.shape[0]),
                   whole_frame_graph=bool(getattr(models["hip"], "_graphed_frame", None) is not None), graph_fps_hip=[], graph_fps_torch=[],
                   window_s=min_s, timer="host clock around whole frames (simple_test), device synchronised at both ends",
                   note="torch = SRF_DVFE=0: the frame as it ran before csrc/dvfe.hip; same process, windows alternated")
        for _ in range(repeats):
            out["graph_fps_hip"].append(round(fps(models["hip"], True), 2))
            out["graph_fps_torch"].append(round(fps(models["torch"], False), 2))
        out["speedup"] = [round(a / b, 3) for a, b in zip(out["graph_fps_hip"], out["graph_fps_torch"])]
        out["ms_per_frame"] = dict(hip=round(1e3 / med(out["graph_fps_hip"]), 3), torch=round(1e3 / med(out["graph_fps_torch"]), 3))
        out["spread_fps"] = dict(hip=spread(out["graph_fps_hip"]), torch=spread(out["graph_fps_torch"]))
    route(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", action="store_true", help="the stages only")
    ap.add_argument("--frame", action="store_true", help="the frames only")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dvfe.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = [dict(stage="box", gpu=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)]

    def gen():
        if not args.frame:
            yield from stages(dev, args.window, args.repeats)
        if not args.stages:
            for tag, config, sweep, seed, npts in SWEEPS[:2]:
                yield frame(config, sweep, seed, npts, dev, max(args.window, 2.0), args.repeats)

    print(json.dumps(lines[0]), flush=True)
    for ln in gen():
        print(json.dumps(ln), flush=True)
        lines.append(ln)
        if args.out:
            with open(args.out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")


if __name__ == "__main__":
    main()
