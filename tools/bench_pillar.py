"""Times the encoder of the pillar configs on its HIP route (`srf_pillar_vfe`, `srf_pillar_scatter_nhwc`, csrc/pillar.hip) against the route
it took before (SRF_PILLAR=0: `plugin/pillar.py` op by op in torch, `srf_densify` into an NCHW canvas, the transposing copy in front of
SECOND), in one process, the routes alternated.

Stage mode (default), at the configs' capacity of 40000 pillars x 20 points x 5 features -> 64 channels on a 512 x 512 canvas:
  vfe (sweep)   the pillars of a synthetic nuScenes sweep dense enough to fill the capacity (`synthetic.nuscenes_sweep`); the mean number
                of points per pillar is reported
  vfe (full)    every pillar full, n = 20: the worst case of a kernel whose work follows sum(num)
  scatter       PointPillarsScatter alone; the old route once as the module ran it (NCHW canvas) and once with the transposing copy
                `nhwc.second_forward` puts behind it
  front         the frame's front as `extract_bev` runs it on the 30000-point sweep of the frame benchmark: voxelize -> encoder -> scatter ->
                the channels-last canvas SECOND's first layer reads
Per stage: warm-up of both routes, then `--repeats` alternated windows of >= `--window` seconds per route, device events around each
window; one JSON line per stage.  GB/s counts rows * (mean points * nf + Cout) * 4 bytes plus the 20 bytes of count and coordinate.

Frame mode (--frame): frames/s of srfdet_pillar_nusc_L and srfdet_pillar_r50_nusc_LC (num_proposals = 200, the inputs of bench.py)
through `enable_hip_graphs()`, host clock, both routes alternated, one model copy (and so one set of captured graphs) per route.

  python tools/bench_pillar.py [--stages | --frame] [--out profiles/pillar_bench.json]      # neither flag: the stages, then the frames
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import nhwc, ops, synthetic as S, workloads  # noqa: E402

ROWS, P, NF, COUT, GRID = 40000, 20, 5, 64, 512


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
        os.environ.pop("SRF_PILLAR", None)
    else:
        os.environ["SRF_PILLAR"] = "0"


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
    return round(max(v) - min(v), 1)


def stages(dev, min_s, repeats):
    torch.manual_seed(0)
    model = workloads.build("srfdet_pillar_nusc_L", 200).eval().to(dev)
    g = torch.Generator().manual_seed(0)
    for m in model.pts_voxel_encoder.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    enc, mid, vl = model.pts_voxel_encoder, model.pts_middle_encoder, model.pts_voxel_layer
    with torch.no_grad():
        dense_pts = torch.from_numpy(S.nuscenes_sweep(2000, 250000)).to(dev)
        voxels, c3, num, _ = ops.hard_voxelize(dense_pts, vl.voxel_size, vl.point_cloud_range, P, ROWS)
        coors = torch.nn.functional.pad(c3, (1, 0), value=0).contiguous()
        rows = voxels.shape[0]
        full_num = torch.full_like(num, P)
        full_vox = voxels.clone()
        lo = torch.tensor(vl.point_cloud_range[:3], device=dev)
        cell = torch.tensor(vl.voxel_size, device=dev)
        base = lo + coors[:, [3, 2, 1]].float() * cell
        full_vox[:, :, :3] = base[:, None, :] + torch.rand(rows, P, 3, generator=g).to(dev) * cell
        full_vox[:, :, 3] = torch.rand(rows, P, generator=g).to(dev) * 255

        for name, (v, n) in (("vfe (sweep)", (voxels, num)), ("vfe (full)", (full_vox, full_num))):
            route(True)
            a = enc(v, n, coors)
            route(False)
            b = enc(v, n, coors)
            diff = ((a - b).abs().max() / b.abs().max()).item()
            t = alternate({"hip": (True, lambda: enc(v, n, coors)), "torch": (False, lambda: enc(v, n, coors))}, min_s, repeats)
            pts = n.float().mean().item()
            nbytes = rows * ((pts * NF + COUT) * 4 + 20)
            yield dict(stage=name, shape=f"{rows} x {P} x {NF} -> {COUT}", mean_points_per_pillar=round(pts, 2), hip_us=t["hip"],
                       torch_us=t["torch"], speedup=[round(y / x, 1) for x, y in zip(t["hip"], t["torch"])], bytes=int(nbytes),
                       hip_gbs=round(nbytes / med(t["hip"]) / 1e3, 1), routes_max_diff_over_max=float(f"{diff:.3e}"), window_s=min_s)

        feats = enc(voxels, num, coors)
        route(True)
        a = mid(feats, coors, 1)
        route(False)
        b = mid(feats, coors, 1)
        assert nhwc.is_channels_last(a) and not nhwc.is_channels_last(b) and torch.equal(a, b)
        t = alternate({"hip": (True, lambda: mid(feats, coors, 1)), "torch": (False, lambda: mid(feats, coors, 1)),
                       "torch_nhwc": (False, lambda: ops.to_channels_last(mid(feats, coors, 1)))}, min_s, repeats)
        nbytes = 4.0 * (GRID * GRID * COUT + 2 * rows * COUT) + 16 * rows
        yield dict(stage="scatter", shape=f"{rows} x {COUT} -> (1, {COUT}, {GRID}, {GRID})", hip_us=t["hip"], densify_nchw_us=t["torch"],
                   densify_plus_transpose_us=t["torch_nhwc"], speedup=[round(y / x, 1) for x, y in zip(t["hip"], t["torch_nhwc"])],
                   bytes=int(nbytes), hip_gbs=round(nbytes / med(t["hip"]) / 1e3, 1), bit_equal=True, window_s=min_s)

        pts = torch.from_numpy(S.nuscenes_sweep(2000)).to(dev)

        def front():
            x = model.extract_bev([pts])
            return x if nhwc.is_channels_last(x) else ops.to_channels_last(x)
        t = alternate({"hip": (True, front), "torch": (False, front)}, min_s, repeats)
        n_front = int(model.voxelize([pts])[0].shape[0])
        yield dict(stage="front", what="voxelize -> encoder -> scatter -> channels-last canvas", points=int(pts.shape[0]), pillars=n_front,
                   hip_us=t["hip"], torch_us=t["torch"], speedup=[round(y / x, 2) for x, y in zip(t["hip"], t["torch"])],
                   spread_us=dict(hip=spread(t["hip"]), torch=spread(t["torch"])), window_s=min_s)


def frame(config, dev, min_s, repeats):
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    model = workloads.build(config, 200).eval().to(dev)
    use_img = bool(getattr(model, "use_img", False))
    img = torch.from_numpy(S.camera_images(3000)).to(dev) if use_img else None
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig()])]
    pts = torch.from_numpy(S.nuscenes_sweep(2000)).to(dev)
    with torch.no_grad():
        models = {}
        for name, on in (("hip", True), ("torch", False)):
            route(on)
            graphed = copy.deepcopy(model).enable_hip_graphs(img_overlap=True)
            for _ in range(3):
                graphed.simple_test(img, [pts], copy.deepcopy(metas))
            models[name] = graphed
        torch.cuda.synchronize()

        def fps(m, on):
            route(on)
            n, t0 = 0, time.perf_counter()
            while True:
                m.simple_test(img, [pts], copy.deepcopy(metas))
                n += 1
                if n % 4 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= min_s:
                        break
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        out = dict(config=config, num_proposals=200, points=int(pts.shape[0]), images=None if img is None else list(img.shape),
                   graph_fps_hip=[], graph_fps_torch=[], window_s=min_s,
                   timer="host clock around whole frames (simple_test), device synchronised at both ends",
                   note="torch = SRF_PILLAR=0: the frame as it ran before csrc/pillar.hip; same process, windows alternated")
        for _ in range(repeats):
            out["graph_fps_hip"].append(round(fps(models["hip"], True), 2))
            out["graph_fps_torch"].append(round(fps(models["torch"], False), 2))
        out["speedup"] = [round(a / b, 3) for a, b in zip(out["graph_fps_hip"], out["graph_fps_torch"])]
    route(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stages", action="store_true", help="the stages only")
    ap.add_argument("--frame", action="store_true", help="the frames only")
    ap.add_argument("--config", action="append", help="frame mode: the configs to run (default: both)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pillar.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    def gen():
        if not args.frame:
            yield from stages(dev, args.window, args.repeats)
        if not args.stages:
            for c in args.config or ["srfdet_pillar_nusc_L", "srfdet_pillar_r50_nusc_LC"]:
                yield frame(c, dev, max(args.window, 2.0), args.repeats)

    for ln in gen():
        print(json.dumps(ln), flush=True)
        lines.append(ln)
        if args.out:
            with open(args.out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")


if __name__ == "__main__":
    main()
