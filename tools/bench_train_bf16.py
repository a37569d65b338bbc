#!/usr/bin/env python3
"""Times the bf16-product mode of the training convolutions (`train_conv.mfma_dtype`, `SRFDet.train_mfma_dtype`; csrc/wgrad_bf16.hip,
csrc/gemm_bf16.hip) against the f32 routes it is an alternative to, in one process, windows alternated.

--layers (default): the eight trainable layer shapes of config 4 (tools/wgrad_bench.py, profiles/r05_wgrad_bench.txt; bs = 2: 12 camera
images), each in its three directions: the weight gradient on `srf_conv_wgrad_nhwc_bf16` against `srf_conv_wgrad_nhwc`, the forward and
the data gradient on the bf16 GEMMs against today's routes (Winograd F(4,3) for 3x3, the split GEMM for 1x1).  Post-ReLU-like random
data (not zeros: bf16 loops clock higher on zeros).  One JSON row per shape with the microseconds of every alternated repeat;
`wgrad_wins` = the slowest bf16 repeat is faster than the fastest f32 repeat.

--step: config 4 (LC training, bs = 2, np = 900) with the switch off and on, alternated on ONE model: iterations/s of every window and a
torch.profiler kernel table per route.

  python tools/bench_train_bf16.py [--out profiles/train_bf16_layer_bench.json]
  python tools/bench_train_bf16.py --step [--out profiles/train_bf16_step_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import ops, synthetic, train_conv, training, workloads  # noqa: E402
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes  # noqa: E402
from wgrad_bench import SHAPES  # noqa: E402

BF16 = torch.bfloat16


def window(fn, min_s):
    """Mean time of fn() in us over a window of at least min_s seconds (device events around the whole window)."""
    n = 4
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


def layer(what, N, H, W, Cin, Cout, k, dev, min_s, repeats):
    if N * H * W * max(Cin, Cout) * 4 >= (1 << 31):
        N = N // 2
        what += f" (N = {N})"
    g_ = torch.Generator().manual_seed(Cin * 7 + Cout)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g_) * 1.5 + 0.2).to(dev)
    g = (torch.randn(N, H, W, Cout, generator=g_) * 0.05).to(dev)
    w = (torch.randn(Cout, Cin, k, k, generator=g_) / (k * k * Cin) ** 0.5).to(dev)
    s, t = (torch.rand(Cout, generator=g_) + 0.5).to(dev), (torch.randn(Cout, generator=g_) * 0.1).to(dev)
    assert train_conv.bf16_layer_ok(k, N, H, W, Cin, Cout) and ops.conv_wgrad_bf16_supported(g, x, k)
    mode = train_conv.mfma_dtype(BF16)
    lm = train_conv._LayerMode(mode, what, None)
    pairs = dict(wgrad=(lambda: ops.conv_wgrad_nhwc(g, x, k), lambda: ops.conv_wgrad_nhwc_bf16(g, x, k)),
                 fwd=(lambda: train_conv._layer_fwd(x, w, s, t, True), lambda: train_conv._layer_fwd(x, w, s, t, True, bf16=True)),
                 dgrad=(lambda: train_conv._layer_dgrad(g, w), lambda: train_conv._layer_dgrad(g, w, lm)))
    fl = 2.0 * N * H * W * Cin * Cout * k * k
    row = dict(layer=what, shape=f"{Cin}->{Cout} {k}x{k} @{N}x{H}x{W}", gflop=round(fl / 1e9, 1), window_s=min_s,
               timer="device events around each window; f32 and bf16 windows alternated per repeat")
    with torch.no_grad():
        for name, (f32, bf) in pairs.items():
            for f in (f32, bf):
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            t_f, t_b = [], []
            for _ in range(repeats):
                t_f.append(window(f32, min_s))
                t_b.append(window(bf, min_s))
            row[name] = dict(f32_us=[round(v, 1) for v in t_f], bf16_us=[round(v, 1) for v in t_b],
                             speedup=[round(a / b, 3) for a, b in zip(t_f, t_b)], bf16_tflops=round(fl / sorted(t_b)[len(t_b) // 2] / 1e6, 1),
                             bf16_wins=max(t_b) < min(t_f))
    row["wgrad_wins"] = row["wgrad"]["bf16_wins"]
    row["f32_routes"] = dict(wgrad="srf_conv_wgrad_nhwc", fwd="srf_wino43" if k == 3 else "srf_conv1x1_nhwc (split / f32 MFMA by the size rule)",
                             dgrad="as fwd, on the rotated / transposed weight")
    return row


def random_gt(dev, n, rng):
    xy, z = rng.uniform(-45, 45, (n, 2)), rng.uniform(-2.5, 0.0, (n, 1))
    size, yaw, vel = rng.uniform(1.0, 5.0, (n, 3)), rng.uniform(-3.1, 3.1, (n, 1)), rng.normal(0, 1, (n, 2))
    t = torch.tensor(np.concatenate([xy, z, size, yaw, vel], 1), dtype=torch.float32, device=dev)
    return LiDARInstance3DBoxes(t, box_dim=9), torch.from_numpy(rng.integers(0, 10, n)).to(dev)


def kernel_table(step, top=25):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(2):
            step()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.events():
        if ev.device_type.name != "CUDA":
            continue
        r = rows.setdefault(ev.name, [0, 0.0])
        r[0] += 1
        r[1] += ev.device_time_total if hasattr(ev, "device_time_total") else ev.cuda_time_total
    tot = sum(r[1] for r in rows.values())
    return dict(kernel_ms_per_step=round(tot / 2e3, 1),
                top=[dict(kernel=name[:100], calls_per_step=n / 2, ms_per_step=round(us / 2e3, 3)) for name, (n, us) in
                     sorted(rows.items(), key=lambda kv: -kv[1][1])[:top]])


def step_bench(dev, bs, nprop, h, w, iters, repeats):
    torch.manual_seed(0)
    model = workloads.build("srfdet_voxel_nusc_LC", nprop, train=True)
    training.freeze_lidar_components(model)
    model = model.to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=0.01)
    rng = np.random.default_rng(0)
    scale = w / 1600.0
    rig = synthetic.camera_rig(f=1266.0 * scale, cx=816.0 * scale, cy=491.0 * h / 928.0)
    pts = [torch.from_numpy(synthetic.nuscenes_sweep(2000 + i)).to(dev) for i in range(bs)]
    img = torch.cat([torch.from_numpy(synthetic.camera_images(3000 + i, h=h, w=w)) for i in range(bs)], 0).to(dev)
    gts = [random_gt(dev, 20, rng) for _ in range(bs)]
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in rig]) for _ in range(bs)]

    def step():
        losses = model(return_loss=True, img=img, points=pts, img_metas=metas, gt_bboxes_3d=[g[0] for g in gts], gt_labels_3d=[g[1] for g in gts])
        total = sum(losses.values())
        opt.zero_grad(set_to_none=True)
        total.backward()
        torch.nn.utils.clip_grad_norm_(params, 35.0)
        opt.step()

    def its(dtype):
        model.train_mfma_dtype = dtype
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        return iters / (time.perf_counter() - t0)

    for dtype in (None, BF16):          # warm-up of both routes (MIOpen's solver search, the allocator)
        model.train_mfma_dtype = dtype
        for _ in range(3):
            step()
    out = dict(config="srfdet_voxel_nusc_LC training", bs=bs, num_proposals=nprop, image=f"{h}x{w}", iters_per_window=iters,
               timer="host clock around each window of whole steps, device synchronised at both ends; f32 / bf16 windows alternated on one model",
               its_per_s=dict(f32=[], bf16=[]))
    for _ in range(repeats):
        out["its_per_s"]["f32"].append(round(its(None), 3))
        out["its_per_s"]["bf16"].append(round(its(BF16), 3))
    out["bf16_over_f32"] = [round(b / a, 4) for a, b in zip(out["its_per_s"]["f32"], out["its_per_s"]["bf16"])]
    out["clears_the_bar"] = all(r > 1.03 for r in out["bf16_over_f32"])
    out["bar"] = "the mode beats the f32 step by more than 3 % in every alternated pair"
    routes = []
    model.train_mfma_dtype, model.train_mfma_routes = BF16, routes
    step()
    model.train_mfma_routes = None
    out["routes_per_step"] = {f"{d} {r}": sum(1 for x in routes if (x["direction"], x["route"]) == (d, r))
                              for d in ("fwd", "dgrad", "wgrad") for r in ("bf16", "f32")}
    out["kernels"] = {}
    for name, dtype in (("f32", None), ("bf16", BF16)):
        model.train_mfma_dtype = dtype
        out["kernels"][name] = kernel_table(step)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true", help="the default")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--window", type=float, default=0.3, help="--layers: seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8, help="--step: iterations per window")
    ap.add_argument("--bs", type=int, default=2)
    ap.add_argument("--np", type=int, default=900)
    ap.add_argument("--img-hw", default="928x1600")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.step:
        h, w = (int(v) for v in a.img_hw.split("x"))
        out = step_bench(dev, a.bs, a.np, h, w, a.iters, a.repeats)
        print(json.dumps({k: v for k, v in out.items() if k != "kernels"}))
    else:
        out = dict(rows=[layer(*shp, dev, a.window, a.repeats) for shp in SHAPES])
        for r in out["rows"]:
            print(json.dumps(r))
        out["wgrad_wins_on_every_shape"] = all(r["wgrad_wins"] for r in out["rows"])
        print(json.dumps(dict(wgrad_wins_on_every_shape=out["wgrad_wins_on_every_shape"])))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
