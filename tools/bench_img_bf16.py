"""Times the bf16-product mode of the image branch (csrc/gemm_bf16.hip, `nhwc.mfma_dtype`, `SRFDet.img_mfma_dtype`) against the
routes it is an alternative to, in one process, alternating.

Layer mode (default): every distinct (form, shape) pair of the camera branch of srfdet_voxel_nusc_LC (6 x 928 x 1600), taken from
the model itself: one pass of VoVNet-99 + image FPN with `nhwc.conv3x3` / `conv1x1` / `conv_strided` wrapped records each call's
form (3x3 / s1, 3x3 / s2, 1x1 plain / pooled / top-down), shape and how often it occurs per frame.  Each pair then runs on
post-ReLU-like random data (not zeros: bf16 loops clock higher on zeros) with random weights and a random folded BatchNorm + ReLU,
the f32 route (mode off: Winograd F(4,3) / F(2,3), the split GEMM, the f32 conv GEMM) and the bf16 kernel alternated in windows of
>= 0.5 s timed with device events.  One JSON line per pair: us and TFLOP/s (direct-convolution FLOPs of the layer) of both, the
fraction of the 2.5 PFLOP/s dense bf16 peak, bytes moved per launch (activations in + out in f32, weights once), the speed-up, and a
summary line with the per-frame totals weighted by the occurrence counts.

Frame mode (--frame): the LC frame at num_proposals = 200 through enable_hip_graphs(), three routes in one process, alternated:
default f32, img_autocast_dtype = bfloat16 (torch autocast, the reference's auto_fp16 mode), img_mfma_dtype = bfloat16; frames/s of
every repeat.

  python tools/bench_img_bf16.py [--out profiles/img_bf16_layer_bench.json]
  python tools/bench_img_bf16.py --frame [--out profiles/img_bf16_frame_bench.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import nhwc, synthetic as S, workloads  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0
BF16 = torch.bfloat16


def window(fn, min_s):
    """Mean time of fn() in us over a window of at least min_s seconds (device events around the whole window)."""
    n, total = 8, 0.0
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


def camera_layers(dev):
    """The (form, shape) pairs of one camera-branch pass of the LC model, in execution order, with their counts."""
    torch.manual_seed(0)
    model = workloads.build("srfdet_voxel_nusc_LC", 200).eval().to(dev)
    img = torch.from_numpy(S.camera_images(3000)).to(dev)[0]          # (6, 3, 928, 1600)
    seen = {}
    orig = (nhwc.conv3x3, nhwc.conv1x1, nhwc.conv_strided)

    def note(form, x, conv, top=None):
        N, H, W, cin = x.shape
        key = (form, N, H, W, cin, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0],
               tuple(top.shape[1:3]) if top is not None else None)
        seen[key] = seen.get(key, 0) + 1

    def conv3x3(x, conv, bn=None, relu=False, out=None):
        note("conv3x3", x, conv)
        return orig[0](x, conv, bn, relu, out=out)

    def conv1x1(x, conv, bn=None, relu=False, out=None, pool=False, top=None):
        note("conv1x1_pooled" if pool else "conv1x1_topdown" if top is not None else "conv1x1", x, conv, top)
        return orig[1](x, conv, bn, relu, out=out, pool=pool, top=top)

    def conv_strided(x, conv, bn=None, relu=False, out=None):
        note("conv_strided", x, conv)
        return orig[2](x, conv, bn, relu, out=out)

    nhwc.conv3x3, nhwc.conv1x1, nhwc.conv_strided = conv3x3, conv1x1, conv_strided
    try:
        with torch.no_grad():
            feats = model.img_backbone(img)
            model.img_neck(list(feats.values()) if isinstance(feats, dict) else feats)
    finally:
        nhwc.conv3x3, nhwc.conv1x1, nhwc.conv_strided = orig
    del model
    torch.cuda.empty_cache()
    return seen


def layer(key, count, dev, min_s, repeats):
    form, N, H, W, cin, cout, k, stride, pad, top_hw = key
    g = torch.Generator().manual_seed(cin * 7 + cout)
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=False)
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (k * k * cin) ** 0.5)
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    conv, bn = conv.to(dev).eval(), bn.to(dev).eval()
    x = torch.relu(torch.randn(N, H, W, cin, device=dev) * 1.5 + 0.2)          # ~45 % zeros, as behind a ReLU
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty(N, Ho, Wo, cout, device=dev)
    top = torch.randn(N, top_hw[0], top_hw[1], cout, device=dev) if top_hw is not None else None
    if form == "conv3x3":
        fn = lambda: nhwc.conv3x3(x, conv, bn, True, out=y)                      # noqa: E731
    elif form == "conv_strided":
        fn = lambda: nhwc.conv_strided(x, conv, bn, True, out=y)                 # noqa: E731
    else:
        fn = lambda: nhwc.conv1x1(x, conv, bn, True, out=y, pool=form == "conv1x1_pooled", top=top)   # noqa: E731

    def bf():
        with nhwc.mfma_dtype(BF16):
            fn()

    flops = 2.0 * N * Ho * Wo * k * k * cin * cout
    act = 4.0 * N * (H * W * cin + Ho * Wo * cout) + (4.0 * top.numel() if top is not None else 0.0)
    with torch.no_grad():
        routes = []
        with nhwc.mfma_dtype(BF16, routes=routes):
            fn()
        for f in (fn, bf):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t_f32, t_bf = [], []
        for _ in range(repeats):
            t_f32.append(window(fn, min_s))
            t_bf.append(window(bf, min_s))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    tf_f32, tf_bf = flops / med(t_f32) / 1e6, flops / med(t_bf) / 1e6
    return dict(form=form, shape=f"{cin}->{cout} {k}x{k}/s{stride} @{N}x{H}x{W}", per_frame=count, route_in_mode=routes[0]["route"],
                f32_route_us=[round(t, 1) for t in t_f32], bf16_us=[round(t, 1) for t in t_bf],
                speedup=[round(a / b, 3) for a, b in zip(t_f32, t_bf)], flops=flops,
                f32_route_tflops=round(tf_f32, 1), bf16_tflops=round(tf_bf, 1), frac_bf16_peak=round(tf_bf / BF16_PEAK_TFLOPS, 4),
                bytes_f32_route=act + 4.0 * conv.weight.numel(), bytes_bf16=act + 2.0 * conv.weight.numel(),
                window_s=min_s, timer="device events around each window")


def frame(dev, min_s, repeats):
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    model = workloads.build("srfdet_voxel_nusc_LC", 200).eval().to(dev)
    g = torch.Generator().manual_seed(0)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    img = torch.from_numpy(S.camera_images(3000)).to(dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig()])]
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 30000)).to(dev)
    models = {}
    for name in ("f32", "autocast_bf16", "mfma_bf16"):
        m = copy.deepcopy(model)
        if name == "autocast_bf16":
            m.img_autocast_dtype = BF16
        elif name == "mfma_bf16":
            m.img_mfma_dtype = BF16
        m.enable_hip_graphs()
        with torch.no_grad():
            for _ in range(3):
                m.simple_test(img, [pts], copy.deepcopy(metas))
        models[name] = m
    torch.cuda.synchronize()

    def fps(m):
        n, t0 = 0, time.perf_counter()
        with torch.no_grad():
            while True:
                m.simple_test(img, [pts], copy.deepcopy(metas))
                n += 1
                if n % 4 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= min_s:
                        break
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    out = dict(config="srfdet_voxel_nusc_LC", num_proposals=200, images="6 x 928 x 1600", points=int(pts.shape[0]),
               fps={k: [] for k in models}, window_s=min_s,
               timer="host clock around whole frames (simple_test through enable_hip_graphs), device synchronised at both ends",
               note="one process, windows alternated f32 / autocast / mfma per repeat")
    for _ in range(repeats):
        for name, m in models.items():
            out["fps"][name].append(round(fps(m), 2))
    pairs = list(zip(*[out["fps"][k] for k in ("f32", "autocast_bf16", "mfma_bf16")]))
    out["mfma_over_f32"] = [round(c / a, 4) for a, b, c in pairs]
    out["mfma_over_autocast"] = [round(c / b, 4) for a, b, c in pairs]
    out["clears_the_bar"] = all(c > 1.03 * a and c > 1.03 * b for a, b, c in pairs)
    out["bar"] = "img_mfma_dtype beats both other routes by more than 3 % in every alternated repeat"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_img_bf16.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if args.frame:
        lines = [frame(dev, max(args.window, 2.0), args.repeats)]
        print(json.dumps(lines[0]), flush=True)
    else:
        lines = []
        for key, count in camera_layers(dev).items():
            lines.append(layer(key, count, dev, args.window, args.repeats))
            print(json.dumps(lines[-1]), flush=True)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        tot_f32 = sum(med(ln["f32_route_us"]) * ln["per_frame"] for ln in lines)
        tot_bf = sum(med(ln["bf16_us"]) * ln["per_frame"] for ln in lines)
        fl = sum(ln["flops"] * ln["per_frame"] for ln in lines)
        lines.append(dict(summary="all GEMM-shaped layers of one camera-branch pass, medians weighted by per_frame", layers=sum(ln["per_frame"] for ln in lines),
                          f32_routes_ms=round(tot_f32 / 1e3, 3), bf16_ms=round(tot_bf / 1e3, 3), flops=fl,
                          bf16_tflops=round(fl / tot_bf / 1e6, 1), frac_bf16_peak=round(fl / tot_bf / 1e6 / BF16_PEAK_TFLOPS, 4),
                          slower_in_bf16=[ln["shape"] + " " + ln["form"] for ln in lines if med(ln["bf16_us"]) > med(ln["f32_route_us"])]))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
