"""Times the DCNv2 layer (srf_dcnv2_nhwc, csrc/dcn.hip) against the torch route it replaces (SRF_DCN=0), in one process, alternating.

Layer mode (default): the two production shapes of srfdet_dvoxel_waymo_LC (5 cameras at 640 x 960, strides 16 and 32):
x (5, 256, 40, 60) -> 256 and x (5, 512, 20, 30) -> 512, offsets ~ N(0, 2) pixels, random mask logits, a random eval BatchNorm folded
in + ReLU -- what `dense.conv_bn_act` runs for the conv2 of a bottleneck, NCHW in, NCHW out.  Per shape: warm-up, then three
alternated pairs of windows of >= 0.5 s per route, timed with device events; one JSON line per shape with the time per layer of both
routes (every repeat), the kernel alone (ops.dcnv2_nhwc on prepared channels-last operands), FLOPs from the shape (2 M 9 Cin Cout for
the GEMM + 8 M 9 Cin for the blend), TFLOP/s and the fraction of the f32 MFMA peak, and the floor: ops.conv_gemm_nhwc as a plain
3x3 / s1 / p1 convolution on the same tensor (the same GEMM without the gather) with the ratio DCN / plain.

Frame mode (--frame): srfdet_dvoxel_waymo_LC at num_proposals = 200 on a synthetic Waymo sweep with five 640 x 960 images, every
`conv_offset` randomised (its init is zero), eager and through enable_hip_graphs(), frames/s, both routes alternated.  The SRF_DCN=0
frame is what the model ran before the kernel existed.

  python tools/bench_dcn.py [--out profiles/dcn_layer_bench.json]
  python tools/bench_dcn.py --frame [--out profiles/dcn_frame_bench.json]
Kernel time and launch counts: rocprofv3 --kernel-trace --stats -- python tools/bench_dcn.py --once   (a run of its own)
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import dense, derived, ops, synthetic as S, workloads  # noqa: E402
from srfdet3d_amd.compat.dcn import ModulatedDeformConv2dPack  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3
SHAPES = [(5, 256, 40, 60, 256), (5, 512, 20, 30, 512)]


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


def route(on):
    if on:
        os.environ.pop("SRF_DCN", None)
    else:
        os.environ["SRF_DCN"] = "0"


def layer(shape, dev, min_s, repeats, once):
    N, C, H, W, Cout = shape
    g = torch.Generator().manual_seed(C)
    pack = ModulatedDeformConv2dPack(C, Cout, 3, 1, 1, bias=False)
    bn = torch.nn.BatchNorm2d(Cout)
    x = torch.relu(torch.randn(N, C, H, W, generator=g))
    with torch.no_grad():
        # offsets ~ N(0, 2) pixels, mask logits ~ N(0, 1) on this input
        sd = 1.0 / (3 * C ** 0.5 * x.square().mean().sqrt())
        pack.conv_offset.weight.copy_(torch.randn(pack.conv_offset.weight.shape, generator=g) * sd)
        pack.conv_offset.weight[:18] *= 2.0
        bn.running_mean.copy_(torch.randn(Cout, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Cout, generator=g) * 0.1)
    pack, bn, x = pack.to(dev).eval(), bn.to(dev).eval(), x.to(dev)
    M = N * H * W
    flops = 2.0 * M * 9 * C * Cout + 8.0 * M * 9 * C
    with torch.no_grad():
        off_std = pack.conv_offset(x)[:, :18].std().item()
        route(True)
        y_hip = dense.conv_bn_act(pack, bn, True, x)
        route(False)
        y_torch = dense.conv_bn_act(pack, bn, True, x)
        diff = ((y_hip - y_torch).abs().max() / y_torch.abs().max()).item()
        # the kernel alone, and the plain convolution on the same channels-last tensor
        xh = ops.to_channels_last(x).permute(0, 2, 3, 1)
        om = ops.conv_gemm_nhwc(xh, pack._packed("dcn_offset", pack.conv_offset.weight), 27, (3, 3), 1, 1, None, pack.conv_offset.bias)
        pw = pack._packed("dcn", pack.weight)
        scale, shift = derived.fold_bn(bn)
        yk = torch.empty(N, H, W, Cout, device=dev)
        yp = torch.empty(N, H, W, Cout, device=dev)

        def kernel():
            ops.dcnv2_nhwc(xh, om[..., :18], om[..., 18:], pw, Cout, (3, 3), 1, 1, 1, 1, True, scale, shift, True, out=yk)

        def plain():
            ops.conv_gemm_nhwc(xh, pw, Cout, (3, 3), 1, 1, scale, shift, True, out=yp)

        def module():
            dense.conv_bn_act(pack, bn, True, x)

        if once:      # one call of each, for a kernel trace
            route(True)
            module()
            route(False)
            module()
            route(True)
            plain()
            torch.cuda.synchronize()
            return None
        for fn in (kernel, plain):
            for _ in range(20):
                fn()
        for on in (True, False):
            route(on)
            for _ in range(20):
                module()
        torch.cuda.synchronize()
        t_hip, t_torch, t_kernel, t_plain = [], [], [], []
        for _ in range(repeats):
            route(True)
            t_hip.append(window(module, min_s))
            route(False)
            t_torch.append(window(module, min_s))
            route(True)
            t_kernel.append(window(kernel, min_s / 2))
            t_plain.append(window(plain, min_s / 2))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    tf = flops / (med(t_kernel) * 1e-6) / 1e12
    return dict(shape=f"x ({N}, {C}, {H}, {W}) -> {Cout}, 3x3 / s1 / p1, deform_groups 1", offset_std_px=round(off_std, 2),
                hip_route_us=[round(t, 1) for t in t_hip], torch_route_us=[round(t, 1) for t in t_torch],
                speedup=[round(b / a, 2) for a, b in zip(t_hip, t_torch)],
                hip_route_is="to_channels_last + conv_offset (conv_gemm_nhwc) + srf_dcnv2_nhwc (BN + ReLU epilogue) + copy to NCHW",
                torch_route_is="conv_offset (MIOpen) + 9 x (grid_sample, mask multiply, 1x1 conv2d, add) + fused BN / ReLU pass",
                kernel_us=[round(t, 1) for t in t_kernel], plain_conv_gemm_us=[round(t, 1) for t in t_plain],
                dcn_over_plain=round(med(t_kernel) / med(t_plain), 3), flops=flops, kernel_tflops=round(tf, 2),
                frac_f32_mfma_peak=round(tf / F32_MFMA_PEAK_TFLOPS, 4), peak_tflops=F32_MFMA_PEAK_TFLOPS,
                routes_max_diff_over_max=float(f"{diff:.3e}"), window_s=min_s, timer="device events around each window")


def randomize(model, img):
    g = torch.Generator().manual_seed(0)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)

    def hook(mod, args):   # conv_offset ~ N(0, s), s from the layer's own input: offsets of about one pixel
        rms = args[0].square().mean().sqrt().clamp_min(1e-6)
        mod.conv_offset.weight.copy_((torch.randn(mod.conv_offset.weight.shape, generator=g) / (3 * mod.in_channels ** 0.5)).to(rms.device) / rms)

    hooks = [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, ModulatedDeformConv2dPack)]
    with torch.no_grad():
        model.img_backbone(img)
    for h in hooks:
        h.remove()
    return len(hooks)


def frame(dev, min_s, repeats):
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    model = workloads.build("srfdet_dvoxel_waymo_LC", 200).eval().to(dev)
    img = torch.from_numpy(S.camera_images(3000, n_cam=5, h=640, w=960)).to(dev)
    route(False)
    n_dcn = randomize(model, img[0])
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig(n_cam=5, f=1266.0 * 960 / 1600, cx=480.0, cy=320.0)])]
    pts = torch.from_numpy(S.waymo_sweep(5000, 180000)).to(dev)
    models = {}
    for name, on in (("hip", True), ("torch", False)):
        route(on)
        graphed = copy.deepcopy(model).enable_hip_graphs()
        with torch.no_grad():
            for _ in range(3):
                graphed.simple_test(img, [pts], copy.deepcopy(metas))
                model.simple_test(img, [pts], copy.deepcopy(metas))
        models[name] = graphed
    torch.cuda.synchronize()

    def fps(m, on):
        route(on)
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

    out = dict(config="srfdet_dvoxel_waymo_LC", num_proposals=200, images="5 x 640 x 960", points=int(pts.shape[0]), dcn_layers=n_dcn,
               eager_fps_hip=[], eager_fps_torch=[], graph_fps_hip=[], graph_fps_torch=[], window_s=min_s,
               timer="host clock around whole frames (simple_test), device synchronised at both ends",
               note="torch = SRF_DCN=0: the frame as it ran before srf_dcnv2_nhwc; same process, windows alternated")
    for _ in range(repeats):
        out["eager_fps_hip"].append(round(fps(model, True), 2))
        out["eager_fps_torch"].append(round(fps(model, False), 2))
        out["graph_fps_hip"].append(round(fps(models["hip"], True), 2))
        out["graph_fps_torch"].append(round(fps(models["torch"], False), 2))
    route(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--once", action="store_true", help="layer mode: one call per route and shape, no timing (for a kernel trace)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcn.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = [frame(dev, max(args.window, 2.0), args.repeats)] if args.frame else [layer(s, dev, args.window, args.repeats, args.once) for s in SHAPES]
    lines = [ln for ln in lines if ln is not None]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out and lines:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
