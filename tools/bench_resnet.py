"""Times the bottleneck ResNet image backbones on the channels-last executor (`nhwc.resnet`) against the route they took before it
(every convolution an nn.Conv2d on MIOpen in NCHW, BatchNorm + ReLU as a second pass), in one process, alternating.

Layer mode (default): the layer kinds the executor added, at the shapes of ResNet-50 on six 928 x 1600 views -- the 7x7 / stride 2
stem from the NCHW images (srf_stem_conv7_nchw), the padded max pool (srf_nhwc_maxpool3s2_pad1) and conv3 + bn3 + identity + ReLU of
the first bottleneck of each stage on each of the three GEMM families (srf_conv1x1_nhwc_residual / _direct_residual /
_split_residual; "chosen" is what `ops.conv1x1_nhwc_residual` takes by itself).  The other route is what `compat/resnet.py` runs for
the same layer with the executor off: `dense.conv_bn_act` (+ `torch.relu_(out + identity)`) on NCHW tensors.  Per layer: warm-up of
every route, then `--repeats` alternated windows of >= `--window` seconds per route, device events around each window; one JSON line
per layer.

Frame mode (--frame): srfdet_voxel_r50_nusc_LC (six 928 x 1600 images, the sizes of bench.py) and srfdet_dvoxel_waymo_LC (five
640 x 960 images, the sizes of tools/bench_dcn.py --frame) at num_proposals = 200: the image branch alone (`extract_img_feat`: backbone
+ FPN, device events) and whole frames through `enable_hip_graphs()` (frames/s, host clock), both routes alternated.  The "off" route
switches off `nhwc.resnet` alone, which is what SRF_IMG_NHWC=0 does to the image branch of these models (ResNet through the modules,
the FPN behind it on NCHW tensors) while the BEV half keeps its executor -- the frame as it ran before.

  python tools/bench_resnet.py [--out profiles/resnet_layer_bench.json]
  python tools/bench_resnet.py --frame [--out profiles/resnet_frame_bench.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import dense, derived, nhwc, ops, synthetic as S, workloads  # noqa: E402
from srfdet3d_amd.compat.dcn import ModulatedDeformConv2dPack  # noqa: E402

N_IMG, H_IMG, W_IMG = 6, 928, 1600
# conv3 of the first bottleneck of each stage of ResNet-50 at 6 x 928 x 1600: (K, Cout, H, W)
CONV3 = [(64, 256, 232, 400), (128, 512, 116, 200), (256, 1024, 58, 100), (512, 2048, 29, 50)]
FAMILY_ENV = {"lds": dict(SRF_GEMM_SPLIT="0", SRF_GEMM_DIRECT="0"), "direct": dict(SRF_GEMM_SPLIT="0", SRF_GEMM_DIRECT="1"),
              "split": dict(SRF_GEMM_SPLIT_MIN="1"), "chosen": {}}
_REAL_RESNET = nhwc.resnet


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


def family(name):
    for k in ("SRF_GEMM_SPLIT", "SRF_GEMM_DIRECT", "SRF_GEMM_SPLIT_MIN"):
        os.environ.pop(k, None)
    os.environ.update(FAMILY_ENV[name])


def route(on):
    """The executor for the ResNet (on) or the modules as written (off)."""
    nhwc.resnet = _REAL_RESNET if on else (lambda net, x: None)


def alternate(fns, min_s, repeats, warm=10):
    """name -> [us per call, one per repeat]; `fns` is name -> (setup, fn); the routes take turns within every repeat."""
    for setup, fn in fns.values():
        setup()
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (setup, fn) in fns.items():
            setup()
            out[k].append(round(window(fn, min_s), 1))
    return out


def _bn(c, g):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return bn.eval()


def layers(dev, min_s, repeats):
    g = torch.Generator().manual_seed(0)
    nothing = lambda: None  # noqa: E731
    with torch.no_grad():
        # ---- stem ----
        conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False).to(dev).eval()
        bn = _bn(64, g).to(dev)
        x = torch.randn(N_IMG, 3, H_IMG, W_IMG, generator=g).to(dev)
        scale, shift = derived.fold_bn(bn)
        y = torch.empty(N_IMG, H_IMG // 2, W_IMG // 2, 64, device=dev)
        t = alternate({"hip": (nothing, lambda: ops.stem_conv7_nchw(x, conv.weight, scale, shift, True, out=y)),
                       "torch": (nothing, lambda: dense.conv_bn_act(conv, bn, True, x))}, min_s, repeats)
        fl = 2.0 * 147 * 64 * y.numel() / 64
        nbytes = 4.0 * (x.numel() + y.numel())
        med = sorted(t["hip"])[len(t["hip"]) // 2]
        yield dict(layer="stem", shape=f"({N_IMG}, 3, {H_IMG}, {W_IMG}) -> 64, 7x7 / s2 / p3 + BN + ReLU", hip_us=t["hip"], torch_us=t["torch"],
                   speedup=[round(b / a, 2) for a, b in zip(t["hip"], t["torch"])], hip_is="srf_stem_conv7_nchw (NCHW in, NHWC out)",
                   torch_is="MIOpen conv2d + srf_channel_affine (NCHW in, NCHW out)", flops=fl, hip_tflops=round(fl / med / 1e6, 2),
                   hip_gbs=round(nbytes / med / 1e3, 1), window_s=min_s)
        # ---- pool ----
        pool = torch.nn.MaxPool2d(3, 2, 1)
        yn = dense.conv_bn_act(conv, bn, True, x)
        p = torch.empty(N_IMG, H_IMG // 4, W_IMG // 4, 64, device=dev)
        t = alternate({"hip": (nothing, lambda: ops.nhwc_maxpool3s2_pad1(y, out=p)), "torch": (nothing, lambda: pool(yn))}, min_s, repeats)
        med = sorted(t["hip"])[len(t["hip"]) // 2]
        yield dict(layer="pool", shape=f"({N_IMG}, {H_IMG // 2}, {W_IMG // 2}, 64), 3x3 / s2 / p1", hip_us=t["hip"], torch_us=t["torch"],
                   speedup=[round(b / a, 2) for a, b in zip(t["hip"], t["torch"])], hip_is="srf_nhwc_maxpool3s2_pad1 (NHWC)",
                   torch_is="nn.MaxPool2d (NCHW)", hip_gbs=round(4.0 * (y.numel() + p.numel()) / med / 1e3, 1), window_s=min_s)
        del x, y, yn, p
        # ---- conv3 + bn3 + identity + ReLU ----
        for K, Cout, H, W in CONV3:
            c3 = torch.nn.Conv2d(K, Cout, 1, bias=False).to(dev).eval()
            b3 = _bn(Cout, g).to(dev)
            a = torch.relu(torch.randn(N_IMG, K, H, W, generator=g)).to(dev)
            idt = torch.relu(torch.randn(N_IMG, Cout, H, W, generator=g)).to(dev)
            ah = ops.to_channels_last(a).permute(0, 2, 3, 1)
            ih = ops.to_channels_last(idt).permute(0, 2, 3, 1)
            out = torch.empty(N_IMG, H, W, Cout, device=dev)
            kinds = []
            choose = ops._choose_gemm

            def spy(*args, **kw):
                r = choose(*args, **kw)
                kinds.append(r[0])
                return r
            ops._choose_gemm = spy
            fns = {f: ((lambda f=f: family(f)), (lambda: nhwc.conv1x1_residual(ah, c3, b3, ih, True, out=out))) for f in FAMILY_ENV}
            fns["torch"] = ((lambda: family("chosen")), (lambda: torch.relu_(dense.conv_bn_act(c3, b3, False, a) + idt)))
            family("chosen")
            kinds.clear()
            nhwc.conv1x1_residual(ah, c3, b3, ih, True, out=out)
            chosen = kinds[-1]
            ref = torch.relu_(dense.conv_bn_act(c3, b3, False, a) + idt)
            diff = ((out.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max()).item()
            t = alternate(fns, min_s, repeats)
            ops._choose_gemm = choose
            family("chosen")
            fl = 2.0 * K * Cout * N_IMG * H * W
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            yield dict(layer="conv3 + bn3 + identity + ReLU", shape=f"{K} -> {Cout} @ {N_IMG} x {H} x {W}", chosen_family=chosen,
                       **{f"{k}_us": v for k, v in t.items()}, speedup_chosen=[round(b / a, 2) for a, b in zip(t["chosen"], t["torch"])],
                       tflops={k: round(fl / med[k] / 1e6, 2) for k in FAMILY_ENV}, flops=fl,
                       torch_is="MIOpen conv2d + srf_channel_affine + add + relu_ (NCHW)", routes_max_diff_over_max=float(f"{diff:.3e}"),
                       window_s=min_s)


def randomize(model, img):
    g = torch.Generator().manual_seed(0)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)

    def hook(mod, args):   # conv_offset ~ N(0, s), s from the layer's own input: offsets of about one pixel (as tools/bench_dcn.py)
        rms = args[0].square().mean().sqrt().clamp_min(1e-6)
        mod.conv_offset.weight.copy_((torch.randn(mod.conv_offset.weight.shape, generator=g) / (3 * mod.in_channels ** 0.5)).to(rms.device) / rms)

    hooks = [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, ModulatedDeformConv2dPack)]
    if hooks:
        route(False)
        with torch.no_grad():
            model.img_backbone(img)
        route(True)
    for h in hooks:
        h.remove()


def frame(config, dev, min_s, repeats):
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    waymo = "waymo" in config
    n_cam, h, w = (5, 640, 960) if waymo else (N_IMG, H_IMG, W_IMG)
    model = workloads.build(config, 200).eval().to(dev)
    img = torch.from_numpy(S.camera_images(3000, n_cam=n_cam, h=h, w=w)).to(dev)
    randomize(model, img[0])
    rig = S.camera_rig(n_cam=5, f=1266.0 * 960 / 1600, cx=480.0, cy=320.0) if waymo else S.camera_rig()
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in rig])]
    pts = torch.from_numpy(S.waymo_sweep(5000, 180000) if waymo else S.nuscenes_sweep(2000)).to(dev)
    with torch.no_grad():
        route(True)
        on = model.extract_img_feat(img, copy.deepcopy(metas))
        route(False)
        off = model.extract_img_feat(img, copy.deepcopy(metas))
        diff = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(on, off))
        t = alternate({"hip": (lambda: route(True), lambda: model.extract_img_feat(img, copy.deepcopy(metas))),
                       "torch": (lambda: route(False), lambda: model.extract_img_feat(img, copy.deepcopy(metas)))}, min_s, repeats, warm=3)
        models = {}
        for name, flag in (("hip", True), ("torch", False)):
            route(flag)
            graphed = copy.deepcopy(model).enable_hip_graphs(img_overlap=True)
            for _ in range(3):
                graphed.simple_test(img, [pts], copy.deepcopy(metas))
            models[name] = graphed
        torch.cuda.synchronize()

        def fps(m, flag):
            route(flag)
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

        out = dict(config=config, num_proposals=200, images=f"{n_cam} x {h} x {w}", points=int(pts.shape[0]),
                   img_branch_ms_hip=[round(v / 1e3, 3) for v in t["hip"]], img_branch_ms_torch=[round(v / 1e3, 3) for v in t["torch"]],
                   img_branch_speedup=[round(b / a, 3) for a, b in zip(t["hip"], t["torch"])], graph_fps_hip=[], graph_fps_torch=[],
                   routes_max_diff_over_max=float(f"{diff:.3e}"), window_s=min_s,
                   timer="image branch: device events around windows of extract_img_feat; frames: host clock around simple_test, device "
                         "synchronised at both ends",
                   note="torch = nhwc.resnet switched off, NOT the environment switch SRF_IMG_NHWC=0: for the image branch the two are the same "
                        "route (ResNet through the modules on MIOpen, the FPN on NCHW tensors), but SRF_IMG_NHWC=0 would also take the BEV "
                        "backbone and neck off the executor, which they were on before; same process, windows alternated")
        for _ in range(repeats):
            out["graph_fps_hip"].append(round(fps(models["hip"], True), 2))
            out["graph_fps_torch"].append(round(fps(models["torch"], False), 2))
    route(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--config", action="append", help="frame mode: the configs to run (default: both)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resnet.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    if args.frame:
        gen = (frame(c, dev, max(args.window, 2.0), args.repeats) for c in (args.config or ["srfdet_voxel_r50_nusc_LC", "srfdet_dvoxel_waymo_LC"]))
    else:
        gen = layers(dev, args.window, args.repeats)
    for ln in gen:
        print(json.dumps(ln), flush=True)
        lines.append(ln)
        if args.out:
            with open(args.out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")


if __name__ == "__main__":
    main()
