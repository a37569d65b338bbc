"""Times the bf16-product mode of the sparse encoder (csrc/spconv_bf16.hip, `sparse.mfma_dtype`, `SRFDet.sparse_mfma_dtype`) against
the f32 route it is an alternative to, in one process, alternating.

Layer mode (default): the layers of the five shapes with a bf16-product form, on the rulebooks of a 30k-point nuScenes sweep
(srfdet_voxel_nusc_L) and a 180k-point Waymo sweep (srfdet_dvoxel_waymo_L), taken from the models themselves: one eager pass of the
encoder with `ops.spconv_fwd` wrapped records each such call's shape, rulebook, row plan and how often it occurs per frame.  Each
distinct (shape, rulebook) then runs on post-ReLU-like random data (not zeros) with random weights and a random folded BatchNorm +
ReLU: the f32 route (`srf_spconv_fwd_packed` with the row plan the encoder passes) and the bf16 kernel alternated in windows of
>= 0.5 s timed with device events, three repeats.  One JSON line per layer: us and TFLOP/s of the PAIRS' FLOPs (2 pairs Cin Cout) of
both, the speed-up per repeat, and whether the bf16 form is faster by more than the spread of the repeats (else the shape belongs in
`ops.SPCONV_BF16_NOT_FASTER`); a summary line with the per-frame totals.

Frame mode (--frame): frames/s of nusc_L and waymo_L with the switch off and on, and of nusc_LC with and without `img_mfma_dtype`
under both, every model through enable_hip_graphs(), alternated in one process; per config the relative RMS difference of the BEV
map and the largest difference of the pre-NMS box parameters between the two routes of the sparse encoder (eager passes).

  python tools/bench_spconv_bf16.py [--out profiles/spconv_bf16_layer_bench.json]
  python tools/bench_spconv_bf16.py --frame [--out profiles/spconv_bf16_frame_bench.json]
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
from srfdet3d_amd import ops, synthetic as S, workloads  # noqa: E402
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes  # noqa: E402

BF16 = torch.bfloat16
BF16_PEAK_TFLOPS, F32_PEAK_TFLOPS = 2500.0, 157.3
CONFIGS = {"nusc_L": ("srfdet_voxel_nusc_L", "nuscenes_sweep", 2000, 30000), "waymo_L": ("srfdet_dvoxel_waymo_L", "waymo_sweep", 5000, 180000),
           "nusc_LC": ("srfdet_voxel_nusc_LC", "nuscenes_sweep", 2000, 30000)}


def window(fn, min_s):
    """Mean time of fn() in us over a window of at least min_s seconds (device events around the whole window)."""
    n = 8
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


def randomize_bn(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def build(name, dev, num_proposals=200):
    cfg, sweep, seed, points = CONFIGS[name]
    torch.manual_seed(0)
    model = workloads.build(cfg, num_proposals).eval()
    randomize_bn(model)
    pts = torch.from_numpy(getattr(S, sweep)(seed, points)).to(dev)
    return model.to(dev), pts


def encoder_layers(name, dev):
    """The calls of one eager encoder pass that have a bf16-product form: {(K, Cin, Cout, A_in, A_out, subm): [count, nbr, plan, pairs]}."""
    model, pts = build(name, dev)
    seen = {}
    real = ops.spconv_fwd

    def spconv_fwd(feats, weight, nbr, alpha=None, beta=None, residual=None, relu=False, pair_counts=None, packed=None, rows_dev=None,
                   tiles=None, subm=False):
        K, cin, cout = weight.shape
        if ops.spconv_bf16_supported(K, cin, cout):
            key = (K, cin, cout, feats.shape[0], nbr.shape[1], bool(subm))
            if key not in seen:
                seen[key] = [0, nbr.clone(), None if tiles is None else tiles.clone(), int((nbr >= 0).sum().item())]
            seen[key][0] += 1
        return real(feats, weight, nbr, alpha, beta, residual, relu, pair_counts, packed, rows_dev, tiles, subm)

    ops.spconv_fwd = spconv_fwd
    try:
        with torch.no_grad():
            model.extract_bev([pts])
    finally:
        ops.spconv_fwd = real
    del model
    torch.cuda.empty_cache()
    return seen


def layer(name, key, rec, dev, min_s, repeats):
    K, cin, cout, a_in, a_out, subm = key
    count, nbr, plan, pairs = rec
    g = torch.Generator().manual_seed(cin * 7 + cout + K)
    x = torch.relu(torch.randn(a_in, cin, generator=g) * 1.5 + 0.2).to(dev)          # ~45 % zeros, as behind a ReLU
    w = (torch.randn(K, cin, cout, generator=g) / (K * cin) ** 0.5).to(dev)
    alpha, beta = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
    p32, pbf = ops.pack_spconv_weights(w), ops.pack_spconv_bf16_weights(w)
    f32 = lambda: ops.spconv_fwd(x, w, nbr, alpha, beta, None, True, packed=p32, tiles=plan, subm=subm)      # noqa: E731
    bf = lambda: ops.spconv_fwd_bf16(x, w, nbr, pbf, alpha, beta, None, True)                               # noqa: E731
    with torch.no_grad():
        a, b = f32(), bf()
        rel = ((b.double() - a.double()).pow(2).mean().sqrt() / a.double().pow(2).mean().sqrt()).item()
        for f in (f32, bf):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t32, tbf = [], []
        for _ in range(repeats):
            t32.append(window(f32, min_s))
            tbf.append(window(bf, min_s))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    flops = 2.0 * pairs * cin * cout
    spread = max(max(t32) / min(t32), max(tbf) / min(tbf)) - 1.0
    return dict(config=name, shape=f"{cin}->{cout} k{K} {'subm' if subm else 'strided'}", rows_in=a_in, rows_out=a_out, pairs=pairs,
                pairs_per_row=round(pairs / max(a_out, 1), 2), per_frame=count, f32_route_us=[round(t, 1) for t in t32],
                bf16_us=[round(t, 1) for t in tbf], speedup=[round(p / q, 3) for p, q in zip(t32, tbf)], spread_of_repeats=round(spread, 4),
                faster_beyond_spread=min(t32) > max(tbf) * (1.0 + spread), flops=flops,
                f32_route_tflops=round(flops / med(t32) / 1e6, 2), bf16_tflops=round(flops / med(tbf) / 1e6, 2),
                frac_f32_mfma_peak=round(flops / med(t32) / 1e6 / F32_PEAK_TFLOPS, 4), frac_bf16_mfma_peak=round(flops / med(tbf) / 1e6 / BF16_PEAK_TFLOPS, 4),
                rel_rms_diff_of_outputs=rel, window_s=min_s, timer="device events around each window")


def _set(model, sparse_bf16, img_bf16=False):
    m = copy.deepcopy(model)
    if sparse_bf16:
        m.sparse_mfma_dtype = BF16
    if img_bf16:
        m.img_mfma_dtype = BF16
    return m


def frame_config(name, dev, min_s, repeats):
    model, pts = build(name, dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    img = None
    if model.use_img:
        img = torch.from_numpy(S.camera_images(3000)).to(dev)
        metas[0]["lidar2img"] = [m for m in S.camera_rig()]
    # what the switch changes, measured eagerly on one frame: the BEV map and the pre-NMS boxes
    out = dict(config=CONFIGS[name][0], num_proposals=200, points=int(pts.shape[0]))
    with torch.no_grad():
        res = {}
        for tag, on in (("f32", False), ("bf16", True)):
            m = _set(model, on)
            bev = m.extract_bev([pts]).float().clone()
            feats = m.extract_point_features([pts])
            img_feats = m.extract_img_feat(img, copy.deepcopy(metas)) if img is not None else None
            _, boxes = m.bbox_head(img_feats, feats, copy.deepcopy(metas))
            res[tag] = (bev, boxes.float().clone())
            del m
        a, b = res["f32"], res["bf16"]
        out["bev_rel_rms_diff"] = ((b[0].double() - a[0].double()).pow(2).mean().sqrt() / a[0].double().pow(2).mean().sqrt()).item()
        out["pre_nms_box_max_abs_diff"] = (b[1] - a[1]).abs().max().item()
    combos = [("sparse_f32", False, False), ("sparse_bf16", True, False)]
    if model.use_img:
        combos = [("img_f32_sparse_f32", False, False), ("img_f32_sparse_bf16", True, False), ("img_bf16_sparse_f32", False, True),
                  ("img_bf16_sparse_bf16", True, True)]
    models = {}
    for tag, sp, im in combos:
        m = _set(model, sp, im).enable_hip_graphs()
        with torch.no_grad():
            for _ in range(3):
                m.simple_test(img, [pts], copy.deepcopy(metas))
        models[tag] = m
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

    out.update(fps={k: [] for k in models}, window_s=min_s, note="one process, windows alternated over the routes per repeat",
               timer="host clock around whole frames (simple_test through enable_hip_graphs), device synchronised at both ends")
    for _ in range(repeats):
        for tag, m in models.items():
            out["fps"][tag].append(round(fps(m), 2))
    tags = list(models)
    out["sparse_bf16_over_f32"] = {f"{tags[i + 1]} / {tags[i]}": [round(q / p, 4) for p, q in zip(out["fps"][tags[i]], out["fps"][tags[i + 1]])]
                                   for i in range(0, len(tags), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--configs", default=None, help="comma-separated subset of nusc_L,waymo_L (layer mode) / nusc_L,waymo_L,nusc_LC (--frame)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spconv_bf16.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []
    if args.frame:
        for name in (args.configs.split(",") if args.configs else ["nusc_L", "waymo_L", "nusc_LC"]):
            lines.append(frame_config(name, dev, max(args.window, 2.0), args.repeats))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    else:
        for name in (args.configs.split(",") if args.configs else ["nusc_L", "waymo_L"]):
            for key, rec in encoder_layers(name, dev).items():
                lines.append(layer(name, key, rec, dev, args.window, args.repeats))
                print(json.dumps(lines[-1]), flush=True)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        layers = list(lines)
        for name in sorted({ln["config"] for ln in layers}):
            sel = [ln for ln in layers if ln["config"] == name]
            t32 = sum(med(ln["f32_route_us"]) * ln["per_frame"] for ln in sel)
            tbf = sum(med(ln["bf16_us"]) * ln["per_frame"] for ln in sel)
            fl = sum(ln["flops"] * ln["per_frame"] for ln in sel)
            lines.append(dict(summary=f"{name}: the 64- / 128-channel layers of one encoder pass, medians weighted by per_frame",
                              layers=sum(ln["per_frame"] for ln in sel), f32_route_ms=round(t32 / 1e3, 3), bf16_ms=round(tbf / 1e3, 3),
                              flops=fl, f32_route_tflops=round(fl / t32 / 1e6, 2), bf16_tflops=round(fl / tbf / 1e6, 2),
                              not_faster_beyond_spread=[ln["shape"] + f" @{ln['rows_out']}" for ln in sel if not ln["faster_beyond_spread"]]))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
