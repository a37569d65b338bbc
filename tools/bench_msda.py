"""Times multi-scale deformable attention (srf_msda_fwd, csrc/msda.hip) and the LiDAR BEV encoder around it against the torch route
(SRF_MSDA=0: one grid_sample per level), in one process, alternating.

Kernel mode (default): the nuScenes shape of `encoder_lidar` -- levels 184^2, 92^2, 46^2, 23^2 (S = Q = 44 965 rows), 8 heads x 16
channels, 4 points -- with the offsets of a freshly initialised attention (the ring: 1..4 pixels) plus N(0, 0.5).  One JSON line: time per
call, the bytes gathered (rows x heads x 64 samples-corners x 64 B segments) and the gather rate they make, to be read against the
Infinity-Cache row of the gather table of the MI355X notes (8.6 TB/s chip-wide for 1 152-byte rows; these segments are 64 bytes), and the
same on the KITTI shape (200 x 176 ..., 8 x 32 channels).
Layer mode (--layer): one `BaseTransformerLayer` of the encoder on the same rows, `forward_rows` (six launches and an add) against the
module's torch route on the (S, 1, C) sequence; warm-up, then alternated windows.
Frame mode (--frame): srfdet_voxel_nusc_L with `bbox_head.with_lidar_encoder=True` at num_proposals = 200 on a synthetic sweep, through
enable_hip_graphs(), frames/s, both routes alternated, and the same model without the encoder for scale.
Backward mode (--backward): training.  Per shape the backward kernel alone (srf_msda_bwd, csrc/msda_bwd.hip; the bytes its atomics add
and the rate they make, to be read against the 1.3 TB/s float-atomic row of the MI355X notes), the sampling core forward + backward as
`ops._MsdaFn` against `multi_scale_deformable_attn_pytorch`, and one encoder layer forward + backward in eval mode with gradients on
(dropout an identity), both routes alternated, with `torch.cuda.max_memory_allocated` of a step on each route.

  python tools/bench_msda.py [--layer | --frame | --backward] [--out FILE]   (--out appends one JSON line per result;
                                                                               profiles/msda_bench.json, profiles/msda_bwd_bench.json)
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import ops, synthetic as S, workloads  # noqa: E402
from srfdet3d_amd.compat import transformer as T  # noqa: E402

SHAPES = {"nusc": ([(184, 184), (92, 92), (46, 46), (23, 23)], 128), "kitti": ([(200, 176), (100, 88), (50, 44), (25, 22)], 256)}
HEADS, POINTS = 8, 4


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


def route(on):
    if on:
        os.environ.pop("SRF_MSDA", None)
    else:
        os.environ["SRF_MSDA"] = "0"


def rows_case(name, dev, seed=0):
    """x (S, C) rows, pos (S, C), ref (S, L, 2) and a layer with non-trivial offsets for a shape of SHAPES."""
    shapes, C = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    S_ = sum(h * w for h, w in shapes)
    layer = T.build_transformer_layer(dict(type="BaseTransformerLayer", attn_cfgs=dict(type="MultiScaleDeformableAttention", embed_dims=C,
                                                                                      num_levels=len(shapes)),
                                           ffn_cfgs=dict(type="FFN", embed_dims=C, feedforward_channels=2 * C, num_fcs=2, ffn_drop=0.1,
                                                         act_cfg=dict(type="ReLU", inplace=True)),
                                           operation_order=("self_attn", "norm", "ffn", "norm")))
    att = layer.attentions[0]
    with torch.no_grad():
        att.sampling_offsets.weight.copy_(torch.randn(att.sampling_offsets.weight.shape, generator=g) * (0.5 / C ** 0.5))
        att.attention_weights.weight.copy_(torch.randn(att.attention_weights.weight.shape, generator=g) * (1.0 / C ** 0.5))
    ref = []
    for H, W in shapes:
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        ref.append(torch.stack(((xs.flatten() + 0.5) / W, (ys.flatten() + 0.5) / H), -1))
    ref = torch.cat(ref).unsqueeze(1).repeat(1, len(shapes), 1).contiguous()
    x = torch.randn(S_, C, generator=g)
    pos = torch.randn(S_, C, generator=g) * 0.5
    return layer.eval().to(dev), x.to(dev), pos.to(dev), ref.to(dev), shapes, C


def kernel(name, dev, min_s, repeats):
    layer, x, pos, ref, shapes, C = rows_case(name, dev)
    att = layer.attentions[0]
    ns = HEADS * len(shapes) * POINTS
    with torch.no_grad():
        value = ops.linear(x, att.value_proj.weight, att.value_proj.bias)
        wq, bq = att.qproj()
        qp = ops.linear(x + pos, wq, bq)
        out = torch.empty_like(value)

        def call():
            ops.msda(value, shapes, ref, qp[:, :2 * ns], qp[:, 2 * ns:], HEADS, POINTS, out=out)

        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t = [window(call, min_s) for _ in range(repeats)]
    rows, d = x.shape[0], C // HEADS
    gathered = rows * HEADS * len(shapes) * POINTS * 4 * d * 4.0
    streamed = rows * (3 * ns + 2 * len(shapes) + C) * 4.0
    med = sorted(t)[len(t) // 2]
    return dict(mode="kernel", shape=name, levels=shapes, rows=rows, heads=HEADS, head_dim=d, points=POINTS, kernel_us=[round(v, 1) for v in t],
                gathered_bytes=gathered, segment_bytes=4 * d, value_table_bytes=rows * C * 4.0, streamed_bytes=streamed,
                gather_rate_TBps=round(gathered / (med * 1e-6) / 1e12, 3), offset_std_px=round(qp[:, :2 * ns].std().item(), 2),
                window_s=min_s, timer="device events around each window")


def layer_mode(name, dev, min_s, repeats):
    layer, x, pos, ref, shapes, C = rows_case(name, dev)
    q3, p3, r3 = x.unsqueeze(1), pos.unsqueeze(1), ref.unsqueeze(0)
    with torch.no_grad():
        def hip():
            return layer.forward_rows(x, pos, ref, shapes)

        def torch_route():
            return layer(q3, None, None, query_pos=p3, spatial_shapes=shapes, reference_points=r3)

        a, b = hip(), torch_route()[:, 0]
        diff = ((a - b).abs().max() / b.abs().max()).item()
        for fn in (hip, torch_route):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        t_hip, t_torch = [], []
        for _ in range(repeats):
            t_hip.append(window(hip, min_s))
            t_torch.append(window(torch_route, min_s))
    rows = x.shape[0]
    flops = 2.0 * rows * C * (C + 3 * HEADS * len(shapes) * POINTS + C + 2 * C + 2 * C)
    return dict(mode="layer", shape=name, rows=rows, channels=C, hip_route_us=[round(v, 1) for v in t_hip],
                torch_route_us=[round(v, 1) for v in t_torch], speedup=[round(b / a, 2) for a, b in zip(t_hip, t_torch)],
                gemm_flops=flops, routes_max_diff_over_max=float(f"{diff:.3e}"),
                hip_route_is="srf_linear x 5 (value_proj, offsets + logits, output_proj + residual + LN, fc1 + ReLU, fc2 + residual + LN), "
                             "one add, srf_msda_fwd",
                torch_route_is="the module: srf_linear GEMMs, softmax, 4 x grid_sample, stack, multiply, sum, LayerNorms",
                window_s=min_s, timer="device events around each window")


def backward_mode(name, dev, min_s, repeats):
    """Three lines per shape: srf_msda_bwd alone (into caller-owned buffers, so no zeroing is timed; the sums just grow), the sampling
    core forward + backward as `ops._MsdaFn` against `multi_scale_deformable_attn_pytorch` (softmax and positions included on both
    sides), and one encoder layer forward + backward in eval mode with gradients on, both routes, with the peak memory of each."""
    layer, x, pos, ref, shapes, C = rows_case(name, dev)
    att = layer.attentions[0]
    L, d = len(shapes), C // HEADS
    ns = HEADS * L * POINTS
    rows = x.shape[0]
    common = dict(shape=name, rows=rows, heads=HEADS, head_dim=d, points=POINTS, window_s=min_s, timer="device events around each window")
    g = torch.Generator().manual_seed(1)
    cot = torch.randn(rows, C, generator=g).to(dev)
    with torch.no_grad():
        value = ops.linear(x, att.value_proj.weight, att.value_proj.bias)
        wq, bq = att.qproj()
        qp = ops.linear(x + pos, wq, bq)
    offs, logits = qp[:, :2 * ns], qp[:, 2 * ns:]
    outs = (torch.zeros_like(value), torch.empty(rows, 2 * ns, device=dev), torch.empty(rows, ns, device=dev))

    def kernel_call():
        ops.msda_backward(value, shapes, ref, offs, logits, HEADS, POINTS, cot, out=outs)

    for _ in range(10):
        kernel_call()
    torch.cuda.synchronize()
    t = [window(kernel_call, min_s) for _ in range(repeats)]
    med = sorted(t)[len(t) // 2]
    added = rows * HEADS * L * POINTS * 4 * d * 4.0
    lines = [dict(mode="backward_kernel", kernel_us=[round(v, 1) for v in t], atomic_bytes_upper=added, segment_bytes=4 * d,
                  atomic_rate_TBps=round(added / (med * 1e-6) / 1e12, 3),
                  note="atomic_bytes_upper counts four corners for every sample; samples and corners outside the map add nothing", **common)]

    # ---- the sampling core, forward + backward ----
    lv = [t_.detach().clone().requires_grad_() for t_ in (value, offs.contiguous(), logits.contiguous())]
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device=dev)

    def core_hip():
        for t_ in lv:
            t_.grad = None
        ops.msda_autograd(lv[0], shapes, ref, lv[1], lv[2], HEADS, POINTS).backward(cot)

    def core_torch():
        for t_ in lv:
            t_.grad = None
        w = lv[2].view(1, rows, HEADS, L * POINTS).softmax(-1).view(1, rows, HEADS, L, POINTS)
        loc = ref.view(1, rows, 1, L, 1, 2) + lv[1].view(1, rows, HEADS, L, POINTS, 2) / norm[None, None, None, :, None, :]
        T.multi_scale_deformable_attn_pytorch(lv[0].view(1, rows, HEADS, d), shapes, loc, w).view(rows, C).backward(cot)

    lines.append(dict(mode="backward_core", **_alternate(core_hip, core_torch, lambda: [t_.grad.clone() for t_ in lv],
                                                         ("value", "offs", "logits"), min_s, repeats),
                      hip_route_is="ops._MsdaFn: srf_msda_fwd, srf_msda_bwd and the zeroing of grad_value",
                      torch_route_is="softmax, positions, 4 x grid_sample, stack, multiply, sum and their autograd backward", **common))

    # both routes against the torch route in float64 on the same inputs
    l64 = [t_.detach().double().requires_grad_() for t_ in lv]
    w = l64[2].view(1, rows, HEADS, L * POINTS).softmax(-1).view(1, rows, HEADS, L, POINTS)
    loc = ref.double().view(1, rows, 1, L, 1, 2) + l64[1].view(1, rows, HEADS, L, POINTS, 2) / norm.double()[None, None, None, :, None, :]
    T.multi_scale_deformable_attn_pytorch(l64[0].view(1, rows, HEADS, d), shapes, loc, w).view(rows, C).backward(cot.double())
    vs64 = {}
    for key, fn in (("hip", core_hip), ("torch", core_torch)):
        fn()
        vs64[key] = {}
        for tname, a, b in zip(("value", "offs", "logits"), lv, l64):
            dd, top = (a.grad.double() - b.grad).abs(), b.grad.abs().max()
            vs64[key][tname] = dict(max_diff_over_max=float(f"{(dd.max() / top).item():.3e}"),
                                    share_over_1e_3=float(f"{(dd > 1e-3 * top).double().mean().item():.3e}"),
                                    rms_diff_over_rms=float(f"{(dd.pow(2).mean().sqrt() / b.grad.pow(2).mean().sqrt()).item():.3e}"))
    lines[-1]["grads_vs_torch_float64"] = vs64
    del l64, w, loc
    torch.cuda.empty_cache()

    # ---- one encoder layer, forward + backward, eval mode, gradients on ----
    q3, p3, r3 = x.unsqueeze(1).clone().requires_grad_(), pos.unsqueeze(1), ref.unsqueeze(0)
    cot3 = cot.unsqueeze(1)
    params = [q3] + list(layer.parameters())

    def layer_step():
        for t_ in params:
            t_.grad = None
        layer(q3, None, None, query_pos=p3, spatial_shapes=shapes, reference_points=r3).backward(cot3)

    def layer_hip():
        route(True)
        layer_step()

    def layer_torch():
        route(False)
        layer_step()

    res = _alternate(layer_hip, layer_torch, lambda: [t_.grad.clone() for t_ in params], ["query"] + [n for n, _ in layer.named_parameters()],
                     min_s, repeats)
    route(True)
    lines.append(dict(mode="backward_layer", channels=C, **res,
                      hip_route_is="the module under autograd with the sampling core as ops._MsdaFn", torch_route_is="the module with SRF_MSDA=0",
                      **common))
    return lines


def _alternate(hip, torch_route, grads, names, min_s, repeats):
    """Warm up, compare the two routes' gradients, record each route's peak memory over one step, then time alternated windows."""
    out = {}
    for key, fn in (("hip", hip), ("torch", torch_route)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[f"{key}_peak_MB_above_resident"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        out[f"{key}_max_memory_allocated_MB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        out[key] = grads()
    # The offset gradient is not continuous where a position crosses an integer, and the two routes round the position differently (the
    # torch route goes through normalised coordinates), so a few samples in a million legitimately take the neighbouring cell: the
    # largest difference is theirs.  Hence also the share of elements that differ by more than 1e-3 of the tensor's largest entry.
    per = {}
    for name, a, b in zip(names, out.pop("hip"), out.pop("torch")):
        d, top = (a - b).abs(), b.abs().max().clamp_min(1e-30)
        per[name] = dict(max_diff_over_max=float(f"{(d.max() / top).item():.3e}"), share_over_1e_3=float(f"{(d > 1e-3 * top).float().mean().item():.3e}"))
    diff = max(v["max_diff_over_max"] for v in per.values())
    out["grads_hip_vs_torch"] = per
    t_hip, t_torch = [], []
    for _ in range(repeats):
        t_hip.append(window(hip, min_s))
        t_torch.append(window(torch_route, min_s))
    out.update(hip_route_us=[round(v, 1) for v in t_hip], torch_route_us=[round(v, 1) for v in t_torch],
               speedup=[round(b / a, 2) for a, b in zip(t_hip, t_torch)], grads_max_diff_over_max=float(f"{diff:.3e}"))
    return out


def frame(dev, min_s, repeats):
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 30000)).to(dev)
    enc = workloads.build("srfdet_voxel_nusc_L", 200, **{"bbox_head.with_lidar_encoder": True}).eval()
    with torch.no_grad():
        for m in enc.bbox_head.encoder_lidar.modules():
            if hasattr(m, "sampling_offsets"):
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
    plain = workloads.build("srfdet_voxel_nusc_L", 200).eval()
    models = {}
    for name, model, on in (("hip", enc, True), ("torch", enc, False), ("no_encoder", plain, True)):
        route(on)
        g = copy.deepcopy(model).to(dev).enable_hip_graphs()
        with torch.no_grad():
            for _ in range(3):
                g.simple_test(None, [pts], copy.deepcopy(metas))
        models[name] = (g, on)
    torch.cuda.synchronize()

    def fps(name):
        m, on = models[name]
        route(on)
        n, t0 = 0, time.perf_counter()
        with torch.no_grad():
            while True:
                m.simple_test(None, [pts], copy.deepcopy(metas))
                n += 1
                if n % 4 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= min_s:
                        break
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    out = dict(mode="frame", config="srfdet_voxel_nusc_L + bbox_head.with_lidar_encoder=True", num_proposals=200, points=int(pts.shape[0]),
               graph_fps_hip=[], graph_fps_torch=[], graph_fps_no_encoder=[], window_s=min_s,
               timer="host clock around whole frames (simple_test), device synchronised at both ends",
               note="torch = SRF_MSDA=0; same process, windows alternated; no_encoder = the config as shipped (flag off)")
    for _ in range(repeats):
        out["graph_fps_hip"].append(round(fps("hip"), 2))
        out["graph_fps_torch"].append(round(fps("torch"), 2))
        out["graph_fps_no_encoder"].append(round(fps("no_encoder"), 2))
    route(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", action="store_true")
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--backward", action="store_true", help="srf_msda_bwd alone, the core and one layer forward + backward, both routes")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window and route")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msda.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if args.frame:
        lines = [frame(dev, max(args.window, 2.0), args.repeats)]
    elif args.backward:
        lines = [ln for n in SHAPES for ln in backward_mode(n, dev, args.window, args.repeats)]
    elif args.layer:
        lines = [layer_mode(n, dev, args.window, args.repeats) for n in SHAPES]
    else:
        lines = [kernel(n, dev, args.window, args.repeats) for n in SHAPES]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
