#!/usr/bin/env python3
"""Generate tests/golden/lidar_encoder.npz from the reference's own Python (run in the build container only).

What runs: the reference's `SRFDetHead._build_lidar_encoder`, `_init_weights`, `create_2D_grid`, `PositionEmbeddingLearned` and
`_get_lidar_encoder_feats` (srfdet_head.py:25-45, :209-263, :657-758), loaded by path with the stand-in loader of make_fixtures.py,
in eval mode.  No reference source is copied: this script executes the file where it lies and stores the arrays it returns.

Unpinned part: mmcv is not installed, so `build_transformer_layer_sequence` and `MultiScaleDeformableAttention` (srfdet_head.py:10-11)
are this repository's srfdet3d_amd/compat/transformer.py, on its torch route (CPU).  The fixture therefore pins everything the head
does around the encoder (grids, the x / H and y / W normalisation in float32, position and level embeddings, the flatten / split
order) and holds the encoder itself to its own float64 evaluation; the operator inside is held to its written definition by
tests/test_msda_ref.py and tests/test_gpu_msda.py.

Weights and inputs come from detgen on both sides, so the file holds outputs only.  Per case, each run in float64 and in float32:
    <case>.out<l>   float64 output of level l, (B, C, H_l, W_l); the low 20 mantissa bits are zeroed (2^-33 relative, five orders below
                    the float32 figure) so that the file compresses
    <case>.e_f32    max |f32 - f64| / max |f64| over the case's four levels, against the stored float64 arrays: the float32 figure the tests
                    scale their bound from.  The host GEMM's summation order depends on its thread count, so the float32 run is repeated
                    with 1, 2, 4, 8 and 16 threads and with the library's default, and the largest figure is stored.
Cases (name: C, grid_size, B; levels are int(grid_size / 8 / 2**l)):
    c128: 128, [128, 96, 40], 2     16 x 12, 8 x 6, 4 x 3, 2 x 1
    c256: 256, [96, 128, 40], 1     12 x 16, 6 x 8, 3 x 4, 1 x 2: non-square the other way (the H / W quirk), a one-pixel level

usage:  python tests/golden/make_lidar_encoder_fixture.py [--ref /root/reference]
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_fixtures as MF  # noqa: E402  (also puts the repository root on sys.path)
import detgen  # noqa: E402

CASES = {"c128": (128, [128, 96, 40], 2), "c256": (256, [96, 128, 40], 1)}
LEVELS, OUT_SIZE_FACTOR = 4, 8


def level_sizes(grid_size):
    xs, ys = grid_size[0] // OUT_SIZE_FACTOR, grid_size[1] // OUT_SIZE_FACTOR
    return [(int(xs / 2 ** l), int(ys / 2 ** l)) for l in range(LEVELS)]


def prefix(case):
    return f"lidarenc.{case}."


def inputs(case):
    """The BEV pyramid of a case, float32 numpy (B, C, H, W) per level."""
    C, grid, B = CASES[case]
    return [detgen.det(f"{prefix(case)}feat{l}", (B, C, H, W), scale=0.5) for l, (H, W) in enumerate(level_sizes(grid))]


def encoder_cfg(C):
    """`lidar_encoder_cfg` of the configs (settings only), at C channels."""
    from srfdet3d_amd import workloads
    cfg = workloads.model_cfg("srfdet_voxel_nusc_L").bbox_head.lidar_encoder_cfg
    cfg = {k: v for k, v in cfg.items()}
    layer = dict(cfg["transformerlayers"])
    layer["attn_cfgs"] = dict(layer["attn_cfgs"], embed_dims=C)
    layer["ffn_cfgs"] = dict(layer["ffn_cfgs"], embed_dims=C, feedforward_channels=2 * C)
    layer["feedforward_channels"] = 2 * C
    cfg["transformerlayers"] = layer
    return cfg


def load_encoder_params(module, case):
    """det_param for every parameter and buffer of the encoder part of a head (the reference's stub or this repository's head)."""
    with torch.no_grad():
        for n, p in list(module.named_parameters()) + list(module.named_buffers()):
            if n.startswith(("encoder_lidar.", "bev_pos_encoder_mlvl_embed.", "bev_level_embeds")):
                p.copy_(torch.from_numpy(detgen.det_param(prefix(case) + n, p.shape)).to(p.dtype))
    return module


def run_case(head, case, dtype):
    C, grid, B = CASES[case]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        hd = object.__new__(head.SRFDetHead)
        nn.Module.__init__(hd)
        hd.with_lidar_encoder, hd.lidar_encoder_cfg, hd.lidar_feat_lvls, hd.feat_channels_lidar = True, encoder_cfg(C), LEVELS, C
        hd.grid_size, hd.out_size_factor = grid, OUT_SIZE_FACTOR
        hd.prior_prob, hd.use_focal_loss, hd.use_fed_loss, hd.num_classes = 0.01, True, False, 10
        hd._build_lidar_encoder()
        hd._init_weights()
        hd.eval()
        load_encoder_params(hd, case)
        feats = [torch.from_numpy(f).to(dtype) for f in inputs(case)]
        with torch.no_grad():
            out = hd._get_lidar_encoder_feats(feats)
        return [o.double().numpy() for o in out]
    finally:
        torch.set_default_dtype(old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    MF.install_stand_ins()
    _, head = MF.load_reference(args.ref)
    from srfdet3d_amd.compat import transformer as T
    head.build_transformer_layer_sequence = T.build_transformer_layer_sequence
    head.MultiScaleDeformableAttention = T.MultiScaleDeformableAttention
    out = {}
    default_threads = torch.get_num_threads()
    for case in CASES:
        o64 = [(o.view(np.uint64) & ~np.uint64((1 << 20) - 1)).view(np.float64) for o in run_case(head, case, torch.float64)]
        top = max(np.abs(o).max() for o in o64)
        figures = {}
        for threads in (1, 2, 4, 8, 16, default_threads):
            torch.set_num_threads(threads)
            o32 = run_case(head, case, torch.float32)
            figures[threads] = max(np.abs(a - b).max() for a, b in zip(o32, o64)) / top
        torch.set_num_threads(default_threads)
        out[f"{case}.e_f32"] = np.float64(max(figures.values()))
        for l, o in enumerate(o64):
            out[f"{case}.out{l}"] = o
        print(case, [o.shape for o in o64], "max |f64|", top, "e_f32 per thread count", figures)
    path = os.path.join(HERE, "lidar_encoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
