"""`SRFDetHead(with_lidar_encoder=True)` on the host: construction from the configs' own `lidar_encoder_cfg`, state_dict names and shapes,
the attention's initialisation, `encode_lidar` on the CPU against the reference's `_get_lidar_encoder_feats`
(tests/golden/lidar_encoder.npz, made by tests/golden/make_lidar_encoder_fixture.py), and that nothing changes with the flag off."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from srfdet3d_amd import workloads
from srfdet3d_amd.compat import transformer as T
from srfdet3d_amd.compat.registry import build_head

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import detgen  # noqa: E402

CASES = {"c128": (128, [128, 96, 40], 2), "c256": (256, [96, 128, 40], 1)}      # make_lidar_encoder_fixture.CASES


def _head(name, **over):
    m = workloads.model_cfg(name, **{"bbox_head.with_lidar_encoder": True})
    hc = dict(m.bbox_head)
    hc.update(num_proposals=16, train_cfg=None, test_cfg=m.test_cfg, use_img=False, **over)
    return build_head(hc)


def fixture_head(case, dtype=torch.float32):
    """This repository's head for a fixture case, with the fixture's weights (shared with tests/test_gpu_lidar_encoder.py)."""
    C, grid, _ = CASES[case]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        m = workloads.model_cfg("srfdet_voxel_nusc_L", **{"bbox_head.with_lidar_encoder": True})
        hc = dict(m.bbox_head)
        enc = dict(hc["lidar_encoder_cfg"])
        layer = dict(enc["transformerlayers"])
        layer["attn_cfgs"] = dict(layer["attn_cfgs"], embed_dims=C)
        layer["ffn_cfgs"] = dict(layer["ffn_cfgs"], embed_dims=C, feedforward_channels=2 * C)
        layer["feedforward_channels"] = 2 * C
        enc["transformerlayers"] = layer
        hc.update(num_proposals=16, train_cfg=None, test_cfg=m.test_cfg, use_img=False, grid_size=grid, feat_channels_lidar=C,
                  lidar_encoder_cfg=enc, with_dpg=False)
        head = build_head(hc).eval()
    finally:
        torch.set_default_dtype(old)
    with torch.no_grad():
        for n, p in list(head.named_parameters()) + list(head.named_buffers()):
            if n.startswith(("encoder_lidar.", "bev_pos_encoder_mlvl_embed.", "bev_level_embeds")):
                p.copy_(torch.from_numpy(detgen.det_param(f"lidarenc.{case}." + n, p.shape)).to(p.dtype))
    return head


def fixture_inputs(case):
    C, grid, B = CASES[case]
    sizes = [(int(grid[0] // 8 / 2 ** l), int(grid[1] // 8 / 2 ** l)) for l in range(4)]
    return [torch.from_numpy(detgen.det(f"lidarenc.{case}.feat{l}", (B, C, H, W), scale=0.5)) for l, (H, W) in enumerate(sizes)]


def fixture_error(case, out, gold):
    """max |out - f64| / max |f64| over the four levels: the normalisation of the stored `e_f32`."""
    want = [gold[f"{case}.out{l}"] for l in range(4)]
    top = max(np.abs(w).max() for w in want)
    return max(np.abs(o.detach().double().cpu().numpy() - w).max() for o, w in zip(out, want)) / top


def _expected_keys(C, F, levels=4, layers=2, heads=8, points=4):
    ns = heads * levels * points
    keys = {"bev_level_embeds": (levels, C)}
    for i in range(layers):
        p = f"encoder_lidar.layers.{i}."
        for name, shape in (("sampling_offsets", (2 * ns, C)), ("attention_weights", (ns, C)), ("value_proj", (C, C)), ("output_proj", (C, C))):
            keys[f"{p}attentions.0.{name}.weight"], keys[f"{p}attentions.0.{name}.bias"] = shape, shape[:1]
        keys[f"{p}ffns.0.layers.0.0.weight"], keys[f"{p}ffns.0.layers.0.0.bias"] = (F, C), (F,)
        keys[f"{p}ffns.0.layers.1.weight"], keys[f"{p}ffns.0.layers.1.bias"] = (C, F), (C,)
        for n in (0, 1):
            keys[f"{p}norms.{n}.weight"], keys[f"{p}norms.{n}.bias"] = (C,), (C,)
    for l in range(levels):
        p = f"bev_pos_encoder_mlvl_embed.{l}.position_embedding_head."
        keys.update({p + "0.weight": (C, 2, 1), p + "0.bias": (C,), p + "1.weight": (C,), p + "1.bias": (C,), p + "1.running_mean": (C,),
                     p + "1.running_var": (C,), p + "1.num_batches_tracked": (), p + "3.weight": (C, C, 1), p + "3.bias": (C,)})
    return keys


@pytest.mark.parametrize("name,C,F", [("srfdet_voxel_nusc_L", 128, 256), ("srfdet_voxel_kitti_L", 256, 512)])
def test_state_dict_keys_and_shapes(name, C, F):
    head = _head(name)
    assert head.with_lidar_encoder
    sd = {k: tuple(v.shape) for k, v in head.state_dict().items() if k.startswith(("encoder_lidar", "bev_"))}
    assert sd == _expected_keys(C, F)
    if name.endswith("kitti_L"):     # the non-square grid: 1600 x 1408 cells -> 200 x 176, 100 x 88, 50 x 44, 25 x 22
        assert head.bev_level_sizes == [(200, 176), (100, 88), (50, 44), (25, 22)]
        assert [tuple(g.shape) for g in head.bev_pos_mlvl] == [(1, 200 * 176, 2), (1, 100 * 88, 2), (1, 50 * 44, 2), (1, 25 * 22, 2)]
    else:
        assert head.bev_level_sizes == [(184, 184), (92, 92), (46, 46), (23, 23)]
    # with the flag off the key set is the parent's: nothing of the encoder, everything else unchanged
    m = workloads.model_cfg(name)
    hc = dict(m.bbox_head)
    hc.update(num_proposals=16, train_cfg=None, test_cfg=m.test_cfg, use_img=False)
    off = build_head(hc)
    assert not off.with_lidar_encoder
    assert set(off.state_dict()) == set(head.state_dict()) - set(sd)
    assert not [k for k in off.state_dict() if k.startswith(("encoder_lidar", "bev_"))]


def test_msda_init_is_the_ring():
    head = _head("srfdet_voxel_nusc_L")
    atts = [m for m in head.modules() if isinstance(m, T.MultiScaleDeformableAttention)]
    assert len(atts) == 2
    for att in atts:
        assert att.num_heads == 8 and att.num_levels == 4 and att.num_points == 4
        assert not att.sampling_offsets.weight.any() and not att.attention_weights.weight.any() and not att.attention_weights.bias.any()
        assert not att.value_proj.bias.any() and not att.output_proj.bias.any()
        assert att.value_proj.weight.abs().max() <= math.sqrt(6.0 / 256) and att.value_proj.weight.std() > 0.05   # xavier uniform
        bias = att.sampling_offsets.bias.detach().view(8, 4, 4, 2)
        for h in range(8):
            th = np.float32(h) * np.float32(2.0 * math.pi / 8)
            c, s = math.cos(th), math.sin(th)
            ring = np.array([c, s]) / max(abs(c), abs(s))
            for p in range(4):
                assert np.allclose(bias[h, :, p].numpy(), ring[None] * (p + 1), rtol=0, atol=1e-6), (h, p)
    assert head.bev_level_embeds.std() > 0.5      # normal_, after the xavier pass


@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_lidar_meets_the_reference_on_the_cpu(case):
    gold = np.load(os.path.join(GOLDEN, "lidar_encoder.npz"))
    e_f32 = float(gold[f"{case}.e_f32"])
    assert 0 < e_f32 < 1e-5
    head = fixture_head(case)
    feats = fixture_inputs(case)
    with torch.no_grad():
        out = head.encode_lidar(feats)
    assert [tuple(o.shape) for o in out] == [tuple(f.shape) for f in feats]
    err = fixture_error(case, out, gold)
    print(case, "float32 CPU error", err, "stored e_f32", e_f32)
    assert err <= e_f32               # the same arithmetic, operation for operation, as the run that measured the figure
    # float64: the encoder is the reference's to rounding (the stored outputs carry 33 mantissa bits)
    head64 = fixture_head(case, torch.float64)
    with torch.no_grad():
        out64 = head64.encode_lidar([f.double() for f in feats])
    err64 = fixture_error(case, out64, gold)
    print(case, "float64 error", err64)
    assert err64 <= 1e-9


def test_disagreeing_pyramid_is_refused():
    head = fixture_head("c128")
    feats = fixture_inputs("c128")
    feats[3] = torch.zeros(2, 128, 2, 2)
    with pytest.raises(ValueError, match=r"2 x 2.*2 x 1"):
        head.encode_lidar(feats)
    with pytest.raises(ValueError, match="BEV maps"):
        head.encode_lidar(feats[:3])


def test_what_the_configs_do_not_use_is_refused_by_name():
    layer = dict(type="BaseTransformerLayer", attn_cfgs=dict(type="MultiScaleDeformableAttention", embed_dims=128),
                 operation_order=("norm", "self_attn", "norm", "ffn"))
    with pytest.raises(NotImplementedError, match="pre-norm"):
        T.build_transformer_layer(layer)
    with pytest.raises(NotImplementedError, match="cross_attn"):
        T.build_transformer_layer(dict(layer, operation_order=("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")))
    with pytest.raises(NotImplementedError, match="MultiheadAttention"):
        T.build_transformer_layer(dict(layer, attn_cfgs=dict(type="MultiheadAttention", embed_dims=128),
                                       operation_order=("self_attn", "norm", "ffn", "norm")))
    att = T.MultiScaleDeformableAttention(embed_dims=32, num_heads=2, num_levels=1, num_points=1)
    q = torch.zeros(6, 1, 32)
    with pytest.raises(NotImplementedError, match="4 components"):
        att(q, reference_points=torch.zeros(1, 6, 1, 4), spatial_shapes=[(2, 3)])
    with pytest.raises(NotImplementedError, match="key_padding_mask"):
        att(q, reference_points=torch.zeros(1, 6, 1, 2), spatial_shapes=[(2, 3)], key_padding_mask=torch.zeros(1, 6, dtype=torch.bool))
