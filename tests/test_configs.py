"""The drop-in boundary on the host: the reference's config files load unchanged, every registry name resolves,
and the built models carry the reference's state_dict keys."""
import json
import os

import pytest
import torch

import srfdet3d_amd as S
from srfdet3d_amd import workloads
from srfdet3d_amd.compat.config import Config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs.json")
with open(GOLDEN) as _f:
    REF_CFGS = json.load(_f)   # the reference's config files as Config.fromfile evaluates them (tests/golden/make_config_fixture.py)
NAMES = {"srfdet_voxel_nusc_L": "configs/nus/srfdet_voxel_nusc_L.py", "srfdet_voxel_nusc_LC": "configs/nus/srfdet_voxel_nusc_LC.py",
         "srfdet_voxel_kitti_L": "configs/kitti/srfdet_voxel_kitti_L.py", "srfdet_dvoxel_waymo_L": "configs/waymo/srfdet_dvoxel_waymo_L.py",
         "srfdet_pillar_nusc_L": "configs/nus/srfdet_pillar_nusc_L.py", "srfdet_voxel_kitti_LC": "configs/kitti/srfdet_voxel_kitti_LC.py",
         "srfdet_pillar_v299_nusc_LC": "configs/nus/srfdet_pillar_v299_nusc_LC.py",
         "srfdet_pillar_r50_nusc_LC": "configs/nus/srfdet_pillar_r50_nusc_LC.py",
         "srfdet_voxel_r50_nusc_LC": "configs/nus/srfdet_voxel_r50_nusc_LC.py", "srfdet_dvoxel_nusc_L": "configs/others/srfdet_dvoxel_nusc_L.py",
         "srfdet_dvoxel_waymo_LC": "configs/others/srfdet_dvoxel_waymo_LC.py"}


def _plain(o):
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    return o


@pytest.mark.parametrize("name", sorted(NAMES))
def test_workload_json_equals_live_reference_config(name):
    ref = REF_CFGS[name]
    assert ref["source"] == NAMES[name]
    assert ref["plugin"] is True and ref["plugin_dir"] == "mmdet3d_plugin"
    assert _plain(workloads._untuple(ref["model"])) == _plain(workloads.model_cfg(name))


def test_config_fromfile_reads_python_config(tmp_path):
    """Config.fromfile on a config written the way the reference's are: module-level dicts / lists / tuples, helper
    variables, an imported module (dropped), attribute access on nested dicts."""
    f = tmp_path / "cfg.py"
    f.write_text("import os\n"
                 "point_cloud_range = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]\n"
                 "voxel_size = [0.075, 0.075, 0.2]\n"
                 "plugin = True\n"
                 "plugin_dir = 'mmdet3d_plugin'\n"
                 "model = dict(type='SRFDet', pts_voxel_layer=dict(max_num_points=10, voxel_size=voxel_size,\n"
                 "             point_cloud_range=point_cloud_range, max_voxels=(120000, 160000)))\n")
    cfg = Config.fromfile(str(f))
    assert cfg.plugin is True and cfg.plugin_dir == "mmdet3d_plugin" and "os" not in cfg
    assert cfg.model.pts_voxel_layer.max_voxels == (120000, 160000)
    assert cfg.model.pts_voxel_layer.point_cloud_range == [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
    assert cfg.filename == str(f)


def test_cfg_options_override():
    m = workloads.model_cfg("srfdet_voxel_nusc_L", **{"bbox_head.num_proposals": 200})
    assert m.bbox_head.num_proposals == 200 and m["pts_voxel_layer"]["max_voxels"] == (120000, 160000)
    c = Config(a=dict(b=[dict(c=1), dict(c=2)]))
    c.merge_from_dict({"a.b.1.c": 5, "a.d.e": "x"})
    assert c.a.b[1]["c"] == 5 and c.a.d.e == "x"


@pytest.mark.parametrize("name,np_,n_params_m", [("srfdet_voxel_nusc_L", 900, None), ("srfdet_voxel_kitti_L", 100, None),
                                                ("srfdet_dvoxel_waymo_L", 900, None)])
def test_models_build_with_reference_key_names(name, np_, n_params_m):
    model = workloads.build(name, np_)
    keys = set(model.state_dict().keys())
    must = ["pts_middle_encoder.conv_input.0.weight", "pts_middle_encoder.conv_out.0.weight", "pts_backbone.blocks.0.0.weight",
            "pts_neck.lateral_convs.0.conv.weight", "pts_neck.fpn_convs.0.bn.running_mean",
            "bbox_head.init_proposal_boxes.weight", "bbox_head.dpg_dw_convs_lidar.0.conv.weight", "bbox_head.dpg_fc1_lidar.weight",
            "bbox_head.head_series_lidar.4.self_attn_lidar.in_proj_weight",
            "bbox_head.head_series_lidar.0.inst_interact_lidar.dynamic_layer.weight",
            "bbox_head.head_series_lidar.0.bboxes_delta_lidar.bias", "bbox_head.code_weights"]
    if "nusc" in name:
        must += ["pts_middle_encoder.encoder_layers.encoder_layer1.0.conv1.weight",
                 "pts_middle_encoder.encoder_layers.encoder_layer1.2.0.weight", "pts_neck.fpn_convs.3.conv.weight"]
    else:
        must += ["pts_voxel_encoder.vfe_layers.0.linear.weight", "pts_voxel_encoder.vfe_layers.0.norm.running_var",
                 "pts_voxel_encoder.cen2point_pos_enc.0.weight"]
    for k in must:
        assert k in keys, k
    sd = model.state_dict()
    if "nusc" in name:
        assert tuple(sd["pts_middle_encoder.conv_input.0.weight"].shape) == (3, 3, 3, 5, 16)
        assert tuple(sd["bbox_head.dpg_fc1_lidar.weight"].shape) == (1024, 23 * 23)
        assert tuple(sd["bbox_head.init_proposal_boxes.weight"].shape) == (4 * 900, 10)
        stage = sum(p.numel() for p in model.bbox_head.head_series_lidar[0].parameters())
        assert stage == 2144596  # parameter count of one reference LiDAR stage at the nusc_L settings
    if "kitti" in name:
        assert tuple(sd["bbox_head.dpg_fc1_lidar.weight"].shape) == (1024, 25 * 22)
        assert sum(p.numel() for p in model.bbox_head.head_series_lidar[0].parameters()) == 12757387


def test_sparse_encoders_have_packed_kernels_for_wide_layers():
    """every sparse convolution with Cout >= 32 of every reference config's SparseEncoderCustom has a packed-weight kernel
    (srf_spconv_fwd_packed): no inference workload runs the unpacked 32- / 64- / 128-channel forms."""
    from srfdet3d_amd import ops
    from srfdet3d_amd.compat.registry import build_middle_encoder
    from srfdet3d_amd.sparse import _SparseConv
    shapes = set()
    for name in sorted(NAMES):
        enc = workloads.model_cfg(name).get("pts_middle_encoder")
        if enc is None or enc["type"] != "SparseEncoderCustom":
            continue
        for m in build_middle_encoder(enc).modules():
            if isinstance(m, _SparseConv) and m.out_channels >= 32:
                K = m.kernel_size[0] * m.kernel_size[1] * m.kernel_size[2]
                assert ops.spconv_packed_supported(K, m.in_channels, m.out_channels), (name, K, m.in_channels, m.out_channels)
                shapes.add((K, m.in_channels, m.out_channels))
    assert {(27, 16, 32), (27, 32, 32), (27, 64, 64), (27, 128, 128), (3, 128, 128)} <= shapes, shapes


def test_lc_head_builds_with_fusion_stage():
    m = workloads.model_cfg("srfdet_voxel_nusc_LC")
    hc = dict(m.bbox_head)
    hc.update(num_proposals=16, train_cfg=None, test_cfg=m.test_cfg, use_img=True)
    head = S.compat.build_head(hc)
    assert sum(p.numel() for p in head.head_series_lidar[0].parameters()) == 2177492
    keys = set(head.state_dict())
    assert {"img_convs.3.weight", "dpg_fc2_img.weight", "head_series_lidar.0.output_fused_proj.weight"} <= keys


@pytest.mark.parametrize("name", ["srfdet_voxel_r50_nusc_LC", "srfdet_dvoxel_nusc_L"])
def test_additional_configs_build(name):
    """every config of the reference except the DCNv2 one builds from its unchanged model dict (the large VoVNet ones are
    built in the GPU tests)."""
    m = workloads.build(name, 16)
    assert sum(p.numel() for p in m.parameters()) > 1e6


def test_dcnv2_definition():
    """compat/dcn.py against the definition: zero offsets + unit mask = plain convolution; integer offsets = a shifted
    tap; fractional offsets = bilinear interpolation with zero padding (checked against an explicit loop)."""
    import torch
    import torch.nn.functional as F
    from srfdet3d_amd.compat.dcn import ModulatedDeformConv2dPack, modulated_deform_conv2d
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 6, 9, 11, generator=g)
    w = torch.randn(4, 6, 3, 3, generator=g)
    Ho, Wo = 5, 6     # stride 2, pad 1
    off0 = torch.zeros(2, 18, Ho, Wo)
    one = torch.ones(2, 9, Ho, Wo)
    torch.testing.assert_close(modulated_deform_conv2d(x, off0, one, w, None, 2, 1), F.conv2d(x, w, None, 2, 1), rtol=1e-5, atol=1e-5)
    off = torch.randn(2, 18, Ho, Wo, generator=g) * 1.5
    m = torch.rand(2, 9, Ho, Wo, generator=g)
    got = modulated_deform_conv2d(x, off, m, w, None, 2, 1)
    want = torch.zeros(2, 4, Ho, Wo)
    H, W = 9, 11
    for n in range(2):
        for ho in range(Ho):
            for wo in range(Wo):
                for t in range(9):
                    i, j = divmod(t, 3)
                    py = ho * 2 - 1 + i + float(off[n, 2 * t, ho, wo])
                    px = wo * 2 - 1 + j + float(off[n, 2 * t + 1, ho, wo])
                    y0, x0 = int(torch.floor(torch.tensor(py))), int(torch.floor(torch.tensor(px)))
                    v = torch.zeros(6)
                    for yy, xx, wt in ((y0, x0, (1 - (py - y0)) * (1 - (px - x0))), (y0, x0 + 1, (1 - (py - y0)) * (px - x0)),
                                       (y0 + 1, x0, (py - y0) * (1 - (px - x0))), (y0 + 1, x0 + 1, (py - y0) * (px - x0))):
                        if 0 <= yy < H and 0 <= xx < W:
                            v = v + wt * x[n, :, yy, xx]
                    want[n, :, ho, wo] += (w[:, :, i, j] @ v) * m[n, t, ho, wo]
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    pack = ModulatedDeformConv2dPack(6, 4, 3, 2, 1, bias=False)
    assert set(pack.state_dict()) == {"weight", "conv_offset.weight", "conv_offset.bias"}
    torch.testing.assert_close(pack(x), 0.5 * F.conv2d(x, pack.weight, None, 2, 1), rtol=1e-5, atol=1e-5)  # sigmoid(0) = 0.5


def test_waymo_lc_config_builds_with_dcn():
    m = workloads.build("srfdet_dvoxel_waymo_LC", 16)
    from srfdet3d_amd.compat.dcn import ModulatedDeformConv2dPack
    bb = m.img_backbone
    assert isinstance(bb.layer3[0].conv2, ModulatedDeformConv2dPack) and not isinstance(bb.layer2[0].conv2, ModulatedDeformConv2dPack)
    assert bb.layer3[0].conv1.stride == (2, 2)   # caffe style: the stride sits on the 1x1


def test_resnet_state_dict_names_follow_mmdet():
    from srfdet3d_amd.compat.registry import build_backbone
    import torch
    r = build_backbone(dict(type="ResNet", depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                            norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, style="pytorch")).eval()
    keys = set(r.state_dict())
    for k in ("conv1.weight", "bn1.running_mean", "layer1.0.downsample.0.weight", "layer1.0.downsample.1.weight",
              "layer3.5.conv2.weight", "layer4.2.bn3.bias"):
        assert k in keys
    assert r.layer2[0].conv2.stride == (2, 2) and r.layer2[0].conv1.stride == (1, 1)      # pytorch style
    assert not r.conv1.weight.requires_grad and not r.layer1[0].conv1.weight.requires_grad and r.layer2[0].conv1.weight.requires_grad
    with torch.no_grad():
        outs = r(torch.zeros(1, 3, 64, 96))
    assert [o.shape[1] for o in outs] == [256, 512, 1024, 2048] and outs[0].shape[-2:] == (16, 24)
