"""LiDAR+camera pieces against fixtures produced by the reference's own Python (tests/golden/fusion_nusc.npz):
VoVNet-99 and the 5-stage fusion decoder (image DPG, img_convs, per-camera RoIs, camera sum, fused projection)."""
import os

import numpy as np
import pytest
import torch

import detgen
from oracle import pipeline
from srfdet3d_amd import synthetic as S, workloads
from srfdet3d_amd.compat.registry import build_head
from srfdet3d_amd.plugin.vovnet import VoVNet

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "fusion_nusc.npz"))
Pc, N_CAM = 16, 6


def test_vovnet99_matches_reference():
    net = VoVNet("V-99-eSE", input_ch=3, out_features=["stage2", "stage3", "stage4", "stage5"]).eval()
    detgen.load_det_params(net, "vov.")
    with torch.no_grad():
        out = net(torch.from_numpy(detgen.det("vov.img", (1, 3, 32, 48))))
    for k, v in out.items():
        ref = GOLD["vov." + k]
        assert tuple(v.shape) == ref.shape
        np.testing.assert_allclose(v.numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())


def lc_head():
    m = workloads.model_cfg("srfdet_voxel_nusc_LC")
    hc = dict(m.bbox_head)
    hc.update(num_proposals=Pc, train_cfg=None, test_cfg=m.test_cfg, use_img=True)
    hd = build_head(hc).eval()
    detgen.load_det_params(hd, "headlc.")
    pf = [torch.from_numpy(detgen.det(f"headlc.feat{i}", (1, 128, s, s), scale=0.5)) for i, s in enumerate((184, 92, 46, 23))]
    imf = [torch.from_numpy(detgen.det(f"headlc.img{i}", (1, N_CAM, 256, h, w), scale=0.5))
           for i, (h, w) in enumerate(((32, 56), (16, 28), (8, 14), (4, 7)))]
    metas = [dict(lidar2img=[m for m in S.camera_rig(f=177.0, cx=112.0, cy=64.0)])]
    return hd, pf, imf, metas


def test_cpu_fusion_head_stage_by_stage_matches_reference():
    hd, pf, imf, metas = lc_head()
    forced = list(zip(GOLD["headlc.stage_in_boxes"], GOLD["headlc.stage_in_prop"]))
    logits, boxes = pipeline.head_forward(hd, imf, pf, metas, stage_inputs=forced)
    np.testing.assert_allclose(boxes.numpy(), GOLD["headlc.boxes"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(logits.numpy(), GOLD["headlc.logits"], rtol=1e-4, atol=2e-4)


@pytest.mark.gpu
def test_gpu_fusion_head_stage_by_stage_matches_reference(dev):
    """HIP box->BEV+6-camera RoIs, HIP gathers on both pyramids, camera sum, fused projection, stage arithmetic."""
    hd, pf, imf, metas = lc_head()
    hd = hd.to(dev)
    pf = [f.to(dev).contiguous(memory_format=torch.channels_last) for f in pf]
    with torch.no_grad():
        imf = [hd.img_convs[i](f.to(dev).flatten(0, 1)).unflatten(0, (1, N_CAM)) for i, f in enumerate(imf)]
    lo = torch.tensor(hd.pc_range[:3], device=dev)
    ext = torch.tensor(hd.pc_range[3:], device=dev) - lo
    for s, stage in enumerate(hd.head_series_lidar):
        bx = torch.from_numpy(GOLD["headlc.stage_in_boxes"][s].copy()).to(dev)
        prop = torch.from_numpy(GOLD["headlc.stage_in_prop"][s].copy()).to(dev)
        with torch.no_grad():
            logits, pred, _ = stage(imf, pf, bx, prop, hd.roi_extractor_lidar, metas, pooler_img=hd.roi_extractor_img)
        pred = pred.clone()
        pred[..., :3] = pred[..., :3] * ext + lo
        np.testing.assert_allclose(pred.cpu().numpy(), GOLD["headlc.boxes"][s], rtol=0, atol=1e-4)
        np.testing.assert_allclose(logits.cpu().numpy(), GOLD["headlc.logits"][s], rtol=1e-4, atol=3e-4)
    # the dynamic proposal generator (LiDAR + image DPG, on this library's GEMM and row-reduction forms): its output is
    # the reference's input of stage 0
    with torch.no_grad():
        ib, ipf = hd._get_init_proposals(imf, pf)
        ib = ib.clone()
        ib[..., :3] = ib[..., :3].sigmoid()
    np.testing.assert_allclose(ib.cpu().numpy(), GOLD["headlc.stage_in_boxes"][0], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(ipf.cpu().numpy().reshape(GOLD["headlc.stage_in_prop"][0].shape), GOLD["headlc.stage_in_prop"][0],
                               rtol=1e-4, atol=2e-5)
    # free-running loop through SRFDetHead.forward (image DPG + img_convs on MIOpen included).  The stage contract
    # (1e-4) is the teacher-forced loop above; here the differences of the proposals (1e-5) and of the img_convs'
    # summation order feed a random-weight stage that amplifies them ~100x, so the first stage is only required to stay
    # within 3e-3 (all five free-running stages at 1e-4 on a damped fixture: test_gpu_decoder_free.py)
    hd2, pf2, imf2, metas2 = lc_head()
    hd2 = hd2.to(dev)
    with torch.no_grad():
        lg, bx = hd2([f.to(dev) for f in imf2], [f.to(dev) for f in pf2], metas2)
    np.testing.assert_allclose(bx.cpu().numpy()[0], GOLD["headlc.boxes"][0], rtol=0, atol=3e-3)


@pytest.mark.gpu
def test_gpu_fusion_stage_bs2_reference_and_corrected_cam_indexing(dev):
    """bs = 2 exposes the reference's image-RoI indexing quirk (SURVEY.md finding 7): by default the HIP path
    reproduces it (checked against the CPU oracle, which follows srfdet_head.py:2520-2547 literally); with
    `corrected_cam_indexing` every sample reads its own cameras, i.e. equals the bs = 1 result of that sample."""
    hd, pf, imf, metas = lc_head()
    hd = hd.to(dev)
    g = torch.Generator().manual_seed(5)
    pf2 = [torch.cat([f, torch.randn(f.shape, generator=g) * 0.5], 0) for f in pf]
    imf2 = [torch.cat([f, torch.randn(f.shape, generator=g) * 0.5], 0) for f in imf]
    metas2 = [metas[0], dict(lidar2img=[m for m in S.camera_rig(f=177.0, cx=100.0, cy=70.0)])]
    bx = torch.from_numpy(np.concatenate([GOLD["headlc.stage_in_boxes"][0], GOLD["headlc.stage_in_boxes"][1]], 0).copy())
    prop = torch.from_numpy(np.concatenate([GOLD["headlc.stage_in_prop"][0], GOLD["headlc.stage_in_prop"][1]], 0).copy())
    stage = hd.head_series_lidar[0]
    with torch.no_grad():
        conv = lambda fs: [hd.img_convs[i](f.to(dev).flatten(0, 1)).unflatten(0, (f.shape[0], N_CAM)) for i, f in enumerate(fs)]
        im_dev = conv(imf2)
        pf_dev = [f.to(dev) for f in pf2]
        lg, pred, _ = stage(im_dev, pf_dev, bx.clone().to(dev), prop.to(dev), hd.roi_extractor_lidar, metas2,
                            pooler_img=hd.roi_extractor_img)
    # sample 1 under the reference indexing reads
    # cameras of BOTH samples, so it differs from its stand-alone result; the corrected indexing restores equality
    with torch.no_grad():
        alone = stage([f[1:2] for f in im_dev], [f[1:2] for f in pf_dev], bx[1:2].clone().to(dev), prop[1:2].to(dev),
                      hd.roi_extractor_lidar, metas2[1:], pooler_img=hd.roi_extractor_img)[1]
        stage.corrected_cam_indexing = True
        fixed = stage(im_dev, pf_dev, bx.clone().to(dev), prop.to(dev), hd.roi_extractor_lidar, metas2,
                      pooler_img=hd.roi_extractor_img)[1]
    assert (pred[1] - alone[0]).abs().max().item() > 1e-3
    torch.testing.assert_close(fixed[1], alone[0], rtol=0, atol=1e-4)


def test_pillar_feature_net_matches_reference():
    from srfdet3d_amd.plugin.pillar import PillarFeatureNetCustom
    pfn = PillarFeatureNetCustom(in_channels=5, feat_channels=[64], with_distance=False, voxel_size=[0.2, 0.2, 8],
                                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01),
                                 point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], legacy=False).eval()
    detgen.load_det_params(pfn, "pfn.")
    Np, Mp = 60, 20
    num = (np.arange(Np) % Mp + 1).astype(np.int32)
    vox = (detgen.det("pfn.voxels", (Np, Mp, 5)) * (np.arange(Mp)[None, :, None] < num[:, None, None])).astype(np.float32)
    pc = np.stack([np.zeros(Np), np.zeros(Np), np.arange(Np) % 512, (np.arange(Np) * 7) % 512], 1).astype(np.int32)
    with torch.no_grad():
        out = pfn(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(pc))
    np.testing.assert_allclose(out.numpy(), GOLD["pfn.out"], rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_pillar_config_runs_end_to_end(dev):
    """configs/nus/srfdet_pillar_nusc_L.py: 20-point pillars on a 512 x 512 grid, PointPillarsScatter, 3-block SECOND."""
    from oracle import oracle as O
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    torch.manual_seed(0)
    model = workloads.build("srfdet_pillar_nusc_L", 64).eval().to(dev)
    pts = S.nuscenes_sweep(2000)
    p = torch.from_numpy(pts).to(dev)
    with torch.no_grad():
        voxels, num, coors = model.voxelize([p])
        v, c, n = O.hard_voxelize(pts, [0.2, 0.2, 8], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], 20, 40000)
        np.testing.assert_array_equal(coors[:, 1:].cpu().numpy(), c)
        np.testing.assert_array_equal(num.cpu().numpy(), n)
        assert voxels.cpu().numpy().tobytes() == v.tobytes()
        feats = model.pts_voxel_encoder(voxels, num, coors)
        canvas = model.pts_middle_encoder(feats, coors, 1)
        assert canvas.shape == (1, 64, 512, 512)
        ref = O.densify(feats.cpu().numpy(), np.concatenate([coors[:, :1].cpu().numpy(), np.zeros((len(c), 1), np.int32), c[:, 1:]], 1).astype(np.int32), 1, [1, 512, 512])
        np.testing.assert_array_equal(canvas.cpu().numpy(), ref.reshape(1, 64, 512, 512))
        res = model.simple_test(None, [p], [dict(box_type_3d=LiDARInstance3DBoxes)])
    assert set(res[0]["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"}
