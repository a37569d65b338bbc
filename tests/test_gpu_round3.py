"""Round-3 GPU tests asked for by VERDICT r2:

* the reference's VoVNet fixture (`vov.stage2..5`, produced by the reference's own vovnet.py: tests/golden/make_fixtures.py)
  on the HIP channels-last executor -- the kernels that are 90 % of the LC frame met it only through the torch modules before;
* one LC training step at BASELINE.json config 4's real per-GPU shape (bs = 2, 6 x 928 x 1600 per frame, np = 900, 30k points);
* the LC three-graph frame captured, replayed and destroyed twice in one process (what the product shares
  with the experiment that once crashed, and why it is safe);
* the implicit-im2col GEMM on a batch whose input exceeds one 32-bit buffer descriptor."""
import copy
import gc
import os

import numpy as np
import pytest
import torch

import detgen
from srfdet3d_amd import nhwc, ops, synthetic as S, workloads
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
from srfdet3d_amd.plugin import training
from srfdet3d_amd.plugin.vovnet import VoVNet

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "fusion_nusc.npz"))


@pytest.mark.parametrize("wino43", ["1", "0"])
def test_vovnet99_reference_fixture_on_the_hip_kernels(dev, monkeypatch, wino43):
    """`vov.img` through nhwc.vovnet_forward (srf_stem_conv_nchw, srf_wino43 / srf_wino3x3, srf_conv_gemm_nhwc,
    srf_conv1x1_nhwc_pooled, srf_ese_gate, srf_nhwc_affine, srf_nhwc_maxpool3s2) against the stage outputs the reference's
    VoVNet (vovnet.py:269-374) produced for the same weights and image: 2e-4 of each map's maximum."""
    monkeypatch.setenv("SRF_WINO43", wino43)
    net = VoVNet("V-99-eSE", input_ch=3, out_features=["stage2", "stage3", "stage4", "stage5"]).eval()
    detgen.load_det_params(net, "vov.")
    net = net.to(dev)
    x = torch.from_numpy(detgen.det("vov.img", (1, 3, 32, 48))).to(dev)
    with torch.no_grad():
        assert nhwc.vovnet_supported(net, x)
        out = nhwc.vovnet_forward(net, x)
    assert list(out) == ["stage2", "stage3", "stage4", "stage5"]
    for k, v in out.items():
        ref = GOLD["vov." + k]
        assert tuple(v.shape) == ref.shape and v.stride(1) == 1      # logical NCHW, channels-last strides
        err = np.abs(v.cpu().numpy() - ref).max()
        assert err <= 2e-4 * np.abs(ref).max(), (k, err, np.abs(ref).max())


def test_lc_training_step_at_config4_shape(dev):
    """BASELINE.json configs[3] on one GPU at its real per-GPU shape: srfdet_voxel_nusc_LC, bs = 2, six 928 x 1600 views per
    frame, np = 900 (the config's own), 30k-point sweeps, LiDAR branch frozen (tools/train.py:220-234), VoVNet with
    frozen_stages = 2 / norm_eval (vovnet.py:354-374): forward_train -> loss_ota -> backward -> clip -> AdamW.  Size-independent
    properties: the full loss dict, finite positive losses, finite non-zero gradients on parameters of every trainable part,
    none on the frozen ones, parameters move, a second step runs."""
    torch.manual_seed(0)
    model = workloads.build("srfdet_voxel_nusc_LC", 900, train=True)
    training.freeze_lidar_components(model)
    model = model.to(dev).train()
    rng = np.random.default_rng(0)
    rig = [m for m in S.camera_rig()]
    pts = [torch.from_numpy(S.nuscenes_sweep(2000 + i)).to(dev) for i in range(2)]
    assert all(p.shape[0] >= 25000 for p in pts)
    img = torch.cat([torch.from_numpy(S.camera_images(3000 + i)) for i in range(2)], 0).to(dev)
    assert tuple(img.shape) == (2, 6, 3, 928, 1600)
    gtb, gtl = [], []
    for i in range(2):
        n = 20
        b = np.concatenate([rng.uniform(-45, 45, (n, 2)), rng.uniform(-2.5, -0.5, (n, 1)), rng.uniform([1.5, 3.5, 1.4], [2.2, 5.0, 2.0], (n, 3)),
                            rng.uniform(-np.pi, np.pi, (n, 1)), rng.normal(0, 1, (n, 2))], 1)
        gtb.append(LiDARInstance3DBoxes(torch.tensor(b, dtype=torch.float32, device=dev), box_dim=9))
        gtl.append(torch.from_numpy(rng.integers(0, 10, n)).to(dev))
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=rig) for _ in range(2)]
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=0.01)
    named = dict(model.named_parameters())
    probe = "bbox_head.head_series_lidar.0.output_fused_proj.weight"
    before = named[probe].detach().clone()
    for it in range(2):
        losses = model(return_loss=True, img=img, points=pts, img_metas=metas, gt_bboxes_3d=gtb, gt_labels_3d=gtl)
        assert set(losses) == {"loss_cls", "loss_bbox"} | {f"s.{i}.{n}" for i in range(4) for n in ("loss_cls", "loss_bbox")}
        vals = {k: float(v.detach()) for k, v in losses.items()}
        assert all(np.isfinite(v) and v > 0 for v in vals.values()), vals
        opt.zero_grad(set_to_none=True)
        sum(losses.values()).backward()
        for k in (probe, "bbox_head.head_series_lidar.4.bboxes_delta_lidar.weight", "bbox_head.img_convs.0.weight",
                  "img_neck.fpn_convs.0.conv.weight", "img_neck.lateral_convs.3.conv.weight", "bbox_head.init_proposal_boxes.weight"):
            gr = named[k].grad
            assert gr is not None and torch.isfinite(gr).all() and gr.abs().sum() > 0, k
        trainable_backbone = [n for n, p in named.items() if n.startswith("img_backbone.") and p.requires_grad]
        assert trainable_backbone and not any(n.split(".")[1] in ("stem", "stage2", "stage3") for n in trainable_backbone)
        assert any(named[n].grad is not None and named[n].grad.abs().sum() > 0 for n in trainable_backbone if "stage5" in n)
        assert all(p.grad is None for n, p in named.items() if n.startswith("pts_"))
        assert all(p.grad is None for n, p in named.items() if n.startswith("img_backbone.stem"))
        torch.nn.utils.clip_grad_norm_(params, 35.0)
        opt.step()
    assert not torch.equal(named[probe].detach(), before)
    del model, opt, losses
    gc.collect()
    torch.cuda.empty_cache()


def _randomize_bn(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def test_lc_three_graph_frame_capture_replay_destroy_twice(dev):
    """The LC frame is three hipGraphs: the camera graph (captured on a side stream, with the coarse FPN chains forked onto
    further streams INSIDE the capture, i.e. events recorded and waited on while capturing), the BEV half, and the decoder half
    captured into the BEV half's memory pool.  Capture -> validate -> replay several frames -> destroy everything -> capture
    again in the same process -> replay: identical pre-NMS tensors both times, and equal to the eager frame."""
    torch.manual_seed(2)
    cpu = workloads.build("srfdet_voxel_nusc_LC", 48).eval()
    _randomize_bn(cpu, 2)
    cpu.bbox_head.test_cfg = dict(cpu.bbox_head.test_cfg, score_thr=0.02)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig(f=1266.0 * 256 / 1600, cx=128.0, cy=80.0)])]
    img = torch.from_numpy(S.camera_images(3000, h=160, w=256)).to(dev)
    frames = [torch.from_numpy(S.nuscenes_sweep(2000 + i, 12000)).to(dev) for i in range(3)]
    eager = copy.deepcopy(cpu).to(dev)
    with torch.no_grad():
        want = []
        for p in frames:
            mt = copy.deepcopy(metas)
            img_feats, pt_feats = eager.extract_feat(img, [p], mt)
            want.append([t.clone() for t in eager.bbox_head.decode(*eager.bbox_head(img_feats, pt_feats, mt))])
    results = []
    for life in range(2):
        g = copy.deepcopy(cpu).to(dev).enable_hip_graphs(img_overlap=True, whole_frame=True)
        with torch.no_grad():
            g.simple_test(img, [frames[0]], copy.deepcopy(metas))      # eager pass + the three captures
            assert g._graphed_frame.entry is not None and g._graphed_frame.entry["head_graph"] is not None
            assert len(g._graphed_img.entries) == 1
            got = []
            for rep in range(2):
                for p in frames:
                    g.simple_test(img, [p], copy.deepcopy(metas))
                    e = g._graphed_frame.entry
                    got.append((e["scores"].clone(), e["boxes"].clone()))
        torch.cuda.synchronize()
        assert g._graphed_frame.stats["replays"] >= 6
        results.append(got)
        # destroy: the graphs, their shared pool and every static buffer
        g._graphed_frame = g._graphed_img = g._graphed_tail = None
        del g, e
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    for (s0, b0), (s1, b1) in zip(*results):
        assert torch.equal(s0, s1) and torch.equal(b0, b1)              # second life = first life, bit for bit
    for i, (s, b) in enumerate(results[0]):
        w = want[i % len(frames)]
        torch.testing.assert_close(s, w[0], rtol=0, atol=1e-5)
        torch.testing.assert_close(b, w[1], rtol=2e-5, atol=1e-4)


def test_conv_gemm_nhwc_batch_beyond_one_descriptor(dev):
    """N H W x_ld 4 >= 2^31 bytes of input (VoVNet stem_3 at 23+ camera images: LC inference at batch 4): the wrapper runs the
    batch in image groups; every image equals the same layer run on that image alone."""
    N, H, W, C = 5, 464, 800, 320            # 5 x 475 MB: two groups of two images and one of one
    assert 4 * N * H * W * C >= (1 << 31)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, C, generator=g).to(dev)[..., :32]      # a 32-channel slice of a 320-channel buffer
    assert ops.conv_gemm_nhwc_supported(x)
    w = (torch.randn(32, 32, 3, 3, generator=g) / 17).to(dev)
    pk = ops.pack_conv_gemm_weights(w)
    y = ops.conv_gemm_nhwc(x, pk, 32, (3, 3), 2, 1, None, None, True)
    for n in (0, 2, 4):
        y1 = ops.conv_gemm_nhwc(x[n:n + 1], pk, 32, (3, 3), 2, 1, None, None, True)
        assert torch.equal(y[n:n + 1], y1)
    assert (y > 0).float().mean().item() > 0.2


def test_blockwise_nms_equals_one_launch(dev):
    """More candidates of one class than a srf_nms_rotated launch takes (4096) run as an exact blockwise greedy NMS
    (postprocess._nms_rotated_blocks: survivors thin the next block through srf_box_iou_rotated, the block then thins itself).
    With a small block size on 3000 boxes it must keep exactly what one launch keeps, in the same order."""
    from srfdet3d_amd import postprocess
    g = torch.Generator().manual_seed(4)
    n = 3000
    bev = torch.cat([torch.rand(n, 2, generator=g) * 60 - 30, torch.rand(n, 2, generator=g) * 4 + 1, torch.rand(n, 1, generator=g) * 6.28 - 3.14], 1).to(dev)
    scores = torch.rand(n, generator=g).to(dev)
    want = ops.nms_rotated(bev, scores, 0.2)
    assert 200 < want.numel() < n - 200
    for block in (257, 1024):
        got = postprocess._nms_rotated_blocks(bev, scores, 0.2, block=block)
        assert torch.equal(got, want)
    # and through the public entry point: 5000 boxes of ONE class above the threshold
    n = 5000
    boxes = torch.cat([torch.rand(n, 2, generator=g) * 100 - 50, torch.zeros(n, 1), torch.rand(n, 2, generator=g) * 4 + 1, torch.ones(n, 1),
                       torch.rand(n, 1, generator=g) * 6.28 - 3.14], 1).to(dev)
    sc = torch.zeros(n, 3)
    sc[:, 1] = torch.rand(n, generator=g) * 0.5 + 0.5
    b, s_, l = postprocess._per_class_nms(boxes, sc.to(dev), 0.1, 10 ** 6, 0.2)
    ref = postprocess._nms_rotated_blocks(boxes[:, [0, 1, 3, 4, 6]].contiguous(), sc[:, 1].to(dev), 0.2, block=4096)
    assert torch.equal(b, boxes[ref]) and bool((l == 1).all())
    # the greedy property against the float64 IoU of tests/rotated_iou_ref.py (not the kernel's own): no two kept boxes overlap
    # above the threshold (all kept x kept pairs), and a dropped box has a kept box of HIGHER score above it (500 dropped boxes)
    import rotated_iou_ref as R
    bev64 = boxes[:, [0, 1, 3, 4, 6]].cpu().numpy()
    kept = ref.cpu().numpy()
    kk = R.iou(bev64[kept], bev64[kept])
    np.fill_diagonal(kk, 0)
    assert float(kk.max()) <= 0.2 + 1e-5
    dropped = np.setdiff1d(np.arange(n), kept)
    assert dropped.size > 500
    dropped = np.random.default_rng(0).choice(dropped, 500, replace=False)
    s1 = sc[:, 1].numpy()
    iou = R.iou(bev64[kept], bev64[dropped])
    iou[s1[kept][:, None] <= s1[dropped][None, :]] = 0          # only a kept box of higher score suppresses
    assert bool((iou.max(axis=0) > 0.2 - 1e-5).all())


@pytest.mark.parametrize("fork_from", ["0", "2"])
def test_fpn_forward_with_level_consumer_capture_equals_eager(dev, monkeypatch, fork_from):
    """nhwc.fpn_forward with a per-level consumer (the head's img_convs as the tail of each level's chain): captured into a
    hipGraph -- where the chains of the levels >= SRF_FPN_FORK fork onto side streams (2), or none does (0) -- the replay must
    equal the eager result bit for bit, and both the plain two-step form (FPN, then the consumer on every level)."""
    from srfdet3d_amd.compat.necks import FPN
    monkeypatch.setenv("SRF_FPN_FORK", fork_from)
    torch.manual_seed(3)
    fpn = FPN(in_channels=[64, 96, 128, 160], out_channels=64, num_outs=4).to(dev).eval()
    convs = torch.nn.ModuleList([torch.nn.Conv2d(64, 32, 3, padding=1) for _ in range(4)]).to(dev).eval()
    sizes = [(40, 64), (20, 32), (10, 16), (5, 8)]
    feats = [torch.randn(2, c, h, w, device=dev).contiguous(memory_format=torch.channels_last) for c, (h, w) in zip([64, 96, 128, 160], sizes)]
    consumer = lambda i, x: nhwc.conv3x3(x, convs[i])  # noqa: E731
    with torch.no_grad():
        assert nhwc.fpn_supported(fpn, feats)
        plain = [nhwc.nchw_view(nhwc.conv3x3(nhwc.nhwc_view(o), convs[i])) for i, o in enumerate(nhwc.fpn_forward(fpn, feats))]
        with nhwc.level_consumer(fpn, consumer):
            eager = nhwc.fpn_forward(fpn, feats)
        assert isinstance(eager, nhwc.ConsumedLevels) and getattr(fpn, "_srf_level_consumer", None) is None
        for a, b in zip(eager, plain):
            assert torch.equal(a, b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side), nhwc.level_consumer(fpn, consumer):
            got = nhwc.fpn_forward(fpn, feats)
        for rep in range(2):
            for o in got:
                o.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(got, eager):
                assert torch.equal(a, b)


def test_stair_nhwc_equals_the_module_stair(dev):
    """SRFDetHead._stair_nhwc (the depthwise stair of the proposal generator on channels-last levels: srf_nhwc_dwconv3x3s2 writing
    slices of the next level's concat buffer) against the module stair (Conv2d + BN + ReLU, torch.cat) of srfdet_head.py:520-537."""
    from srfdet3d_amd.compat.cnn import ConvModule
    from srfdet3d_amd.plugin.heads import SRFDetHead
    torch.manual_seed(1)
    chans = [16, 32, 48]
    convs = torch.nn.ModuleList([ConvModule(c, c, kernel_size=3, stride=2, padding=1, groups=c, norm_cfg=dict(type="BN2d", eps=1e-3, momentum=0.01))
                                 for c in chans]).to(dev).eval()
    _randomize_bn(convs, 3)
    feats = [torch.randn(2, 16, 32, 48, device=dev), torch.randn(2, 16, 16, 24, device=dev), torch.randn(2, 16, 8, 12, device=dev)]
    with torch.no_grad():
        x = convs[0](feats[0])
        for lvl in range(1, len(feats)):
            x = torch.cat([feats[lvl], x], dim=1)
            if lvl < len(convs):
                x = convs[lvl](x)
        cl = [f.contiguous(memory_format=torch.channels_last) for f in feats]
        got = SRFDetHead._stair_nhwc(list(convs), cl)
    assert got.shape == x.shape
    torch.testing.assert_close(got, x, rtol=1e-5, atol=1e-5)


def test_packed_weight_caches_are_dropped_on_mode_switch(dev):
    """nhwc caches key on (weight._version, data_ptr); an update through `.data` changes neither.  `train()` / `eval()` and
    `load_state_dict` of the detector call nhwc.invalidate_caches, after which the next pass packs the new weights."""
    conv = torch.nn.Conv2d(96, 32, 3, padding=1, bias=False).to(dev)
    x = torch.randn(1, 8, 12, 96, device=dev)
    with torch.no_grad():
        y0 = nhwc.conv3x3(x, conv).clone()
        conv.weight.data.mul_(2.0)                       # invisible to the cache key
        assert torch.equal(nhwc.conv3x3(x, conv), y0)    # stale on purpose: this is what the invalidation is for
        holder = torch.nn.Sequential(conv)
        nhwc.invalidate_caches(holder)
        y1 = nhwc.conv3x3(x, conv)
    torch.testing.assert_close(y1, 2 * y0, rtol=1e-5, atol=1e-6)


def test_lc_frame_at_full_size_graphs_equal_eager(dev):
    """The headline configuration at the headline size (30k points, six 928 x 1600 views, np = 200): the three-graph frame
    (camera graph beside the BEV half, decoder half after the join) against the eager frame -- pre-NMS scores within 1e-5, box
    parameters within 1e-4 (the contract of north_star), on two different sweeps and on replays."""
    torch.manual_seed(0)
    cpu = workloads.build("srfdet_voxel_nusc_LC", 200).eval()
    _randomize_bn(cpu, 0)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig()])]
    img = torch.from_numpy(S.camera_images(3000)).to(dev)
    frames = [torch.from_numpy(S.nuscenes_sweep(2000 + i)).to(dev) for i in range(2)]
    eager = copy.deepcopy(cpu).to(dev)
    with torch.no_grad():
        want = []
        for p in frames:
            mt = copy.deepcopy(metas)
            img_feats, pt_feats = eager.extract_feat(img, [p], mt)
            want.append([t.clone() for t in eager.bbox_head.decode(*eager.bbox_head(img_feats, pt_feats, mt))])
    del eager
    g = copy.deepcopy(cpu).to(dev).enable_hip_graphs(img_overlap=True, whole_frame=True)
    with torch.no_grad():
        g.simple_test(img, [frames[0]], copy.deepcopy(metas))          # eager pass + captures
        for rep in range(2):
            for p, w in zip(frames, want):
                g.simple_test(img, [p], copy.deepcopy(metas))
                e = g._graphed_frame.entry
                torch.testing.assert_close(e["scores"], w[0], rtol=0, atol=1e-5)
                torch.testing.assert_close(e["boxes"], w[1], rtol=2e-5, atol=1e-4)
    assert g._graphed_frame.stats["replays"] >= 4
    g._graphed_frame = g._graphed_img = g._graphed_tail = None
    del g
    gc.collect()
    torch.cuda.empty_cache()


def test_graphs_are_recaptured_when_the_packed_weights_are_dropped(dev):
    """`eval()` / `train()` / `load_state_dict` drop the packed-weight images (nhwc.invalidate_caches); a captured
    hipGraph holds their raw pointers, so the graphs must go with them.  Capture, switch modes, let the allocator hand the freed
    blocks to something else, run again: the frame must equal the eager frame, not read recycled memory as weights."""
    torch.manual_seed(0)
    cpu = workloads.build("srfdet_voxel_nusc_L", 32).eval()
    _randomize_bn(cpu, 0)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)]
    pts = torch.from_numpy(S.nuscenes_sweep(2000, 8000)).to(dev)
    eager = copy.deepcopy(cpu).to(dev)
    with torch.no_grad():
        f = eager.extract_point_features([pts])
        want = [t.clone() for t in eager.bbox_head.decode(*eager.bbox_head(None, f, metas))]
    g = copy.deepcopy(cpu).to(dev).enable_hip_graphs(whole_frame=True)
    with torch.no_grad():
        for _ in range(3):
            g.simple_test(None, [pts], copy.deepcopy(metas))
        first = g._graphed_frame
        assert first.stats["replays"] >= 1
        g.eval()                                           # nothing changed (same mode, same parameter tensors and versions): kept
        assert g._graphed_frame is first
        g.train()
        g.eval()                                           # a mode switch drops the packed weights -> must drop the graphs too
        assert g._graphed_frame is not first and g._graphed_frame.entry is None
        junk = [torch.full((1 << 20,), float("nan"), device=dev) for _ in range(64)]   # recycle the freed blocks
        for _ in range(3):
            g.simple_test(None, [pts], copy.deepcopy(metas))
        e = g._graphed_frame.entry
        assert g._graphed_frame.stats["replays"] >= 1
        torch.testing.assert_close(e["scores"], want[0], rtol=0, atol=1e-5)
        torch.testing.assert_close(e["boxes"], want[1], rtol=2e-5, atol=1e-4)
        sd = {k: v.clone() for k, v in g.state_dict().items()}
        g.load_state_dict(sd)
        assert g._graphed_frame.entry is None
    del junk
    g._graphed_frame = g._graphed_img = g._graphed_tail = None
    del g
    gc.collect()
    torch.cuda.empty_cache()
