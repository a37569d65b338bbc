"""Training the LiDAR BEV encoder on the GPU: with gradients on, `MultiScaleDeformableAttention` runs its sampling core as `ops._MsdaFn`
(srf_msda_fwd / srf_msda_bwd) instead of the torch core, and the gradients of `encode_lidar` are those of the float64 model.

Accuracy: fixture case c128 (the 16 x 12 pyramid, B = 2) in eval mode, loss = sum of the encoded pyramid times a fixed cotangent.  Per
tensor (the four input maps, every encoder, position-embedding and level-embedding parameter) e = max |g - g64| / max |g64| against
`fixture_head(case, dtype=torch.float64)` on the CPU; the GPU's e must be within 4 x the e of the float32 torch route on the host,
computed here.  The margin is the forward test's (tests/test_gpu_lidar_encoder.py), for the same reasons -- the MFMA GEMMs' summation
order and the LayerNorms -- plus the order of the atomics in grad_value."""
import numpy as np
import pytest
import torch

from srfdet3d_amd import ops
from srfdet3d_amd.compat import transformer as T
from test_lidar_encoder_host import CASES, detgen, fixture_head, fixture_inputs

pytestmark = pytest.mark.gpu
CASE = "c128"
PREFIXES = ("encoder_lidar.", "bev_pos_encoder_mlvl_embed.", "bev_level_embeds")
_HOST = {}


def cotangents(feats):
    return [torch.from_numpy(detgen.det(f"lidarenc.{CASE}.cot{l}", f.shape)) for l, f in enumerate(feats)]


def gradients(head, feats, cots):
    """d loss / d (the four maps, the encoder's parameters) for loss = sum_l <encode_lidar(feats)[l], cots[l]> -> {name: tensor}."""
    feats = [f.detach().clone().requires_grad_() for f in feats]
    head.zero_grad(set_to_none=True)
    out = head.encode_lidar(feats)
    sum((o * c).sum() for o, c in zip(out, cots)).backward()
    got = {f"feat{l}": f.grad for l, f in enumerate(feats)}
    got.update({n: p.grad for n, p in head.named_parameters() if n.startswith(PREFIXES)})
    return got


def host(dtype):
    """The CPU gradients of the fixture model in `dtype` (the torch route), computed once."""
    if dtype not in _HOST:
        feats = [f.to(dtype) for f in fixture_inputs(CASE)]
        _HOST[dtype] = gradients(fixture_head(CASE, dtype), feats, [c.to(dtype) for c in cotangents(feats)])
    return _HOST[dtype]


class Spy:
    """Counts the calls of `ops.msda_backward` and of the torch core."""

    def __init__(self, monkeypatch):
        self.node = self.torch = 0
        real_b, real_t = ops.msda_backward, T.multi_scale_deformable_attn_pytorch

        def bwd(*a, **k):
            self.node += 1
            return real_b(*a, **k)

        def core(*a, **k):
            self.torch += 1
            return real_t(*a, **k)
        monkeypatch.setattr(ops, "msda_backward", bwd)
        monkeypatch.setattr(T, "multi_scale_deformable_attn_pytorch", core)


def test_gradients_go_through_the_node_and_meet_float64(dev, monkeypatch):
    spy = Spy(monkeypatch)
    head = fixture_head(CASE).to(dev)
    feats = [f.to(dev) for f in fixture_inputs(CASE)]
    assert not head.training and torch.is_grad_enabled()
    got = gradients(head, feats, [c.to(dev) for c in cotangents(feats)])
    torch.cuda.synchronize()
    layers = len(head.encoder_lidar.layers)
    assert layers == 2 and spy.node == layers and spy.torch == 0        # once per layer, and never the torch core
    g64, g32 = host(torch.float64), host(torch.float32)
    assert sorted(got) == sorted(g64) and len(got) > 4 + 20
    worst = 0.0
    for name in sorted(got):
        top = g64[name].abs().max().item()
        assert got[name] is not None and top > 0, name
        e_gpu = (got[name].double().cpu() - g64[name]).abs().max().item() / top
        e_host = (g32[name].double() - g64[name]).abs().max().item() / top
        print(name, "e_gpu", e_gpu, "e_host_f32", e_host, "ratio", e_gpu / e_host)
        worst = max(worst, e_gpu / e_host)
        assert np.isfinite(e_gpu) and e_gpu <= 4 * e_host, name
    print("largest e_gpu / e_host_f32 over", len(got), "tensors:", worst)


def test_srf_msda_0_takes_the_torch_core(dev, monkeypatch):
    spy = Spy(monkeypatch)
    monkeypatch.setenv("SRF_MSDA", "0")
    head = fixture_head(CASE).to(dev)
    feats = [f.to(dev) for f in fixture_inputs(CASE)]
    got = gradients(head, feats, [c.to(dev) for c in cotangents(feats)])
    assert spy.node == 0 and spy.torch == len(head.encoder_lidar.layers)
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    spy.torch = 0
    monkeypatch.delenv("SRF_MSDA")
    monkeypatch.setenv("SRF_MSDA_TRAIN", "0")          # the training switch alone does the same
    gradients(head, feats, [c.to(dev) for c in cotangents(feats)])
    assert spy.node == 0 and spy.torch == len(head.encoder_lidar.layers)


def test_one_training_step(dev, monkeypatch):
    """train(): dropout is live, so the values are not compared; the step goes through the node and every encoder parameter gets a
    finite gradient."""
    spy = Spy(monkeypatch)
    head = fixture_head(CASE).to(dev).train()
    feats = [f.to(dev) for f in fixture_inputs(CASE)]
    torch.manual_seed(0)
    got = gradients(head, feats, [c.to(dev) for c in cotangents(feats)])
    assert spy.node == len(head.encoder_lidar.layers) and spy.torch == 0
    names = [n for n, _ in head.named_parameters() if n.startswith(PREFIXES)]
    assert names and all(got[n] is not None and torch.isfinite(got[n]).all() and got[n].abs().max() > 0 for n in names)


def test_inference_keeps_the_rows_route(dev, monkeypatch):
    spy = Spy(monkeypatch)
    head = fixture_head(CASE).to(dev)
    feats = [f.to(dev) for f in fixture_inputs(CASE)]
    with torch.no_grad():
        assert head._encode_rows_ok(feats, [tuple(f.shape[2:]) for f in feats])
        before = [o.clone() for o in head.encode_lidar(feats)]
    assert spy.node == 0 and spy.torch == 0
    gradients(head, feats, [c.to(dev) for c in cotangents(feats)])
    assert spy.node == len(head.encoder_lidar.layers)
    head.zero_grad(set_to_none=True)
    with torch.no_grad():
        assert head._encode_rows_ok(feats, [tuple(f.shape[2:]) for f in feats])
        after = head.encode_lidar(feats)
    assert spy.torch == 0 and all(torch.equal(a, b) for a, b in zip(after, before))
