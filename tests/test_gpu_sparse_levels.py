"""One sparse encoder, three ways to index its levels (sparse.Level): hash tables, bitmaps with the sizes read back, bitmaps at fixed
capacities with the index pass on its own stream or not -- the same BEV map bit for bit, and nothing of one call left for the next."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = [41, 128, 128]
HEADROOM = 300


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda:0")


def _encoder(dev):
    from srfdet3d_amd import workloads
    from srfdet3d_amd.compat.registry import build_middle_encoder
    torch.manual_seed(5)
    cfg = workloads.model_cfg("srfdet_voxel_nusc_L")["pts_middle_encoder"]
    assert cfg["block_type"] == "basicblock"
    enc = build_middle_encoder(dict(cfg, sparse_shape=SHAPE, init_cfg=None))
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    return enc.eval().requires_grad_(False).to(dev)


def _voxels(seed, dev, n=5000):
    g = torch.Generator().manual_seed(seed)
    cells = torch.randperm(SHAPE[0] * SHAPE[1] * SHAPE[2], generator=g)[:n]
    z, y, x = cells // (SHAPE[1] * SHAPE[2]), (cells // SHAPE[2]) % SHAPE[1], cells % SHAPE[2]
    coors = torch.stack([torch.zeros_like(z), z, y, x], 1).int()
    return torch.randn(n, 5, generator=g).to(dev), coors.to(dev)


def _maps(enc, feats, coors, monkeypatch):
    """The BEV map of one sample by every route, and of the same voxels dealt to two samples by the two eager routes."""
    out = {}
    two = coors.clone()
    two[:, 0] = torch.arange(coors.shape[0], device=coors.device) % 2
    for name, sort in (("hash", False), ("bitmap", True)):
        enc.spatial_sort = sort
        out[name], out[name + "/2"] = enc(feats, coors, 1), enc(feats, two, 2)
    sizes = [(key, lvl.indices.shape[0]) for key, lvl in enc.forward_levels(feats, coors, 1)[1].chain()]
    assert [k for k, _ in sizes] == ["spconv1", "spconv2", "spconv3", "spconv_down2"] and all(n > 0 for _, n in sizes)
    n = coors.shape[0]
    caps = dict({k: v + HEADROOM for k, v in sizes}, __rows__=torch.tensor([n], dtype=torch.int32, device=coors.device))
    pad_c = torch.cat([coors, torch.full((HEADROOM, 4), -1, dtype=torch.int32, device=coors.device)])
    pad_f = torch.cat([feats, torch.zeros(HEADROOM, feats.shape[1], device=feats.device)])
    for name, env in (("static/stream", None), ("static/one", "0")):
        monkeypatch.delenv("SRF_SPARSE_INDEX_STREAM", raising=False)
        if env is not None:
            monkeypatch.setenv("SRF_SPARSE_INDEX_STREAM", env)
        out[name], counts = enc(pad_f, pad_c, 1, static_caps=caps)
        torch.cuda.synchronize()
        assert [(k, int(c.item()), cap) for k, c, cap in counts] == [(k, v, v + HEADROOM) for k, v in sizes]
    monkeypatch.delenv("SRF_SPARSE_INDEX_STREAM", raising=False)
    return out


def test_every_route_gives_the_same_map_and_no_level_outlives_its_call(dev, monkeypatch):
    enc = _encoder(dev)
    a, b = _voxels(31, dev), _voxels(32, dev)
    with torch.no_grad():
        runs = [_maps(enc, *v, monkeypatch) for v in (a, b, a)]
    for maps in runs:
        assert maps["hash"].shape == (1, 256, 16, 16) and maps["hash/2"].shape == (2, 256, 16, 16)
        assert maps["hash"].abs().sum() > 0 and maps["hash/2"][1].abs().sum() > 0
        for name in ("bitmap", "static/stream", "static/one"):
            assert torch.equal(maps[name], maps["hash"]), name
        assert torch.equal(maps["bitmap/2"], maps["hash/2"])
    assert not torch.equal(runs[0]["hash"], runs[1]["hash"])
    for name, m in runs[2].items():
        assert torch.equal(m, runs[0][name]), name
