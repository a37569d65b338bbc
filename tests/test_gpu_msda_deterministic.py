"""SRF_DETERMINISTIC=1 and the LiDAR BEV encoder: `grad_value` of the deformable attention exists only as float atomics
(srf_msda_bwd on the HIP node, grid_sample's backward on the torch core), so a training pass raises instead of running a
non-reproducible kernel quietly.  With the switch unset the encoder trains as before."""
import pytest
import torch

from test_gpu_lidar_encoder_train import CASE, PREFIXES, cotangents, gradients
from test_lidar_encoder_host import fixture_head, fixture_inputs

pytestmark = pytest.mark.gpu


def test_the_encoder_training_pass_raises_under_the_switch(dev, monkeypatch):
    head = fixture_head(CASE).to(dev).train()
    feats = [f.to(dev) for f in fixture_inputs(CASE)]
    cots = [c.to(dev) for c in cotangents(feats)]
    monkeypatch.setenv("SRF_DETERMINISTIC", "1")
    for torch_core in (False, True):                                         # the HIP node and the torch core alike
        if torch_core:
            monkeypatch.setenv("SRF_MSDA_TRAIN", "0")
        with pytest.raises(RuntimeError, match=r"SRF_DETERMINISTIC.*srf_msda_bwd|srf_msda_bwd.*SRF_DETERMINISTIC"):
            gradients(head, feats, cots)
    monkeypatch.delenv("SRF_MSDA_TRAIN")
    with torch.no_grad():                                                    # no gradient recorded: nothing to refuse
        assert all(torch.isfinite(o).all() for o in head.encode_lidar(feats))
    monkeypatch.delenv("SRF_DETERMINISTIC")
    got = gradients(head, feats, cots)                                       # unset: as before
    names = [n for n, _ in head.named_parameters() if n.startswith(PREFIXES)]
    assert names and all(got[n] is not None and torch.isfinite(got[n]).all() for n in names)
