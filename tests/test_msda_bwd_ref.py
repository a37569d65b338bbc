"""The float64 definition of tests/msda_bwd_ref.py (no GPU): it is torch's float64 autograd through `multi_scale_deformable_attn_pytorch`
wherever the two rules agree, and the conditions tests/test_gpu_msda_bwd.py relies on hold on the reference alone."""
import numpy as np
import pytest
import torch

import msda_bwd_ref as R
from srfdet3d_amd.compat.transformer import multi_scale_deformable_attn_pytorch

# cases whose grad_logits is 0 by construction: one sample per (query, head) (the softmax is the constant 1), or one level with every row
# planted, so that the P samples of a (query, head) share one position and t[j] = sum_j a[j] t[j].  There the bound is held against the
# largest magnitude sum Ml instead of the tensor's largest entry.
FLAT_LOGITS = ("d16_one_map_p1", "d32_one_map_q3")
FAULT_CASE = "d16_two_levels_p3"
FAULTS = {"corners": ("grad_offs", "grad_logits"), "sign": ("grad_offs",), "start": ("grad_value", "grad_offs", "grad_logits"),
          "softmax": ("grad_logits",)}


def _compared(name, key):
    """Elements of gradient `key` the GPU test compares: everything, less the kink samples for grad_offs."""
    _, ref = R.reference(name)
    keep = np.ones(ref[key].shape, dtype=bool)
    if key == "grad_offs":
        keep = np.repeat(~ref["kink"].reshape(ref["kink"].shape[0], -1), 2, axis=1)
    return keep


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_is_torch_float64_autograd(name):
    """locations = ref + offs / (W, H) with offs as the leaf.  Non-finite offsets are replaced by 1e6 pixels for torch (far outside: no
    contribution and a zero gradient under both rules); the samples exactly on an integer coordinate or box edge, where grid_sample's
    backward takes another one-sided derivative, are left out of the offset gradient."""
    heads, d, shapes, B, Q, P, _, _, _ = R.CASES[name]
    case, ref = R.reference(name)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    rows = case["ref"].shape[0]
    Q = rows // B
    offs64 = case["offs"].astype(np.float64)
    replaced = ~np.isfinite(offs64).all(-1)
    offs64[replaced] = 1e6
    value = torch.from_numpy(case["value"].astype(np.float64)).view(B, S, heads, d).requires_grad_()
    offs = torch.from_numpy(offs64).view(B, Q, heads, L, P, 2).requires_grad_()
    logits = torch.from_numpy(case["logits"].astype(np.float64)).view(B, Q, heads, L * P).requires_grad_()
    refp = torch.from_numpy(case["ref"].astype(np.float64)).view(B, Q, L, 2)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    loc = refp[:, :, None, :, None, :] + offs / norm[None, None, None, :, None, :]
    out = multi_scale_deformable_attn_pytorch(value, shapes, loc, logits.softmax(-1).view(B, Q, heads, L, P))
    (out * torch.from_numpy(case["grad_out"].astype(np.float64)).view(B, Q, heads * d)).sum().backward()
    got = dict(grad_value=value.grad.reshape(B * S, heads * d).numpy(), grad_offs=offs.grad.reshape(rows, -1).numpy(),
               grad_logits=logits.grad.reshape(rows, -1).numpy())
    skip = np.repeat((ref["on_grid"] | replaced).reshape(rows, -1), 2, axis=1)
    for key, g in got.items():
        keep = ~skip if key == "grad_offs" else np.ones(g.shape, dtype=bool)
        top = ref["Ml"].max() if key == "grad_logits" and name in FLAT_LOGITS else max(np.abs(g).max(), np.abs(ref[key]).max())
        err =np.abs(g - ref[key])[keep].max()
        print(name, key, "max |ref - torch64|", err, "largest entry", top, "compared", int(keep.sum()), "of", keep.size)
        assert keep.sum() > 0
        assert err <= 1e-12 * top
    assert (ref["grad_offs"][np.repeat(replaced.reshape(rows, -1), 2, axis=1)] == 0).all()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_conditions_of_the_gpu_test(name):
    case, ref = R.reference(name)
    bd = R.bounds(name)
    assert all(np.isfinite(ref[k]).all() for k in ("grad_value", "grad_offs", "grad_logits"))
    print(name, "kink samples", int(ref["kink"].sum()), "of", ref["counted"], "counted; most adds per destination", int(ref["Nv"].max()),
          "T", bd["T"])
    assert ref["kink"].sum() <= 1e-3 * ref["counted"]
    for key in ("grad_value", "grad_offs", "grad_logits"):
        keep = _compared(name, key)
        top = np.abs(ref[key]).max()
        if key == "grad_logits" and name in FLAT_LOGITS:
            assert top <= 1e-12 * ref["Ml"].max()
            top = ref["Ml"].max()
        print(name, key, "max bound", bd[key][keep].max(), "largest entry", top, "ratio", bd[key][keep].max() / top)
        assert top > 1e-2 and bd[key][keep].max() < 1e-3 * top


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_errors_exceed_the_bound(fault):
    heads, _, shapes, _, _, P, _, _, _ = R.CASES[FAULT_CASE]
    case, ref = R.reference(FAULT_CASE)
    bd = R.bounds(FAULT_CASE)
    bad = R.msda_bwd_ref(case["value"], shapes, case["ref"], case["offs"], case["logits"], heads, P, case["grad_out"], fault=fault)
    for key in FAULTS[fault]:
        keep = _compared(FAULT_CASE, key)
        over = (np.abs(bad[key] - ref[key]) / np.maximum(bd[key], 1e-300))[keep]
        print(fault, key, "largest planted error / bound", over.max(), "elements over the bound", int((over > 1).sum()), "of", over.size)
        assert over.max() > 100 and (over > 1).mean() > 0.05
