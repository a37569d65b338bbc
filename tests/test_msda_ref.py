"""The float64 definition of multi-scale deformable attention (tests/msda_ref.py) against torch's grid_sample composed as mmcv's pure-torch
function, and against cases small enough to work out by hand.  No GPU."""
import numpy as np
import pytest
import torch

from msda_ref import PYRAMID, make_case, msda_ref
from srfdet3d_amd.compat.transformer import multi_scale_deformable_attn_pytorch


def _torch64(case, shapes, heads, P):
    """The same operator through grid_sample (float64, bilinear, zeros, align_corners=False), as the module composes it."""
    value, ref, offs, logits = (torch.from_numpy(case[k]).double() for k in ("value", "ref", "offs", "logits"))
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    B = value.shape[0] // S
    Q = ref.shape[0] // B
    d = value.shape[1] // heads
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    loc = ref.view(B, Q, 1, L, 1, 2) + offs.view(B, Q, heads, L, P, 2) / norm[None, None, None, :, None, :]
    attn = logits.view(B, Q, heads, L * P).softmax(-1).view(B, Q, heads, L, P)
    return multi_scale_deformable_attn_pytorch(value.view(B, S, heads, d), shapes, loc, attn).reshape(B * Q, heads * d).numpy()


@pytest.mark.parametrize("shapes,B,P,d", [(PYRAMID, 2, 4, 16), ([(5, 7)], 1, 1, 32), ([(5, 7)], 3, 4, 16)])
def test_definition_meets_grid_sample_on_finite_inputs(shapes, B, P, d):
    heads, Q = 2, 40
    case = make_case(heads, d, shapes, B, Q, P, seed=3)
    finite = np.isfinite(case["offs"]).all(axis=(1, 2, 3, 4)) & (np.abs(case["offs"]) < 1e6).all(axis=(1, 2, 3, 4)) \
        & np.isfinite(case["logits"]).all(axis=(1, 2, 3))
    assert finite.sum() >= case["ref"].shape[0] - 6      # all but the rows planted with huge / infinite / NaN offsets and -inf
    got = msda_ref(case["value"], shapes, case["ref"], case["offs"], case["logits"], heads, P)
    clean = dict(case, offs=np.where(finite[:, None, None, None, None], case["offs"], 0).astype(np.float32),
                 logits=np.where(finite[:, None, None, None], case["logits"], 0).astype(np.float32))
    want = _torch64(clean, shapes, heads, P)
    err = np.abs(got["out"] - want)[finite].max()
    print("max |definition - grid_sample| on", int(finite.sum()), "finite rows:", err)
    assert err <= 1e-12 * max(1.0, np.abs(want).max())
    assert (got["D"][finite] >= np.abs(got["out"][finite]) - 1e-12).all() and (got["A"][finite] >= got["D"][finite] - 1e-12).all()


def test_hand_computed_pixel_centre_and_corner():
    """One level of 2 x 3, one head of 16 channels holding the pixel index + 1 (so v[y][x] = 3 y + x + 1), one point, logit 0 (a = 1)."""
    shapes = [(2, 3)]
    value = np.repeat(np.arange(1.0, 7.0)[:, None], 16, axis=1)
    logits = np.zeros((2, 1, 1, 1))
    # query 0: exactly on the centre of pixel (y 1, x 2): position (px, py) = (2, 1) -> ref W - 0.5 = 2 -> ref_x = 2.5 / 3; value 6
    # query 1: (px, py) = (-0.5, -0.5): only corner (0, 0) is inside, with weight 0.5 * 0.5 -> 0.25 * 1
    ref = np.array([[[2.5 / 3, 1.5 / 2]], [[0.0, 0.0]]])
    offs = np.zeros((2, 1, 1, 1, 2))
    r = msda_ref(value, shapes, ref, offs, logits, 1, 1)
    assert np.allclose(r["out"][0], 6.0, rtol=0, atol=1e-14) and np.allclose(r["out"][1], 0.25, rtol=0, atol=1e-14)
    assert np.allclose(r["D"][1], 0.25) and np.allclose(r["A"][1], 1.0)
    # the same through the pixel offsets: ref at the map centre, dx = 2 + 0.5 - 1.5, dy = 1 + 0.5 - 1
    ref2 = np.full((2, 1, 2), 0.5)
    offs2 = np.array([[[[[1.0, 0.5]]]], [[[[-1.5, -1.0]]]]])
    r2 = msda_ref(value, shapes, ref2, offs2, logits, 1, 1)
    assert np.allclose(r2["out"][0], 6.0, rtol=0, atol=1e-14) and np.allclose(r2["out"][1], 0.25, rtol=0, atol=1e-14)


def test_inside_rule_and_softmax_edges():
    shapes = [(2, 3)]
    value = np.ones((6, 16))
    ref = np.full((4, 1, 2), 0.5)
    logits = np.zeros((4, 1, 1, 2))
    offs = np.zeros((4, 1, 1, 2, 2))
    offs[0, 0, 0, 0] = (np.nan, 0.0)          # a NaN position contributes 0: the other point (weight 1/2, at the centre) is left
    offs[1, 0, 0, 0] = (np.inf, 0.0)
    offs[2, 0, 0, 0] = (-2.5, 0.0)            # px = 1.5 - 2.5 - 0.5 = -1.5... the map centre is px = 1.0: 1.0 - 2.5 = -1.5 < -1
    logits[3, 0, 0, 0] = -np.inf              # softmax (0, 1)
    r = msda_ref(value, shapes, ref, offs, logits, 1, 2)
    assert np.allclose(r["out"][:3], 0.5) and np.allclose(r["out"][3], 1.0)
