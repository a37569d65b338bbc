"""tests/set_loss_ref.py, the float64 text of the definition in csrc/setloss.hip, against float64 autograd through `training.FocalLoss` /
`training.L1Loss` composed as `SRFDetHead.loss_classification` / `loss_boxes` compose them: losses and gradients to 1e-12 relative, both
sides being float64.  Cases: gamma 2 and 1.5, an empty sample, a label equal to C (background), a target with dx = 0 (log gives -inf) and
one with dx < 0 (NaN), a prediction equal to its target, a zero code weight.  The f32 form of the text is the float64 form rounded once."""
import numpy as np
import pytest
import torch

import set_loss_ref as R

KW = dict(alpha=0.25, w_cls=2.0, w_box=0.25)
SHAPES = [(8, 8, 7), (10, 10, 9)]


def build(D, Dw, Dg, seed=0):
    """S 3, B 2, P 33, C 5; sample 1 is empty.  Sample 0 has 6 boxes: box 1 has class C, box 2 has dx = 0, box 3 has dx < 0, and the
    prediction matched to box 4 in stage 0 equals its target exactly; code weight 2 is zero."""
    C = 5
    c = R.case(seed, 3, 2, 33, C, D, Dw, Dg, ns=[6, 0], logit_scale=2.0)
    c["labels"][0, 1] = C
    c["gt"][0, 2, 3] = 0.0
    c["gt"][0, 3, 3] = -1.5
    c["gt_idx"][:, 0, :6] = np.arange(6)                 # every special box is matched in every stage, once
    c["gt_idx"][:, 0, 6:11] = 5
    c["cw"][2] = 0.0
    return c


def exact_row(c, dtype):
    """The prediction of slot 4 of (stage 0, sample 0) := its normalised target, computed the way the route under test computes it."""
    u = c["gt"][0, c["gt_idx"][0, 0, 4]].astype(dtype)
    tn = np.concatenate([u[:3], np.log(u[3:6]), [np.sin(u[6]), np.cos(u[6])], u[7:]])
    return int(c["pred_idx"][0, 0, 4]), tn


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("D,Dw,Dg", SHAPES)
def test_float64_text_is_float64_autograd(gamma, D, Dw, Dg):
    c = build(D, Dw, Dg)
    c = {k: (v.astype(np.float64) if v.dtype == np.float32 and k not in ("cw", "num") else v) for k, v in c.items()}
    p, tn = exact_row(c, np.float64)
    c["boxes"][0, 0, p, :Dw] = tn[:Dw]
    loss, gl, gb, matched, box_rows = R.ref(c, gamma=gamma, **KW)
    t_loss, t_gl, t_gb = R.torch_route(c, gamma=gamma, dtype=torch.float64, **KW)
    np.testing.assert_allclose(loss, t_loss, rtol=1e-12, atol=0)
    np.testing.assert_allclose(gl, t_gl, rtol=1e-12, atol=0)
    np.testing.assert_allclose(gb, t_gb, rtol=1e-12, atol=0)
    # the cases are there: an empty sample, the rows of dx = 0 and dx < 0 out of the box loss, the exact row and the zero weight without gradient
    assert not matched[:, 1].any() and matched[:, 0].sum() == 3 * 11
    assert (matched & ~box_rows).sum() == 2 * 3
    assert box_rows[0, 0, p] and not gb[0, 0, p].any()
    assert not gb[..., 2].any() and gb[..., 0].any()
    assert (gb[..., Dw:] == 0).all() and (gb[~box_rows] == 0).all()
    row_c = c["pred_idx"][0, 0, 1]                        # matched to the box of class C: a background row
    assert (gl[0, 0, row_c] > 0).all()
    assert np.isfinite(loss).all() and (loss > 0).all()


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_f32_text_is_the_float64_text_rounded(gamma):
    c = build(10, 10, 9, seed=1)
    loss, gl, gb, _, _ = R.ref(c, gamma=gamma, **KW)
    loss32, gl32, gb32, _, _ = R.ref(c, gamma=gamma, dtype=np.float32, **KW)
    assert loss32.dtype == gl32.dtype == gb32.dtype == np.float32 and loss.dtype == gl.dtype == gb.dtype == np.float64
    for x32, x in ((loss32, loss), (gl32, gl), (gb32, gb)):
        np.testing.assert_array_equal(x32, x.astype(np.float32))
    assert np.array_equal(np.sign(gb32), np.sign(gb))     # no box gradient rounds to zero


def test_out_of_range_slots_are_skipped_and_a_non_finite_stage_has_no_gradient():
    c = build(8, 8, 7, seed=2)
    base = R.ref(c, gamma=2.0, **KW)
    d = {k: v.copy() for k, v in c.items()}
    P = c["logits"].shape[2]
    k = int(c["count"][1, 0])
    d["pred_idx"][1, 0, k], d["gt_idx"][1, 0, k] = P, 0                     # a row past the end
    d["pred_idx"][1, 0, k + 1], d["gt_idx"][1, 0, k + 1] = 0, -1            # a box before the start
    d["count"][1, 0] = k + 2
    d["count"][2, 1] = P + 5                                                 # clamped to P; the slots hold -1
    for x, y in zip(base, R.ref(d, gamma=2.0, **KW)):
        np.testing.assert_array_equal(x, y)
    d = {k: v.copy() for k, v in c.items()}
    d["boxes"][1, 0, c["pred_idx"][1, 0, 0], 0] = np.inf
    loss, gl, gb, _, _ = R.ref(d, gamma=2.0, **KW)
    assert loss[1, 1] == R.F32_MAX and not gb[1].any() and gb[0].any() and gb[2].any()
    np.testing.assert_array_equal(gl, base[1])
    np.testing.assert_array_equal(loss[[0, 2]], base[0][[0, 2]])
