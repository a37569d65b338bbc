"""tests/rotated_iou_ref.py against closed forms and symmetries it cannot get right by accident (no GPU).  Both sides of every
comparison are float64 formulas of well-conditioned cases: tolerance 1e-12."""
import numpy as np
import pytest

import rotated_iou_ref as R

TOL = 1e-12
GROUPS, P, Q = 40, 5, 6  # 1200 pairs of the generator's kind per generator, 48 000 pairs in all


def test_axis_aligned_pairs_equal_the_interval_formula():
    rng = np.random.default_rng(0)
    k = 3000
    a = np.concatenate([rng.uniform(-5, 5, (k, 2)), rng.uniform(0.2, 6, (k, 2)), np.zeros((k, 1))], axis=1).astype(np.float32)
    b = np.concatenate([a[:, :2] + rng.uniform(-4, 4, (k, 2)), rng.uniform(0.2, 6, (k, 2)), np.zeros((k, 1))], axis=1).astype(np.float32)
    A, B = a.astype(np.float64), b.astype(np.float64)
    ox = np.minimum(A[:, 0] + A[:, 2] / 2, B[:, 0] + B[:, 2] / 2) - np.maximum(A[:, 0] - A[:, 2] / 2, B[:, 0] - B[:, 2] / 2)
    oy = np.minimum(A[:, 1] + A[:, 3] / 2, B[:, 1] + B[:, 3] / 2) - np.maximum(A[:, 1] - A[:, 3] / 2, B[:, 1] - B[:, 3] / 2)
    inter = np.clip(ox, 0, None) * np.clip(oy, 0, None)
    want = inter / (A[:, 2] * A[:, 3] + B[:, 2] * B[:, 3] - inter)
    assert 0.2 < (want > 0).mean() < 0.95 and want.max() > 0.7
    np.testing.assert_allclose(R.iou_pairs(a, b), want, rtol=0, atol=TOL)
    m = R.iou(a[:60], b[:70])                     # the (n, m) form addresses the same pairs
    np.testing.assert_allclose(np.diagonal(m), want[:60], rtol=0, atol=TOL)
    np.testing.assert_allclose(m, R.iou_pairs(np.repeat(a[:60], 70, 0), np.tile(b[:70], (60, 1))).reshape(60, 70), rtol=0, atol=0)


def test_square_turned_by_quarter_pi_in_a_square_is_the_regular_octagon():
    a = np.array([[3.0, -2.0, 1.0, 1.0, 0.3]])
    b = np.array([[3.0, -2.0, 1.0, 1.0, 0.3 + np.pi / 4]])
    area = 2 * np.sqrt(2) - 2
    np.testing.assert_allclose(R.intersection(a, b), [[area]], rtol=0, atol=TOL)
    np.testing.assert_allclose(R.iou(a, b), [[area / (2 - area)]], rtol=0, atol=TOL)
    np.testing.assert_allclose(R.iou(b.astype(np.float32), a.astype(np.float32)), [[area / (2 - area)]], rtol=0, atol=1e-7)


def test_identical_disjoint_touching_and_zero_area():
    a, b = R.identical(5, 50, 2, 3)
    m = R.iou(a, b)
    for g in range(50):
        np.testing.assert_allclose(m[2 * g:2 * g + 2, 3 * g:3 * g + 3], 1.0, rtol=0, atol=TOL)
    far = a.copy()
    far[:, 0] += 40.0                              # further than any diagonal (at most 11.6 m)
    assert np.all(R.iou_pairs(a, far) == 0.0)
    # exact contact on a dyadic lattice (the first half of the groups has yaw 0): 0, not a sliver
    ta, tb = R.touching(6, 64, 3, 4)
    m = R.iou(ta, tb)
    for g in range(32):
        assert np.all(m[3 * g:3 * g + 3, 4 * g:4 * g + 4] == 0.0)
    for g in range(32, 64):                        # turned pairs touch up to float32 rounding of the centres
        assert np.all(m[3 * g:3 * g + 3, 4 * g:4 * g + 4] < 1e-4)   # sliver <= 4e-6 m x 10 m
    # moved 1/8 m towards a along x the same boxes overlap
    one_a, one_b = np.array([[0, 0, 2, 2, 0]], np.float32), np.array([[2, 0.5, 2, 2, 0]], np.float32)
    assert R.iou(one_a, one_b)[0, 0] == 0.0
    one_b[0, 0] -= 0.125
    np.testing.assert_allclose(R.iou(one_a, one_b), [[0.125 * 1.5 / (8 - 0.125 * 1.5)]], rtol=0, atol=TOL)
    za, zb = R.zero_width(7, 50, 3, 4)
    m = R.iou(za, zb)
    dead_a, dead_b = za[:, 2] * za[:, 3] < 1e-14, zb[:, 2] * zb[:, 3] < 1e-14
    assert dead_a.sum() > 50 and dead_b.sum() > 50 and (~dead_a).sum() > 20
    assert np.all(m[dead_a] == 0.0) and np.all(m[:, dead_b] == 0.0)
    live = m[np.ix_(~dead_a, ~dead_b)]
    assert live.max() == pytest.approx(1.0, abs=TOL)


def _moved(x, pivot, phi, t):
    c, s = np.cos(phi), np.sin(phi)
    d = x[:, :2] - pivot
    y = x.copy()
    y[:, 0] = c * d[:, 0] - s * d[:, 1] + t[0]
    y[:, 1] = s * d[:, 0] + c * d[:, 1] + t[1]
    y[:, 4] = x[:, 4] + phi
    return y


@pytest.mark.parametrize("name", list(R.PAIR_GENERATORS))
def test_invariances_of_every_generated_pair(name):
    """A common rotation and translation of both boxes, (w, h, yaw) -> (h, w, yaw + pi/2) and yaw -> yaw + pi leave the IoU
    unchanged.  On float64 copies of the inputs, so that no float32 rounding of the moved boxes enters; the motion turns about a
    pivot next to the data (the far generator sits at 3000 m, where a float64 coordinate carries 5e-13)."""
    a32, b32 = R.PAIR_GENERATORS[name](11, GROUPS, P, Q)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    a, b = np.repeat(a, Q, axis=0), np.tile(b.reshape(GROUPS, Q, 5), (1, P, 1)).reshape(-1, 5)   # the in-group pairs
    want = R.iou_pairs(a, b)
    np.testing.assert_array_equal(want, R.iou_pairs(a32.repeat(Q, axis=0), b.astype(np.float32)))  # float32 in = its float64 copy
    if name == "zero_width":
        assert np.all(want[(a[:, 2] * a[:, 3] < 1e-14) | (b[:, 2] * b[:, 3] < 1e-14)] == 0)
    rng = np.random.default_rng(12)
    pivot = np.round(a[:, :2].mean(axis=0))
    for _ in range(2):
        phi, t = rng.uniform(-np.pi, np.pi), rng.uniform(-10, 10, 2)
        np.testing.assert_allclose(R.iou_pairs(_moved(a, pivot, phi, t), _moved(b, pivot, phi, t)), want, rtol=0, atol=TOL)
    sw = b.copy()
    sw[:, 2], sw[:, 3], sw[:, 4] = b[:, 3], b[:, 2], b[:, 4] + np.pi / 2
    np.testing.assert_allclose(R.iou_pairs(a, sw), want, rtol=0, atol=TOL)
    tu = a.copy()
    tu[:, 4] += np.pi
    np.testing.assert_allclose(R.iou_pairs(tu, b), want, rtol=0, atol=TOL)
    np.testing.assert_allclose(R.iou_pairs(b, a), want, rtol=0, atol=TOL)                       # and it is symmetric


def test_greedy_nms_against_the_quadratic_loop():
    boxes, scores = R.mixed_scene(3, 50)
    scores[10:14] = scores[10]                     # a tie: lower index first
    classes = np.arange(50) % 2
    for cls in (None, classes):
        for thr in (0.2, 0.4):
            got, margin = R.greedy_nms(boxes, scores, thr, classes=cls)
            m = R.iou(boxes, boxes)
            keep = []
            for i in sorted(range(50), key=lambda i: (-scores[i], i)):
                if all(m[j, i] <= thr or (cls is not None and cls[j] != cls[i]) for j in keep):
                    keep.append(i)
            assert list(got) == keep and 5 < len(keep) < 50
            pairs = [abs(m[j, i] - thr) for j in keep for i in range(50)
                     if (scores[i], -i) < (scores[j], -j) and (cls is None or cls[i] == cls[j])]
            assert margin == pytest.approx(min(pairs), abs=TOL)
    one, margin = R.greedy_nms(boxes[:1], scores[:1], 0.4)
    assert list(one) == [0] and margin == np.inf


def test_scenes_are_what_they_claim():
    boxes, scores, obj = R.clustered_scene(3)
    assert boxes.shape == (900, 5) and boxes.dtype == np.float32 and scores.dtype == np.float32
    m = R.iou(boxes, boxes)
    same = obj[:, None] == obj[None, :]
    assert m[same].min() > 0.9 and m[~same].max() == 0.0
    assert (np.abs(boxes[:, 4]) > np.pi).any()     # the flipped copies leave [-pi, pi]
    for n in (1, 2, 63, 4096):
        b, s = R.mixed_scene(5, n)
        assert b.shape == (n, 5) and s.shape == (n,)
