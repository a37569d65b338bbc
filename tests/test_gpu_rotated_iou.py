"""srf_rotated_iou (csrc/nms.hip) and everything built on it against the float64 clip of tests/rotated_iou_ref.py, on the pairs
the NMS and the OTA assigner actually receive: clusters of nearly identical boxes, the same rectangle written differently, boxes
that share edges and corners -- where a method with in/out and parallel-edge decisions flips on the last bit -- next to pairs in
general position.

IoU values: |gpu - float64| <= 1e-5 for EVERY pair of every call, no pair left out (the project's number for this quantity).
NMS: the kept index list and its order equal the float64 greedy NMS exactly; the inputs are seeded so that the smallest
|IoU - thr| the float64 reference meets is above 1e-4, ten times the IoU bound, asserted on the reference before the GPU is
looked at, so no keep can legitimately flip."""
import numpy as np
import pytest
import torch

import make_fixtures_r2 as mf2
import rotated_iou_ref as R
from srfdet3d_amd import ops, postprocess
from srfdet3d_amd.plugin import training

pytestmark = pytest.mark.gpu
BOUND = 1e-5
MARGIN = 1e-4
GROUPS, P, Q = 182, 10, 11     # 20 020 pairs of the generator's kind in a (1820, 2002) call; 1820 * 2002 = 248 mod 256


def _gpu_iou(a, b, dev):
    out = ops.box_iou_rotated(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert out.shape == (a.shape[0], b.shape[0]) and out.dtype == torch.float32
    return out.cpu().numpy().astype(np.float64)


def _check(name, got, ref, bound):
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref)
    i, j = np.unravel_index(np.argmax(err), err.shape)
    print(f"rotated IoU {name}: {got.size} pairs, max |gpu - float64| = {err.max():.3e} (gpu {got[i, j]:.7f}, float64 {ref[i, j]:.7f}), "
          f"{int((err > bound).sum())} pairs above {bound:g}")
    assert err.max() <= bound, (name, float(err.max()), int((err > bound).sum()), (int(i), int(j)), float(got[i, j]), float(ref[i, j]))


@pytest.mark.parametrize("name", list(R.PAIR_GENERATORS))
def test_iou_matches_float64_clip_on_every_pair(dev, name):
    a, b = R.PAIR_GENERATORS[name](21, GROUPS, P, Q)
    n, m = a.shape[0], b.shape[0]
    assert n != m and (n * m) % 256 != 0 and GROUPS * P * Q >= 20000 and a.dtype == b.dtype == np.float32
    ref = R.iou(a, b)
    got = _gpu_iou(a, b, dev)
    _check(name, got, ref, BOUND)
    back = _gpu_iou(b, a, dev)
    _check(name + " (b, a)", back, ref.T, BOUND)
    sym = np.abs(got - back.T).max()
    print(f"rotated IoU {name}: max |iou(a, b) - iou(b, a)^T| = {sym:.3e}")
    assert sym <= 2 * BOUND, (name, sym)


@pytest.mark.parametrize("name", list(R.PAIR_GENERATORS))
def test_iou_single_row_and_single_column(dev, name):
    a, b = R.PAIR_GENERATORS[name](22, 1, 1, 37)
    _check(name + " (1, 37)", _gpu_iou(a, b, dev), R.iou(a, b), BOUND)
    a, b = R.PAIR_GENERATORS[name](23, 1, 41, 1)
    _check(name + " (41, 1)", _gpu_iou(a, b, dev), R.iou(a, b), BOUND)


def test_iou_hand_checked_pair(dev):
    """a = (0, 0, 2, 3, 0), b = (0, -1, 4, 2, pi/2 as float32): the intersection is 2 x 2.5, IoU = 5 / 9."""
    a = np.array([[0, 0, 2, 3, 0]], np.float32)
    b = np.array([[0, -1, 4, 2, np.float32(np.pi / 2)]], np.float32)
    assert abs(R.iou(a, b)[0, 0] - 5 / 9) < 1e-7
    assert abs(_gpu_iou(a, b, dev)[0, 0] - 5 / 9) <= BOUND and abs(_gpu_iou(b, a, dev)[0, 0] - 5 / 9) <= BOUND


@pytest.mark.parametrize("jitter", [0.0, 1e-6])
def test_bbox_overlaps_3d_of_a_box_set_against_its_copy(dev, jitter):
    """training.bbox_overlaps_3d of (n, 9) boxes against a copy of themselves (a prediction on its ground truth) against the
    float64 composition around the float64 BEV intersection, the whole matrix within 2e-5: at equal boxes
    d IoU3d / d IoU2d = 1 and it is below 1 elsewhere; the other 1e-5 is the float32 torch arithmetic around the kernel."""
    rng = np.random.default_rng(31)
    n = 300
    size = R.CLASS_SIZES[rng.integers(0, len(R.CLASS_SIZES), n)] * rng.uniform(0.9, 1.1, (n, 2))
    b1 = np.concatenate([rng.uniform(-55, 55, (n, 2)), rng.uniform(-2.5, -0.5, (n, 1)), size, rng.uniform(1.4, 2.0, (n, 1)),
                         rng.uniform(-np.pi, np.pi, (n, 1)), rng.normal(0, 1, (n, 2))], axis=1).astype(np.float32)
    b1[n // 2:, :2] = b1[:n - n // 2, :2] + rng.uniform(-1.5, 1.5, (n // 2, 2)).astype(np.float32)   # neighbours that overlap too
    scale = np.concatenate([np.ones((n, 3)), b1[:, 3:7], np.ones((n, 2))], axis=1)
    b2 = (b1 + (rng.uniform(-1, 1, b1.shape) * jitter * scale).astype(np.float32)).astype(np.float32)
    t1, t2 = torch.from_numpy(b1), torch.from_numpy(b2)
    ref = mf2.bbox_overlaps_3d_f64(t1, t2, bev_inter=R.intersection(b1[:, [0, 1, 3, 4, 6]], b2[:, [0, 1, 3, 4, 6]])).numpy()
    assert ref.dtype == np.float64 and np.diagonal(ref).min() > 0.999 and 100 < (ref > 0).sum() - n
    got = training.bbox_overlaps_3d(t1.to(dev), t2.to(dev)).cpu().numpy().astype(np.float64)
    _check(f"bbox_overlaps_3d, copy jittered by {jitter:g}", got, ref, 2 * BOUND)


# ------------------------------------------------------------------------------------------------------------------------- NMS
def _nms(boxes, scores, thr, dev, classes=None):
    cls = None if classes is None else torch.from_numpy(np.asarray(classes, dtype=np.int64)).to(dev)
    return ops.nms_rotated(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), thr, classes=cls).cpu().numpy()


def _reference(boxes, scores, thr, classes=None):
    want, margin = R.greedy_nms(boxes, scores, thr, classes=classes)
    assert margin > MARGIN, f"test data has an IoU within {MARGIN:g} of the threshold ({margin:.3e})"
    return want


SCENE_SEED = 3


@pytest.mark.parametrize("thr", [0.4, 0.2])
def test_nms_of_a_clustered_scene_keeps_one_box_per_object(dev, thr):
    """50 objects x 18 copies jittered by 10^U(-7, -2), every sixth with yaw + pi: the float64 greedy NMS keeps the best copy of
    every object and nothing else, and so must the kernels, in the same order."""
    boxes, scores, obj = R.clustered_scene(SCENE_SEED)
    want = _reference(boxes, scores, thr)
    assert len(want) == 50 and sorted(obj[want]) == list(range(50))
    got = _nms(boxes, scores, thr, dev)
    np.testing.assert_array_equal(got, want)


def _two_class_scene():
    boxes, scores, obj = R.clustered_scene(SCENE_SEED)
    cls = (np.arange(len(obj)) % 18) % 2            # each object's copies spread over two classes
    return boxes, scores, obj, cls


def test_nms_classes_keeps_two_boxes_per_object(dev):
    boxes, scores, obj, cls = _two_class_scene()
    for thr in (0.4, 0.2):
        want = _reference(boxes, scores, thr, classes=cls)
        assert len(want) == 100 and sorted(obj[want] * 2 + cls[want]) == list(range(100))
        np.testing.assert_array_equal(_nms(boxes, scores, thr, dev, classes=cls), want)


@pytest.mark.parametrize("with_classes", [False, True])
def test_nms_counted_is_the_greedy_nms_of_the_prefix(dev, with_classes):
    """nms_rotated_counted with the live count at 0, 1, the edges of a mask word, n - 1, n and above n: rows past the count are
    never kept, the rows before it are kept as the float64 greedy NMS of that prefix keeps them."""
    boxes, scores, obj, cls = _two_class_scene()
    n = boxes.shape[0]
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    sb, ss, sc = boxes[order], scores[order], cls[order]
    tb = torch.from_numpy(sb).to(dev)
    tc = torch.from_numpy(sc.astype(np.int64)).to(dev) if with_classes else None
    for live in (0, 1, 63, 64, 65, n - 1, n, n + 7):
        k = min(live, n)
        want = _reference(sb[:k], ss[:k], 0.4, classes=sc[:k] if with_classes else None)
        flags = np.zeros(n, dtype=np.int32)
        flags[want] = 1
        got = ops.nms_rotated_counted(tb, torch.tensor([live], dtype=torch.int32, device=dev), 0.4, classes=tc).cpu().numpy()
        np.testing.assert_array_equal(got, flags, err_msg=f"live = {live}")
        if live >= n:
            assert flags.sum() == (100 if with_classes else 50)


def test_multiclass_nms_paths_on_the_clustered_scene(dev):
    """postprocess.box3d_multiclass_nms, its fixed-shape form and the blockwise NMS on the scene: the survivors of the float64
    per-class greedy NMS, class-major, descending score inside a class."""
    boxes, scores, obj, cls = _two_class_scene()
    n = boxes.shape[0]
    assert scores.min() > 0
    b3 = np.zeros((n, 9), np.float32)
    b3[:, [0, 1, 3, 4, 6]] = boxes
    b3[:, 2], b3[:, 5] = -1.0, 1.5
    b3[:, 7:] = np.random.default_rng(0).normal(0, 1, (n, 2))
    s2 = np.zeros((n, 2), np.float32)
    s2[np.arange(n), cls] = scores
    want = _reference(boxes, scores, 0.4, classes=cls)
    want = want[np.lexsort((-scores[want].astype(np.float64), cls[want]))]      # class-major, descending score inside
    tb, ts = torch.from_numpy(b3).to(dev), torch.from_numpy(s2).to(dev)
    ob, os_, ol = postprocess.box3d_multiclass_nms(tb, ts, 0.0, 10 ** 6, 0.4)
    np.testing.assert_array_equal(ob.cpu().numpy(), b3[want])
    np.testing.assert_array_equal(os_.cpu().numpy(), scores[want])
    np.testing.assert_array_equal(ol.cpu().numpy(), cls[want])
    ob, os_, ol, kept, m = postprocess.box3d_multiclass_nms_static(tb, ts, 0.0, 0.4)
    assert int(kept) == len(want) == 100 and int(m) == n
    np.testing.assert_array_equal(ob.cpu().numpy()[:100], b3[want])
    np.testing.assert_array_equal(os_.cpu().numpy()[:100], scores[want])
    np.testing.assert_array_equal(ol.cpu().numpy()[:100], cls[want])
    for thr in (0.4, 0.2):
        one = _reference(boxes, scores, thr)
        got = postprocess._nms_rotated_blocks(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), thr, block=257)
        np.testing.assert_array_equal(got.cpu().numpy(), one)


# seeds of R.mixed_scene per size, chosen on the float64 reference alone so that its margin at thr 0.4 exceeds MARGIN
SIZE_SEEDS = {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 127: 1, 128: 1, 129: 1, 4095: 2, 4096: 2}


@pytest.mark.parametrize("n", list(SIZE_SEEDS))
def test_nms_sizes_at_the_edges_of_the_mask_words(dev, n):
    """n at the edges of the 64-bit mask words and of the single-wave reduce (64 words = 4096 boxes), clusters and loners mixed."""
    boxes, scores = R.mixed_scene(SIZE_SEEDS[n], n)
    want = _reference(boxes, scores, 0.4)
    assert n < 3 or 0 < len(want) < n
    np.testing.assert_array_equal(_nms(boxes, scores, 0.4, dev), want)


def test_nms_refuses_more_than_4096_boxes(dev):
    boxes, scores = R.mixed_scene(1, 4097)
    with pytest.raises(RuntimeError, match=r"nms_rotated failed \(-3\)"):
        _nms(boxes, scores, 0.4, dev)
    with pytest.raises(RuntimeError, match=r"nms_rotated_classes failed \(-3\)"):
        _nms(boxes, scores, 0.4, dev, classes=np.zeros(4097, np.int64))


@pytest.mark.parametrize("at", [(3, 7, 11), (63, 64, 65), (10, 100, 1000)])
def test_nms_suppression_chain(dev, at):
    """A > B > C in score, IoU(A, B) and IoU(B, C) above the threshold, IoU(A, C) below: B goes, so C stays -- only KEPT boxes
    suppress.  The three inside one mask word, across a word boundary and across row blocks; every other box is a loner."""
    n = 1100
    rng = np.random.default_rng(41)
    grid = np.stack(np.meshgrid(np.arange(40), np.arange(40)), axis=-1).reshape(-1, 2)[:n] * 10.0 + 100.0
    boxes = np.concatenate([grid, np.tile([2.0, 4.0], (n, 1)), rng.uniform(-np.pi, np.pi, (n, 1))], axis=1).astype(np.float32)
    yaw = 0.3
    step = np.array([np.cos(yaw), np.sin(yaw)]) * 0.8            # along the 2 m side: IoU 0.4286 one step apart, 0.1111 two
    for k, i in enumerate(at):
        boxes[i] = [5.0 + k * step[0], -3.0 + k * step[1], 2.0, 4.0, yaw]
    scores = (1.0 - np.arange(n) / n).astype(np.float32)         # rank = index
    m = R.iou(boxes[list(at)], boxes[list(at)])
    assert m[0, 1] > 0.42 and m[1, 2] > 0.42 and m[0, 2] < 0.12
    want = _reference(boxes, scores, 0.4)
    assert list(want) == [i for i in range(n) if i != at[1]]
    np.testing.assert_array_equal(_nms(boxes, scores, 0.4, dev), want)


def test_nms_tied_scores_inside_clusters(dev):
    """Equal proposals give equal logits: all copies of an object share one score.  The sort is stable (lower index first), so
    the first copy of every object survives."""
    boxes, _, obj = R.clustered_scene(SCENE_SEED)
    scores = np.random.default_rng(51).uniform(0, 1, 50).astype(np.float32)[obj]
    perm = np.random.default_rng(52).permutation(len(obj))       # the copies of an object are not neighbours in the input
    boxes, scores, obj = boxes[perm], scores[perm], obj[perm]
    want = _reference(boxes, scores, 0.4)
    assert len(want) == 50 and all(i == np.nonzero(obj == obj[i])[0][0] for i in want)
    np.testing.assert_array_equal(_nms(boxes, scores, 0.4, dev), want)
    cls = np.arange(len(obj)) % 2
    np.testing.assert_array_equal(_nms(boxes, scores, 0.4, dev, classes=cls), _reference(boxes, scores, 0.4, classes=cls))
