"""tests/detect_tail_ref.py (the numpy definition the GPU detection tail is held to) against naive Python loops, and
SRFDetHead.results_from_static, which is host code, against the definition.  No GPU."""
import numpy as np
import pytest
import torch

import detect_tail_ref as T
import rotated_iou_ref as R

F32 = np.float32


def _random_scores(rng, n, C):
    """small score tables with everything the definition has a rule for: ties, NaN, +-inf, +-0, entries on the threshold"""
    s = rng.uniform(-0.2, 1.0, (n, C)).astype(F32)
    kind = rng.integers(0, 4)
    if kind >= 1:   # a few shared values
        s = (np.round(s * 4) / 4).astype(F32)
    if kind >= 2:
        flat = s.reshape(-1)
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            flat[rng.integers(0, flat.size)] = v
    if kind == 3:
        s[:] = s.reshape(-1)[0]
    return s


def _naive_select(scores, thr, capacity):
    flat = [F32(v) for v in scores.reshape(-1)]
    rem = [(i, v) for i, v in enumerate(flat) if v > F32(thr)]
    m, front = len(rem), []
    while rem:
        best = rem[0]
        for p in rem[1:]:
            if p[1] > best[1]:   # strictly better only: the earlier flat index wins a tie (0.0 > -0.0 is false)
                best = p
        rem.remove(best)
        front.append(best)
    L = min(len(flat), capacity)
    rest = [i for i, v in enumerate(flat) if not v > F32(thr)]
    k = min(m, L)
    return [p[0] for p in front[:k]] + rest[:L - k], [p[1] for p in front[:k]] + [F32(-1)] * (L - k), m


def test_select_is_the_naive_selection():
    rng = np.random.default_rng(0)
    seen = dict(ties=0, nan=0, over=0, under=0, empty=0)
    for _ in range(400):
        n, C = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        scores = _random_scores(rng, n, C)
        boxes = rng.uniform(-1, 1, (n, 7)).astype(F32)
        thr = float(rng.choice([0.0, 0.25, 0.5, -0.5, -1.0]))
        cap = int(rng.integers(1, n * C + 3))
        idx, top_s, m = T.select(boxes, scores, thr, cap)
        widx, ws, wm = _naive_select(scores, thr, cap)
        assert m == wm and idx.tolist() == widx and idx.shape == (min(n * C, cap),)
        assert top_s.dtype == F32 and top_s.tobytes() == np.array(ws, dtype=F32).tobytes()     # bit for bit: -0.0 stays -0.0
        cand, cls, bev = T.candidates(boxes, idx, C)
        assert np.array_equal(cand, boxes[idx // C]) and np.array_equal(cls, idx % C) and np.array_equal(bev, cand[:, [0, 1, 3, 4, 6]])
        k = min(m, idx.size)
        T.padding_contract(boxes, scores, thr, idx[:k], cand[k:], top_s[k:], cls[k:], bev[k:], idx[k:] // C)
        front = top_s[:k]
        seen["ties"] += int(k > 1 and np.any(front[1:] == front[:-1]))
        seen["nan"] += int(np.isnan(scores).any())
        seen["over"] += int(m > idx.size)
        seen["under"] += int(0 < m < idx.size)
        seen["empty"] += int(m == 0)
    assert min(seen.values()) >= 10, seen


def _naive_finish(top_s, cls, keep):
    rows = [(j, F32(F32(cls[j]) * F32(4)) - F32(min(max(F32(top_s[j]), F32(0)), F32(1)) * F32(2))) for j in range(len(keep)) if keep[j] != 0]
    for a in range(len(rows)):                       # stable insertion sort on the float32 key
        b = a
        while b > 0 and rows[b][1] < rows[b - 1][1]:
            rows[b], rows[b - 1] = rows[b - 1], rows[b]
            b -= 1
    return [r[0] for r in rows] + [j for j in range(len(keep)) if keep[j] == 0], len(rows)


def test_finish_is_the_naive_stable_sort():
    rng = np.random.default_rng(1)
    equal_keys = 0
    for _ in range(400):
        L, D = int(rng.integers(1, 41)), int(rng.choice([7, 9]))
        live = int(rng.integers(0, L + 1))
        top_s = np.sort(np.round(rng.uniform(0.1, 1.6, L) * 8) / 8)[::-1].astype(F32)     # descending with ties, some above 1
        top_s[live:] = -1
        cls = rng.integers(0, 32, L)
        keep = rng.choice([0, 0, 1, 1, 7, -1], L).astype(np.int32) * (rng.random() < 0.9)
        cand = rng.uniform(-1, 1, (L, D)).astype(F32)
        perm, kept = T.finish(cand, top_s, cls, keep)
        wperm, wkept = _naive_finish(top_s, cls, keep)
        assert perm.tolist() == wperm and kept == wkept and sorted(perm.tolist()) == list(range(L))
        key = T.finish_key(top_s[perm[:kept]], cls[perm[:kept]])
        equal_keys += int(kept > 1 and np.any(key[1:] == key[:-1]))
        packed = T.packed_rows(cand, top_s, cls, perm)
        assert packed.shape == (L, D + 2) and np.array_equal(packed[:, :D], cand[perm]) and np.array_equal(packed[:, D], top_s[perm])
        assert np.array_equal(packed[:, D + 1], cls[perm].astype(F32))
    assert equal_keys >= 50


def test_finish_key_is_coarser_than_the_scores():
    """the reason the order must not rest on the key alone: class 9, scores one ulp apart, one key"""
    s = np.array([0.5, np.nextafter(F32(0.5), F32(1))], dtype=F32)
    assert s[0] != s[1] and np.all(T.finish_key(s, [9, 9]) == F32(35))


def _literal_multiclass_nms(boxes, scores, thr, nms_thr, max_num):
    ob, os_, ol = [], [], []
    for c in range(scores.shape[1]):
        idx = [b for b in range(scores.shape[0]) if scores[b, c] > F32(thr)]
        idx.sort(key=lambda b: -float(scores[b, c]))   # list.sort is stable: the lower box first among equals
        kept = []
        for b in idx:
            if all(R.iou_pairs(boxes[k:k + 1][:, T.BEV_COLS], boxes[b:b + 1][:, T.BEV_COLS])[0] <= nms_thr for k in kept):
                kept.append(b)
        ob += [boxes[b] for b in kept]
        os_ += [scores[b, c] for b in kept]
        ol += [c] * len(kept)
    order = sorted(range(len(os_)), key=lambda j: -float(os_[j]))[:max_num] if len(os_) > max_num else range(len(os_))
    return [ob[j] for j in order], [os_[j] for j in order], [ol[j] for j in order]


@pytest.mark.parametrize("seed", range(6))
def test_multiclass_nms_is_the_per_class_loop(seed):
    rng = np.random.default_rng(seed)
    n, C = 40, 4
    bev = np.concatenate([rng.uniform(-6, 6, (n, 2)), rng.uniform(1, 4, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(F32)
    boxes = T.boxes_from_bev(bev, 9, rng)
    scores = (np.round(rng.uniform(0, 1, (n, C)) * 20) / 20).astype(F32) if seed % 2 else rng.uniform(0, 1, (n, C)).astype(F32)
    for max_num in (10 ** 6, 25):
        b, s, l, margin = T.multiclass_nms(boxes, scores, 0.3, 0.2, max_num)
        wb, ws, wl = _literal_multiclass_nms(boxes, scores, 0.3, 0.2, max_num)
        assert margin > 1e-9
        assert len(wb) == b.shape[0] > 10 and np.array_equal(b, np.array(wb)) and np.array_equal(s, np.array(ws, dtype=F32))
        assert l.tolist() == wl
    # the static chain with room for every candidate returns the same rows in the same order
    ch = T.static_chain(boxes, scores, 0.3, 0.2, 2048)
    b, s, l, _ = T.multiclass_nms(boxes, scores, 0.3, 0.2, 10 ** 6)
    k = ch["kept"]
    assert ch["m"] <= 160 and k == b.shape[0]
    assert np.array_equal(ch["out_boxes"][:k], b) and np.array_equal(ch["out_scores"][:k], s) and np.array_equal(ch["out_labels"][:k], l)
    assert np.array_equal(ch["packed"][:, :9], ch["out_boxes"]) and ch["counts"].tolist() == [k, ch["m"]]


SCENES = [("crowded", 0), ("clusters", 0), ("sparse", 0), ("overflow", 0)]


@pytest.mark.parametrize("kind,seed", SCENES)
def test_scenes_are_off_the_threshold(kind, seed):
    """The frames of the GPU chain tests: distinct scores above the threshold, no IoU within 1e-5 of the NMS threshold (the
    kernel's IoU error is <= 1.8e-6), and the static and the dynamic definition agree where the capacity holds every candidate."""
    boxes, scores, thr, nms_thr = T.scene(kind, seed)
    above = scores[scores > F32(thr)]
    assert np.unique(above).size == above.size
    ch = T.static_chain(boxes, scores, thr, nms_thr, 2048)
    b, s, l, margin = T.multiclass_nms(boxes, scores, thr, nms_thr, 10 ** 6)
    print(f"\nscene {kind}/{seed}: m {ch['m']} kept {ch['kept']} (dynamic {b.shape[0]}) margin {min(margin, ch['margin']):.2e}")
    assert ch["margin"] >= 1e-5 and margin >= 1e-5
    k = ch["kept"]
    if kind == "overflow":
        assert ch["m"] > 2048
    else:
        assert ch["m"] <= 2048 and k == b.shape[0]
        assert np.array_equal(ch["out_boxes"][:k], b) and np.array_equal(ch["out_scores"][:k], s) and np.array_equal(ch["out_labels"][:k], l)
    if kind in ("sparse", "overflow"):
        assert k > 1024     # srf_nms_finish takes its bitonic path
    else:
        assert k <= 1024


def _head(max_per_img, rng_box):
    from srfdet3d_amd.plugin import heads
    hd = object.__new__(heads.SRFDetHead)
    torch.nn.Module.__init__(hd)
    hd.test_cfg = dict(max_per_img=max_per_img, post_center_range=rng_box)
    return hd


def test_results_from_static_is_the_definition():
    """heads.results_from_static against detect_tail_ref.results: the kept rows, the max_per_img cut, the centre filter, None on
    overflow -- including tied scores that straddle the cut.  results_from_static cuts with a stable argsort, so among equal
    scores the earlier row (the lower class, then the lower candidate) stays.  That is this project's choice: the reference's
    `scores.sort(descending=True)` leaves the order of ties unspecified."""
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    box = [-10.0, -10.0, -5.0, 10.0, 10.0, 5.0]
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)] * 2
    rng = np.random.default_rng(3)
    cuts = 0
    for trial in range(60):
        L, D, cut = int(rng.integers(4, 30)), int(rng.choice([7, 9])), int(rng.integers(1, 12))
        packed = rng.uniform(-1, 1, (2, L, D + 2)).astype(F32)
        packed[..., :3] = rng.uniform(-12, 12, (2, L, 3))
        packed[..., D] = np.round(rng.uniform(0.1, 1, (2, L)) * 6) / 6            # few values: ties everywhere
        packed[..., D + 1] = rng.integers(0, 10, (2, L))
        counts = np.stack([[int(rng.integers(0, L + 1)), L] for _ in range(2)]).astype(np.int32)
        hd = _head(cut, box)
        got = hd.results_from_static(torch.from_numpy(packed), torch.from_numpy(counts), metas)
        want = T.results(packed, counts, cut, box)
        for i in range(2):
            assert got[i][0].tensor.numpy().tobytes() == want[i][0].tobytes() and got[i][0].tensor.shape == want[i][0].shape
            assert np.array_equal(got[i][1].numpy(), want[i][1]) and np.array_equal(got[i][2].numpy(), want[i][2])
            assert got[i][2].dtype == torch.int64
            kept = int(counts[i, 0])
            if kept > cut:     # a tie across the cut: the row kept is the earlier one
                s = packed[i, :kept, D]
                cuts += int(np.sort(s)[::-1][cut - 1] == np.sort(s)[::-1][cut])
    assert cuts >= 10
    # the literal case: three rows of one score, room for two -> rows 0 and 1, in that order
    packed = np.zeros((1, 4, 9), dtype=F32)
    packed[0, :, 0] = [1, 2, 3, 4]
    packed[0, :, 7] = [0.5, 0.5, 0.5, 0.25]
    got = _head(2, box).results_from_static(torch.from_numpy(packed), torch.tensor([[4, 4]], dtype=torch.int32), metas[:1])
    assert got[0][0].tensor[:, 0].tolist() == [1.0, 2.0]
    assert _head(2, box).results_from_static(torch.from_numpy(packed), torch.tensor([[4, 5]], dtype=torch.int32), metas[:1]) is None
    assert T.results(packed, [[4, 5]], 2, box) is None


def test_decode_definition_on_hand_values():
    pc = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
    pred = np.array([[0.5, 0.25, 1.0, 0.0, np.log(2.0), np.log(4.0), 1.0, 0.0, 7.0, -8.0]])
    s, b = T.decode(np.array([[0.0, 800.0, -800.0]]), pred, pc)
    assert s.tolist() == [[0.5, 1.0, 0.0]]
    np.testing.assert_allclose(b[0], [0.0, -27.0, 3.0 - 2.0, 1.0, 2.0, 4.0, np.pi / 2, 7.0, -8.0], rtol=1e-15, atol=1e-15)
    assert T.decode(np.zeros((2, 3, 1)), np.zeros((2, 3, 8)), pc)[1].shape == (2, 3, 7)
