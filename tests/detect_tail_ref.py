"""The definition of the detection tail: what turns decoded boxes and scores into detections (srf_decode_boxes ->
srf_nms_select -> rotated NMS -> srf_nms_finish -> srf_host_pack -> SRFDetHead.results_from_static, and its dynamic twin
postprocess.box3d_multiclass_nms).  Plain numpy, no project kernel, no torch.

Everything here but `decode` is selection and permutation: the results are exact, and the tests compare them with `==`.
The float64 rotated NMS is rotated_iou_ref.greedy_nms."""
import numpy as np

import rotated_iou_ref as R

BEV_COLS = [0, 1, 3, 4, 6]  # [x, y, w, l, yaw] of a (n, 7|9|10) box row


# ---------------------------------------------------------------------------------------------------------------- select
def select(boxes, scores, thr, capacity):
    """scores (n, C) float32 -> (flat_idx (L,) int64, top_s (L,) float32, m) with L = min(n * C, capacity).

    A (box, class) pair is valid when its score is > float32(thr) (NaN is not).  m counts the valid pairs.  Rows < min(m, L): the
    valid pairs in descending score, equal scores (+0 and -0 are equal) by ascending flat index i = box * C + class.  Rows
    >= min(m, L): top_s = -1, and flat_idx the pairs at or below the threshold in ascending flat index -- the kernel's header
    states this order; `padding_contract` checks the weaker promise (distinct non-candidates) on its own."""
    scores = np.asarray(scores, dtype=np.float32)
    flat = scores.ravel()
    total = flat.size
    L = min(total, int(capacity))
    with np.errstate(invalid="ignore"):
        valid = flat > np.float32(thr)
    m = int(valid.sum())
    vi = np.nonzero(valid)[0]
    order = vi[np.argsort(-flat[vi].astype(np.float64), kind="stable")]  # -(+0) and -(-0) compare equal: index order
    k = min(m, L)
    flat_idx = np.concatenate([order[:k], np.nonzero(~valid)[0][:L - k]]).astype(np.int64)
    top_s = np.full(L, -1.0, dtype=np.float32)
    top_s[:k] = flat[order[:k]]
    return flat_idx, top_s, m


def candidates(boxes, flat_idx, C):
    """what follows from flat_idx: cand = boxes[i // C], cls = i % C, bev = cand[:, [0, 1, 3, 4, 6]]."""
    boxes = np.asarray(boxes, dtype=np.float32)
    cand = boxes[flat_idx // C]
    return cand, (flat_idx % C).astype(np.int64), cand[:, BEV_COLS]


def padding_contract(boxes, scores, thr, front_idx, cand, top_s, cls, bev, box_of_row):
    """The promise of srf_nms_select's header for the rows past min(m, L), "score -1 and an arbitrary valid box", as assertions
    on those rows (cand, top_s, cls, bev are the rows past the front only; box_of_row their box indices, recovered by the caller
    from a column of `boxes` that names the row; front_idx the flat indices of the front rows)."""
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    n, C = scores.shape
    assert np.all(top_s == np.float32(-1.0)), "a padding row without score -1"
    assert np.all((box_of_row >= 0) & (box_of_row < n) & (cls >= 0) & (cls < C)), "a padding row outside the input"
    with np.errstate(invalid="ignore"):
        assert not np.any(scores[box_of_row, cls] > np.float32(thr)), "a padding row is a pair above the threshold"
    flat = box_of_row.astype(np.int64) * C + cls
    assert np.unique(flat).size == flat.size, "padding rows repeat a pair"
    assert np.intersect1d(flat, front_idx).size == 0, "a padding row repeats a front row"
    assert np.array_equal(cand, boxes[box_of_row]) and np.array_equal(bev, boxes[box_of_row][:, BEV_COLS]), \
        "cand / bev of a padding row are not its pair's box"


# ---------------------------------------------------------------------------------------------------------------- finish
def finish_key(top_s, cls):
    """float32(4 * cls) - float32(2 * clamp(s, 0, 1)), every step rounded to float32: class-major, descending score inside
    a class.  (The key is coarser than the scores for cls >= 1; equal keys keep candidate order, which is score order.)"""
    s = np.clip(np.asarray(top_s, dtype=np.float32), np.float32(0), np.float32(1))
    return (np.asarray(cls).astype(np.float32) * np.float32(4) - s * np.float32(2)).astype(np.float32)


def finish(cand, top_s, cls, keep):
    """-> (perm (L,), kept): survivors (keep != 0) first in a stable sort by finish_key, then the others in candidate order."""
    kp = np.asarray(keep) != 0
    si = np.nonzero(kp)[0]
    key = finish_key(np.asarray(top_s)[si], np.asarray(cls)[si])
    perm = np.concatenate([si[np.argsort(key, kind="stable")], np.nonzero(~kp)[0]]).astype(np.int64)
    return perm, int(si.size)


def packed_rows(cand, top_s, cls, perm):
    """(L, D + 2) float32 rows [box, score, float(label)]: what the graphs read back."""
    cand, top_s, cls = np.asarray(cand, np.float32), np.asarray(top_s, np.float32), np.asarray(cls)
    return np.concatenate([cand[perm], top_s[perm, None], cls[perm, None].astype(np.float32)], axis=1)


# ----------------------------------------------------------------------------------------------------------------- chains
def multiclass_nms(boxes, scores, thr, nms_thr, max_num):
    """The loop of srfdet_head.py:1276-1293 (mmdet3d box3d_multiclass_nms): per class ascending, the boxes with score > thr,
    greedy rotated NMS in descending score (float64), concatenated; then the top max_num by score (ties: the earlier row -- the
    reference's sort leaves them unspecified).  -> (boxes, scores, labels, margin): margin is the smallest |IoU - nms_thr| the
    result rests on."""
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    n, C = scores.shape
    with np.errstate(invalid="ignore"):
        ci, bi = np.nonzero(scores.T > np.float32(thr))  # class-major, box order inside a class
    s = scores[bi, ci]
    kept, margin = R.greedy_nms(boxes[bi][:, BEV_COLS], s, nms_thr, classes=ci)  # descending score, ties by lower row
    kept = kept[np.argsort(ci[kept], kind="stable")]
    if kept.size > max_num:
        kept = kept[np.argsort(-s[kept].astype(np.float64), kind="stable")[:max_num]]
    return boxes[bi[kept]], s[kept], ci[kept].astype(np.int64), margin


def static_chain(boxes, scores, thr, nms_thr, capacity):
    """select -> float64 NMS inside a class over the first min(m, L) rows -> finish.
    -> dict(cand, top_s, cls, bev, m, keep, perm, kept, out_boxes, out_scores, out_labels, packed, counts, margin)."""
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    C = scores.shape[1]
    flat_idx, top_s, m = select(boxes, scores, thr, capacity)
    cand, cls, bev = candidates(boxes, flat_idx, C)
    L = flat_idx.size
    k = min(m, L)
    kept_rows, margin = R.greedy_nms(bev[:k], top_s[:k], nms_thr, classes=cls[:k])
    keep = np.zeros(L, dtype=np.int32)
    keep[kept_rows] = 1
    perm, kept = finish(cand, top_s, cls, keep)
    return dict(flat_idx=flat_idx, cand=cand, top_s=top_s, cls=cls, bev=bev, m=m, keep=keep, perm=perm, kept=kept,
                out_boxes=cand[perm], out_scores=top_s[perm], out_labels=cls[perm], packed=packed_rows(cand, top_s, cls, perm),
                counts=np.array([kept, m], dtype=np.int32), margin=margin)


def results(packed, counts, max_per_img, post_center_range):
    """Host side (SRFDetHead.results_from_static / the end of get_bboxes): per sample the first `kept` rows, cut to the
    max_per_img best by score (ties: the earlier row), then the rows whose centre lies inside post_center_range.
    -> list of (boxes, scores, labels), or None when a sample has more candidates than rows."""
    packed = np.asarray(packed, dtype=np.float32)
    L, D = packed.shape[1], packed.shape[2] - 2
    lo, hi = np.asarray(post_center_range[:3], np.float32), np.asarray(post_center_range[3:], np.float32)
    out = []
    for i in range(packed.shape[0]):
        kept, m = int(counts[i][0]), int(counts[i][1])
        if m > L:
            return None
        rows = packed[i, :kept]
        if kept > max_per_img:
            rows = rows[np.argsort(-rows[:, D].astype(np.float64), kind="stable")[:max_per_img]]
        rows = rows[((rows[:, :3] >= lo) & (rows[:, :3] <= hi)).all(axis=1)]
        out.append((rows[:, :D], rows[:, D], rows[:, D + 1].astype(np.int64)))
    return out


# ----------------------------------------------------------------------------------------------------------------- decode
def decode(logits, pred, pc_range):
    """float64: last-stage logits (..., ncls) and boxes (..., Dd) [centres normalised to the range, log sizes, sin, cos, ...]
    -> (sigmoid(logits), boxes (..., Dd - 1) [centre * extent + lo with z minus h / 2, exp of the sizes, atan2(sin, cos), the
    rest copied]).  pc_range as the float32 values the kernel is given."""
    lg, p = np.asarray(logits, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    r = np.asarray(pc_range, dtype=np.float32)
    lo, ext = r[:3].astype(np.float64), (r[3:] - r[:3]).astype(np.float64)  # the extent is formed in float32, as given
    with np.errstate(over="ignore"):
        scores = 1.0 / (1.0 + np.exp(-lg))
    out = np.empty(p.shape[:-1] + (p.shape[-1] - 1,))
    out[..., :3] = p[..., :3] * ext + lo
    out[..., 3:6] = np.exp(p[..., 3:6])
    out[..., 2] -= out[..., 5] / 2
    out[..., 6] = np.arctan2(p[..., 6], p[..., 7])
    out[..., 7:] = p[..., 8:]
    return scores, out


# ----------------------------------------------------------------------------------------------------------------- scenes
def boxes_from_bev(bev, D, rng):
    """(n, 5) [x, y, w, l, yaw] -> (n, D) rows [x, y, z, w, l, h, yaw, ...] with random z, h and tail columns."""
    n = bev.shape[0]
    out = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    out[:, BEV_COLS] = bev
    out[:, 5] = rng.uniform(1, 2, n).astype(np.float32)
    return out


def distinct_scores(rng, n, C, k, thr):
    """(n, C) float32 scores with exactly k pairs above thr, all of them distinct, at random places; the rest at or below it."""
    s = (rng.uniform(0, 1, n * C) * thr).astype(np.float32)
    s[rng.permutation(n * C)[:n * C // 50]] = np.float32(thr)  # some exactly on the threshold
    v = (np.float32(thr) + (rng.permutation(k) + 1).astype(np.float32) / np.float32(k + 1) * np.float32(1 - thr)).astype(np.float32)
    s[rng.permutation(n * C)[:k]] = v
    assert np.unique(v).size == k and np.all(v > np.float32(thr)) and int((s > np.float32(thr)).sum()) == k
    return s.reshape(n, C)


def scene(kind, seed, D=9):
    """The chain tests' frames -> (boxes (n, D), scores (n, 10), score_thr, nms_thr).  Seeds are chosen (on the CPU) so that no
    IoU the result rests on is within 1e-5 of nms_thr."""
    rng = np.random.default_rng(seed)
    if kind == "crowded":        # 200 boxes on 20 m x 20 m: plenty of overlaps
        n, k = 200, 640
        bev = np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.uniform(1, 4, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1)
        return boxes_from_bev(bev.astype(np.float32), D, rng), distinct_scores(rng, n, 10, k, 0.1), 0.1, 0.4
    if kind == "clusters":       # what five decoder stages leave: 50 objects proposed 18 times each
        bev = R.clustered_scene(seed, objects=50, copies=18)[0]
        return boxes_from_bev(bev, D, rng), distinct_scores(rng, 900, 10, 1600, 0.1), 0.1, 0.2
    if kind == "sparse":         # the NMS keeps more than 1024 of 2048 candidates
        n = 1600
        return boxes_from_bev(R._base(rng, n, span=30), D, rng), distinct_scores(rng, n, 10, 2048, 0.1), 0.1, 0.2
    if kind == "overflow":       # more candidates than the static capacity of 2048
        n = 900
        bev = np.concatenate([rng.uniform(-40, 40, (n, 2)), rng.uniform(1, 4, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1)
        return boxes_from_bev(bev.astype(np.float32), D, rng), distinct_scores(rng, n, 10, 2870, 0.1), 0.1, 0.4
    raise KeyError(kind)
