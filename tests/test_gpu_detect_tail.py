"""The detection tail on the GPU against tests/detect_tail_ref.py: srf_nms_select and srf_nms_finish called directly on both of
their sort paths and on either side of every switch, the static and the dynamic multi-class NMS against the float64 chain,
select_static -> host_pack -> results_from_static against get_bboxes, srf_host_pack past its grid-stride start, and
srf_decode_boxes against float64.  Everything but the decode is selection and permutation and is compared bit for bit.

Decode figures measured on an MI355X are quoted in DESIGN.md section 2 ("the detection tail"); the test prints them
(pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import detect_tail_ref as T

pytestmark = pytest.mark.gpu
F32 = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


# ================================================================================================================= select
def _boxes(rng, n, D):
    """(n, D) float32, all entries distinct enough to tell rows apart; column 2 names the row"""
    b = rng.uniform(-50, 50, (n, D)).astype(F32)
    b[:, 2] = np.arange(n)
    return b


def _select_scores(kind, n, C, m, rng):
    """-> (scores (n, C) float32, thr).  kind "distinct": exactly m pairs above thr, and one entry equal to thr when m < n*C."""
    total = n * C
    v = ((rng.permutation(total) + 1) / (total + 1)).astype(F32)   # distinct values inside (0, 1)
    assert np.unique(v).size == total
    if kind == "distinct":
        thr = float(np.sort(v)[::-1][m]) if m < total else 0.0       # the (m+1)-th best IS the threshold: not a candidate
    elif kind == "shared":      # 30 % of the entries one value, high enough that the capacity cuts inside the block
        v[rng.random(total) < 0.3] = F32(0.9)
        thr = 0.25
    elif kind == "equal":
        v[:] = F32(0.7)
        thr = 0.1
    elif kind == "dup_rows":    # identical proposals: the second half of the boxes repeats the first (the caller copies the boxes)
        v = v.reshape(n, C)
        v[n // 2:2 * (n // 2)] = v[:n // 2]
        thr = 0.5
    elif kind == "special":
        pos = rng.permutation(total)[:3]
        v[pos[0]], v[pos[1]], v[pos[2]] = np.nan, np.inf, -np.inf
        thr = 0.6
    elif kind in ("zeros_out", "zeros_in"):   # +0 and -0 at a threshold of 0 (not candidates), and below it (equal candidates)
        v = (v - F32(0.5)).astype(F32)
        pos = rng.permutation(total)[:min(20, total)]
        v[pos[0::2]], v[pos[1::2]] = F32(0.0), F32(-0.0)
        thr = 0.0 if kind == "zeros_out" else -0.25
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(v.reshape(n, C)), thr


def _check_select(dev, boxes, scores, thr, capacity, unique_rows=True):
    from srfdet3d_amd import ops
    n, C = scores.shape
    tb, ts = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    runs = [ops.nms_select(tb, ts, thr, capacity) for _ in range(2)]
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    cand, top_s, cls, bev, m = [_np(x) for x in runs[0]]
    idx, want_s, want_m = T.select(boxes, scores, thr, capacity)
    want_cand, want_cls, want_bev = T.candidates(boxes, idx, C)
    L = idx.size
    k = min(want_m, L)
    assert cand.shape == want_cand.shape and top_s.shape == (L,) and cls.shape == (L,) and bev.shape == (L, 5) and cls.dtype == np.int64
    assert int(m[0]) == want_m
    assert np.array_equal(_bits(top_s[:k]), _bits(want_s[:k])), "front scores"
    assert np.array_equal(cls[:k], want_cls[:k]) and np.array_equal(cand[:k], want_cand[:k]) and np.array_equal(bev[:k], want_bev[:k])
    if unique_rows:   # the header's promise for the rest, before the exact order
        T.padding_contract(boxes, scores, thr, idx[:k], cand[k:], top_s[k:], cls[k:], bev[k:], cand[k:, 2].astype(np.int64))
    assert np.all(top_s[k:] == F32(-1))
    # ... and the order both sort paths give them: the pairs at or below the threshold by ascending flat index
    assert np.array_equal(cls[k:], want_cls[k:]) and np.array_equal(cand[k:], want_cand[k:]) and np.array_equal(bev[k:], want_bev[k:])
    return want_m, L


# (n, C, D): every n * C the issue names, C in {1, 3, 10, 32} (8 for the 2048 x 8 maximum), D in {7, 9, 10}
SHAPES = [(1, 1, 7), (21, 3, 9), (2, 32, 10), (65, 1, 7), (100, 10, 9), (32, 32, 10), (1025, 1, 7), (2047, 1, 9), (64, 32, 10), (683, 3, 7),
          (900, 10, 9), (2048, 8, 10), (16384, 1, 7)]


@pytest.mark.parametrize("n,C,D", SHAPES)
def test_select_sizes(dev, n, C, D):
    """every size at a third of the pairs above the threshold, at none and at all of them (capacity 2048)"""
    rng = np.random.default_rng(n * 31 + C)
    boxes = _boxes(rng, n, D)
    for m in sorted({0, (n * C + 2) // 3, n * C}):
        scores, thr = _select_scores("distinct", n, C, m, rng)
        got_m, L = _check_select(dev, boxes, scores, thr, 2048)
        assert got_m == m and L == min(n * C, 2048)


@pytest.mark.parametrize("n,C,m", [(900, 10, m) for m in (0, 1, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 9000)]
                         + [(205, 10, m) for m in (2047, 2048, 2049, 2050)] + [(2048, 8, m) for m in (1024, 1025, 4000)])
def test_select_candidate_counts(dev, n, C, m):
    """m alone picks the sort path: the rank sort up to 1024 candidates, the bitonic sort of all pairs beyond; L = 2048"""
    rng = np.random.default_rng(m * 7 + n)
    scores, thr = _select_scores("distinct", n, C, m, rng)
    got_m, L = _check_select(dev, _boxes(rng, n, 9), scores, thr, 2048)
    assert got_m == m and L == 2048


@pytest.mark.parametrize("n,C,m,capacity", [(900, 10, 500, 100), (900, 10, 3000, 4096), (900, 10, 5000, 4096), (100, 10, 300, 2048),
                                            (100, 10, 1000, 2048), (100, 10, 1000, 1000), (100, 10, 700, 999), (2048, 8, 16384, 4096),
                                            (16384, 1, 300, 4096), (900, 10, 1200, 1100), (3, 3, 4, 5000)])
def test_select_capacities(dev, n, C, m, capacity):
    """capacity below m on the rank path and on the bitonic path, above n * C (then L = n * C), and the kernel's 4096"""
    rng = np.random.default_rng(capacity * 13 + m)
    scores, thr = _select_scores("distinct", n, C, m, rng)
    got_m, L = _check_select(dev, _boxes(rng, n, 7), scores, thr, capacity)
    assert got_m == m and L == min(n * C, capacity)


@pytest.mark.parametrize("kind", ["shared", "equal", "dup_rows", "special", "zeros_out", "zeros_in"])
@pytest.mark.parametrize("n,C", [(100, 10), (900, 10), (683, 3)])
def test_select_score_values(dev, kind, n, C):
    """ties (lower flat index first, on both paths), identical proposals, NaN / +inf / -inf, +-0 on and above the threshold"""
    rng = np.random.default_rng(n + len(kind))
    boxes = _boxes(rng, n, 9)
    scores, thr = _select_scores(kind, n, C, 0, rng)
    if kind == "dup_rows":
        boxes[n // 2:2 * (n // 2)] = boxes[:n // 2]
    for capacity in (2048, 300):
        m, L = _check_select(dev, boxes, scores, thr, capacity, unique_rows=kind != "dup_rows")
    if kind == "special":
        assert m == int((scores > F32(thr)).sum()) and np.isnan(scores).sum() == 1     # NaN is no candidate, +inf is the first
    if kind == "shared":   # a capacity cuts inside the block of equal scores
        ranked, cut = T.select(boxes, scores, thr, n * C)[1], 2048 if n * C == 9000 else 300
        assert m > cut and ranked[cut - 1] == ranked[cut] == F32(0.9)


def test_select_rejects_more_than_16384_pairs(dev):
    from srfdet3d_amd import ops
    with pytest.raises(RuntimeError, match="nms_select failed"):
        ops.nms_select(torch.zeros(16385, 7, device=dev), torch.zeros(16385, 1, device=dev), 0.1, 2048)
    torch.cuda.synchronize()


# ================================================================================================================= finish
def _finish_inputs(L, D, rng):
    """candidates shaped as select emits them: descending scores with ties and a tail of -1, classes 0 .. 31; the first scores
    above 1 (the clamp gives them one key inside a class: candidate order decides)"""
    live = max(1, L - L // 8)
    top_s = np.sort((np.round(rng.uniform(0.1, 1, L) * 256) / 256).astype(F32))[::-1].copy()
    head = np.array([3.0, 1.5, 1.5, 1.25, 1.0], dtype=F32)[:min(5, L)]
    top_s[:head.size] = head
    top_s[live:] = -1
    cls = rng.integers(0, 32, L).astype(np.int64)
    cls[:head.size] = 5
    return rng.uniform(-50, 50, (L, D)).astype(F32), top_s, cls


def _keep_pattern(name, L, rng):
    keep = np.zeros(L, dtype=np.int32)
    if name == "all":
        keep[:] = 1
    elif name == "first":
        keep[0] = 1
    elif name == "last":
        keep[-1] = 1
    elif name == "random":
        keep[:] = rng.random(L) < 0.5
    elif name == "flags":       # any non-zero flag is a survivor
        keep[:] = rng.choice(np.array([0, 1, 7, -1], dtype=np.int32), L)
    elif name.startswith("exactly"):
        keep[rng.permutation(L)[:int(name[7:])]] = 1
    elif name != "none":
        raise KeyError(name)
    return keep


FINISH = [(1, "none"), (1, "all"), (64, "random"), (64, "flags"), (1000, "all"), (1000, "random"), (1024, "all"), (1024, "first"),
          (1025, "all"), (1025, "last"), (1025, "random"), (2048, "exactly1024"), (2048, "exactly1025"), (2048, "none"),
          (2048, "flags"), (2048, "all"), (4096, "all"), (4096, "random"), (4096, "first"), (4096, "last"), (4096, "exactly1025")]


@pytest.mark.parametrize("L,pattern", FINISH)
def test_finish(dev, L, pattern):
    """srf_nms_finish on synthetic keep flags, with and without the packed output: every one of the L rows of every output"""
    from srfdet3d_amd import ops
    rng = np.random.default_rng(L * 3 + len(pattern))
    D = 7 if L % 2 else 9
    cand, top_s, cls = _finish_inputs(L, D, rng)
    keep = _keep_pattern(pattern, L, rng)
    perm, kept = T.finish(cand, top_s, cls, keep)
    want_packed = T.packed_rows(cand, top_s, cls, perm)
    tc, tt, tl, tk = (torch.from_numpy(x).to(dev) for x in (cand, top_s, cls, keep))
    m = torch.tensor([12345], dtype=torch.int32, device=dev)
    for with_m in (True, False, True):
        out = ops.nms_finish(tc, tt, tl, tk, m) if with_m else ops.nms_finish(tc, tt, tl, tk)
        torch.cuda.synchronize()
        assert len(out) == (6 if with_m else 4)
        ob, os_, ol, k = [_np(x) for x in out[:4]]
        assert int(k[0]) == kept
        assert np.array_equal(ol, cls[perm]) and ol.dtype == np.int64
        assert np.array_equal(_bits(os_), _bits(top_s[perm])) and np.array_equal(_bits(ob), _bits(cand[perm]))
        if with_m:
            assert np.array_equal(_bits(_np(out[4])), _bits(want_packed)) and _np(out[5]).tolist() == [kept, 12345]
    if pattern.startswith("exactly") or pattern == "all":
        assert kept == (L if pattern == "all" else int(pattern[7:]))


def test_finish_rejects_more_than_4096_rows(dev):
    from srfdet3d_amd import ops
    z = torch.zeros(4097, device=dev)
    with pytest.raises(RuntimeError, match="nms_finish failed"):
        ops.nms_finish(torch.zeros(4097, 7, device=dev), z, z.long(), z.int())
    torch.cuda.synchronize()


# ================================================================================================================== chain
@functools.lru_cache(maxsize=None)
def _scene_ref(kind):
    boxes, scores, thr, nms_thr = T.scene(kind, 0)
    ch = T.static_chain(boxes, scores, thr, nms_thr, 2048)
    full = T.multiclass_nms(boxes, scores, thr, nms_thr, 10 ** 6)
    above = scores[scores > F32(thr)]
    assert np.unique(above).size == above.size, "scores above the threshold must be distinct"
    assert ch["margin"] >= 1e-5 and full[3] >= 1e-5, "an IoU of the scene is on the NMS threshold"
    return boxes, scores, thr, nms_thr, ch, full


def _cut(full, max_num):
    b, s, l = full[:3]
    if s.size > max_num:
        top = np.argsort(-s.astype(np.float64), kind="stable")[:max_num]
        b, s, l = b[top], s[top], l[top]
    return b, s, l


def _same_rows(got, want, what):
    gb, gs, gl = [_np(x) for x in got]
    assert gb.shape == want[0].shape and gl.dtype == np.int64, what
    assert np.array_equal(gl, want[2]), what + ": labels"
    assert np.array_equal(_bits(gs), _bits(want[1])), what + ": scores"
    assert np.array_equal(_bits(gb), _bits(want[0])), what + ": boxes"


@pytest.mark.parametrize("kind", ["crowded", "clusters", "sparse", "overflow"])
def test_chain_is_the_definition(dev, kind):
    """Every path of the multi-class NMS returns the definition's rows, in its order: the fused static path (all L rows, unpacked
    and packed), its torch twin, the dynamic path and the per-class loop, with and without the max_num cut.  "overflow" has more
    candidates than the static capacity: counts[1] says so, the L rows are still the chain over the best L, and the dynamic
    paths give the whole answer."""
    from srfdet3d_amd import postprocess as P
    boxes, scores, thr, nms_thr, ch, full = _scene_ref(kind)
    tb, ts = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    L, k, m = ch["perm"].size, ch["kept"], ch["m"]
    assert (m > L) == (kind == "overflow") and (k > 1024) == (kind in ("sparse", "overflow"))
    sb, ss, sl, kept, cand = P.box3d_multiclass_nms_static(tb, ts, thr, nms_thr)
    assert int(kept.item()) == k and int(cand.item()) == m and kept.dtype == torch.int32 and cand.dtype == torch.int32
    _same_rows((sb, ss, sl), (ch["out_boxes"], ch["out_scores"], ch["out_labels"]), "static")
    packed, counts = P.box3d_multiclass_nms_static(tb, ts, thr, nms_thr, want_packed=True)
    assert np.array_equal(_bits(_np(packed)), _bits(ch["packed"])) and _np(counts).tolist() == [k, m]
    tb_, ts_, tl_, tkept, tcand = P._static_torch(tb, ts, thr, nms_thr, L)
    assert int(tkept.item()) == k and int(tcand.item()) == m
    d = min(m, L)           # past the candidates torch.topk orders equal keys as it likes
    _same_rows((tb_[:d], ts_[:d], tl_[:d]), (ch["out_boxes"][:d], ch["out_scores"][:d], ch["out_labels"][:d]), "_static_torch")
    if kind != "overflow":  # the static rows are the dynamic answer
        _same_rows((sb[:k], ss[:k], sl[:k]), full[:3], "static against the per-class loop")
    for max_num in (10 ** 6, 300):
        want = _cut(full, max_num)
        _same_rows(P.box3d_multiclass_nms(tb, ts, thr, max_num, nms_thr), want, f"dynamic, max_num {max_num}")
        _same_rows(P._per_class_nms(tb, ts, thr, max_num, nms_thr), want, f"per class, max_num {max_num}")


def test_chain_order_does_not_rest_on_the_float_key(dev):
    """Two survivors of class 9 whose scores differ by one ulp share the float32 key 4 * class - 2 * score (both round to 35).  The
    reference's per-class loop lists the higher score first; here it sits at the HIGHER box index, so an order that falls back
    to the box index is wrong.  (postprocess.box3d_multiclass_nms did that until this test: it sorted its survivors by that key.)"""
    from srfdet3d_amd import postprocess as P
    n, C = 8, 10
    rng = np.random.default_rng(5)
    bev = np.stack([np.arange(n) * 20.0 - 70, np.zeros(n), np.full(n, 2.0), np.full(n, 4.0), np.zeros(n)], 1).astype(F32)   # disjoint
    boxes = T.boxes_from_bev(bev, 9, rng)
    scores = np.zeros((n, C), dtype=F32)
    scores[1, 9], scores[6, 9] = F32(0.5), np.nextafter(F32(0.5), F32(1))
    scores[2, 8], scores[5, 8] = np.nextafter(F32(0.25), F32(0)), F32(0.25)
    scores[3, 0], scores[4, 9], scores[0, 3] = 0.9, 0.8, 0.3
    want = T.multiclass_nms(boxes, scores, 0.1, 0.2, 10 ** 6)
    assert want[1].size == 7 and want[2].tolist() == [0, 3, 8, 8, 9, 9, 9]
    assert np.array_equal(want[0][2:4, 0], bev[[5, 2], 0]) and np.array_equal(want[0][4:, 0], bev[[4, 6, 1], 0])
    tb, ts = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    sb, ss, sl, kept, cand = P.box3d_multiclass_nms_static(tb, ts, 0.1, 0.2)
    assert int(kept.item()) == 7 and int(cand.item()) == 7
    _same_rows((sb[:7], ss[:7], sl[:7]), want[:3], "static")
    _same_rows(P._per_class_nms(tb, ts, 0.1, 10 ** 6, 0.2), want[:3], "per class")
    _same_rows(P.box3d_multiclass_nms(tb, ts, 0.1, 10 ** 6, 0.2), want[:3], "dynamic")


# ============================================================================================================== head level
RANGE = [-40.0, -40.0, -5.0, 40.0, 40.0, 5.0]


def _head(C):
    from srfdet3d_amd.plugin import heads
    hd = object.__new__(heads.SRFDetHead)
    torch.nn.Module.__init__(hd)
    hd.use_nms, hd.num_classes = True, C
    hd.test_cfg = dict(score_thr=0.1, nms_thr=0.2, max_per_img=300, post_center_range=RANGE)
    return hd


def _sample(seed, n, C, D, m):
    """n small boxes spread over +-50 m (few overlaps: most candidates survive; a fifth of the centres outside RANGE)"""
    rng = np.random.default_rng(seed)
    bev = np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(0.5, 2, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(F32)
    return T.boxes_from_bev(bev, D, rng), T.distinct_scores(rng, n, C, m, 0.1)


def _static_results(hd, scores, boxes, metas, dev):
    """select_static -> the one packed vector -> the host -> the slicing GraphedFrame.__call__ does -> results_from_static"""
    from srfdet3d_amd import graphs
    packed, counts = hd.select_static(scores, boxes)
    levels = torch.tensor([5, 17, 2 ** 24 - 1], dtype=torch.int32, device=dev)
    h = graphs.GraphedFrame._host_pack((packed, counts), levels).cpu()
    n_pk, n_c = packed.numel(), counts.numel()
    pk, cn = h[:n_pk].view(packed.shape), h[n_pk:n_pk + n_c].to(torch.int32).view(counts.shape)
    assert h[n_pk + n_c:].to(torch.int64).tolist() == [5, 17, 2 ** 24 - 1]
    assert torch.equal(pk, packed.cpu()) and torch.equal(cn, counts.cpu())
    return hd.results_from_static(pk, cn, metas), cn


@pytest.mark.parametrize("D", [9, 7])
@pytest.mark.parametrize("ms", [(700,), (0,), (700, 250), (0, 700), (250, 2500)])
def test_head_static_results_equal_get_bboxes(dev, D, ms):
    """bs = 1 and 2; a sample whose survivors exceed max_per_img = 300, one with no candidate, and one over the static capacity
    (the whole batch is then None: the caller redoes the frame with get_bboxes)"""
    from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes
    n, C = 300, 10
    hd = _head(C)
    pairs = [_sample(11 * i + m + D, n, C, D, m) for i, m in enumerate(ms)]
    boxes = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    scores = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    metas = [dict(box_type_3d=LiDARInstance3DBoxes)] * len(ms)
    static, counts = _static_results(hd, scores, boxes, metas, dev)
    assert counts[:, 1].tolist() == list(ms)
    dynamic = hd.get_bboxes(None, None, metas, decoded=(scores, boxes))
    if max(ms) > 2048:
        assert static is None
        return
    assert len(static) == len(dynamic) == len(ms)
    for i, m in enumerate(ms):
        sb, ss, sl = static[i]
        db, ds, dl = dynamic[i]
        assert sb.tensor.shape == (ss.numel(), D) and sl.dtype == torch.int64
        assert torch.equal(sb.tensor, db.tensor.cpu()) and torch.equal(ss, ds.cpu()) and torch.equal(sl, dl.cpu())
        kept = int(counts[i, 0])
        if m == 700:     # the cut took place, and the range filter removed rows after it
            assert kept > 300 and 100 < ss.numel() < 300
            assert torch.all(ss[:-1] > ss[1:])
        if m == 0:
            assert kept == 0 and ss.numel() == 0


def test_select_static_graph_replays_equal_eager(dev):
    """select_static and the pack captured once on one stream and replayed on frames with 0, ~500, ~1500 and more than L
    candidates, in an order that shrinks as well as grows: every replay is the eager result of the same frame, so no row, count
    or LDS state of an earlier replay survives."""
    from srfdet3d_amd import ops
    n, C, D = 300, 10, 9
    hd = _head(C)
    frames = [_sample(40 + m, n, C, D, m) for m in (1500, 0, 2500, 500, 0)]
    sbuf, bbuf = torch.zeros(1, n, C, device=dev), torch.zeros(1, n, D, device=dev)
    levels = torch.tensor([3, 4], dtype=torch.int32, device=dev)

    def run():
        sel = hd.select_static(sbuf, bbuf)
        return ops.host_pack(sel[0], sel[1], levels)

    bbuf.copy_(torch.from_numpy(frames[0][0]).unsqueeze(0))
    sbuf.copy_(torch.from_numpy(frames[0][1]).unsqueeze(0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = run()
    torch.cuda.synchronize()
    L = min(n * C, 2048)
    for (b, s), m in zip(frames, (1500, 0, 2500, 500, 0)):
        bbuf.copy_(torch.from_numpy(b).unsqueeze(0))
        sbuf.copy_(torch.from_numpy(s).unsqueeze(0))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = run()
        torch.cuda.synchronize()
        assert torch.equal(got, want), m
        assert got[L * (D + 2):].tolist()[1:] == [float(m), 3.0, 4.0]


# =============================================================================================================== host_pack
@pytest.mark.parametrize("na,nb,nc", [(0, 0, 5), (5, 0, 0), (0, 2, 0), (262143 - 5, 2, 3), (262144 - 5, 2, 3), (262145 - 5, 2, 3),
                                      (262144, 1, 0), (6 * 4096 * 12, 12, 8)])
def test_host_pack_sizes(dev, na, nb, nc):
    """one block-stride pass covers 1024 x 256 = 262144 elements: below, on and past it, and the largest frame a graph ships
    (six samples of 4096 rows); integers up to 2^24 - 1 arrive exactly"""
    from srfdet3d_amd import ops
    g = torch.Generator().manual_seed(na + nb + nc)
    a = torch.randn(na, generator=g).to(dev)
    b = torch.randint(0, 2 ** 24, (nb,), generator=g, dtype=torch.int32).to(dev)
    c = torch.randint(0, 2 ** 24, (nc,), generator=g, dtype=torch.int32).to(dev)
    if nb:
        b[-1] = 2 ** 24 - 1
    if nc:
        c[0] = 2 ** 24 - 1
    out = ops.host_pack(a, b, c)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and torch.equal(out, torch.cat([a, b.float(), c.float()]))
    assert torch.equal(out[na:].long(), torch.cat([b, c]).long())


# ============================================================================================================ decode_boxes
PC_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
_SPECIAL_LOGITS = [0.0, 30.0, -30.0, 100.0, -100.0, 17.5, -17.5]
_SPECIAL_SINCOS = [(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 0.0), (-0.0, -1.0), (1e-30, -1.0), (0.6, 0.8), (-0.6, -0.8)]


def _decode_inputs(lead, ncls, Dd, seed):
    rng = np.random.default_rng(seed)
    R = int(np.prod(lead))
    logits = (rng.standard_normal((R, ncls)) * 3).astype(F32)
    pred = rng.standard_normal((R, Dd)).astype(F32)
    pred[:, :3] = rng.uniform(0, 1, (R, 3))
    pred[:, 3:6] = rng.uniform(-3, 4, (R, 3))
    ang, mag = rng.uniform(-np.pi, np.pi, R), rng.uniform(0.05, 2, R)          # all four quadrants, not normalised
    pred[:, 6], pred[:, 7] = np.sin(ang) * mag, np.cos(ang) * mag
    for r in range(0, R, 2):          # every other row carries one of the planted values
        logits[r, r % ncls] = _SPECIAL_LOGITS[(r // 2) % len(_SPECIAL_LOGITS)]
        pred[r, 6], pred[r, 7] = _SPECIAL_SINCOS[(r // 2) % len(_SPECIAL_SINCOS)]
        pred[r, 3 + r % 3] = [-3.0, 4.0, 0.0][(r // 2) % 3]
    return logits.reshape(*lead, ncls), pred.reshape(*lead, Dd)


def _ulps(x, ref, unit=None):
    """max |x - ref| in float32 ulps of the reference value (of `unit` where the value is a difference of larger terms)"""
    unit = np.abs(ref) if unit is None else unit
    return float(np.max(np.abs(x.astype(np.float64) - ref) / np.spacing(unit.astype(F32)).astype(np.float64))) if ref.size else 0.0


@pytest.mark.parametrize("lead,ncls,Dd", [((1,), 1, 8), ((127,), 3, 10), ((128,), 10, 8), ((129,), 1, 10), ((2, 900), 10, 10), ((2, 900), 3, 8)])
def test_decode_boxes_against_float64(dev, lead, ncls, Dd):
    """srf_decode_boxes against detect_tail_ref.decode.  The centres equal torch's float32 multiply-then-add bit for bit and the
    tail columns are copies.  For the columns that go through expf / atan2f / the sigmoid no tolerance is fixed in advance: e_torch
    is the error of torch's own float32 ops on the same inputs against float64, in ulps of the value, and
    e_hip <= 2 * max(e_torch, 1 ulp).  z = centre - h / 2 is a difference: its unit is the ulp of its larger term."""
    from srfdet3d_amd import ops
    from srfdet3d_amd.plugin.bbox_util import denormalize_bbox
    logits, pred = _decode_inputs(lead, ncls, Dd, 7 * ncls + Dd + int(np.prod(lead)))
    want_s, want_b = T.decode(logits, pred, PC_RANGE)
    tl, tp = torch.from_numpy(logits).to(dev), torch.from_numpy(pred).to(dev)
    scores, boxes = ops.decode_boxes(tl, tp, PC_RANGE)
    torch.cuda.synchronize()
    assert scores.shape == tl.shape and boxes.shape == (*lead, Dd - 1)
    lo = torch.tensor(PC_RANGE[:3], device=dev)
    ext = torch.tensor(PC_RANGE[3:], device=dev) - lo
    mid = tp.clone()
    mid[..., :3] = mid[..., :3] * ext + lo
    tref = denormalize_bbox(mid, PC_RANGE)
    tref[..., 2] = tref[..., 2] - tref[..., 5] * 0.5
    tref_s = torch.sigmoid(tl)
    assert torch.equal(boxes[..., :2], mid[..., :2]) and torch.equal(boxes[..., 7:], tp[..., 8:])
    hb, hs, tb, ts = _np(boxes), _np(scores), _np(tref), _np(tref_s)
    assert np.isfinite(hb).all() and np.all((hs >= 0) & (hs <= 1))
    z_unit = np.maximum(np.maximum(np.abs(want_b[..., 2] + want_b[..., 5] / 2), want_b[..., 5] / 2), np.abs(want_b[..., 2]))
    cols = [("score", hs, ts, want_s, None), ("z", hb[..., 2], tb[..., 2], want_b[..., 2], z_unit)]
    cols += [(name, hb[..., c], tb[..., c], want_b[..., c], None) for name, c in (("w", 3), ("l", 4), ("h", 5), ("yaw", 6))]
    figures = {name: (_ulps(h, w, u), _ulps(t, w, u)) for name, h, t, w, u in cols}
    print(f"\ndecode_boxes {lead} ncls {ncls} Dd {Dd}: (e_hip, e_torch) in ulps " + "  ".join(f"{k} {a:.2f}/{b:.2f}" for k, (a, b) in figures.items()))
    for name, (e_hip, e_torch) in figures.items():
        assert e_hip <= 2 * max(e_torch, 1.0), (name, e_hip, e_torch)
