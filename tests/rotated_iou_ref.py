"""float64 reference of the rotated BEV IoU and of the greedy NMS built on it, and the generators of the box pairs the NMS and
the OTA assigner actually meet (clusters of nearly identical boxes, a box on its ground truth) next to pairs in general
position.  Plain numpy, no project kernel.

Boxes are (cx, cy, w, h, yaw[rad]).  The intersection is a Sutherland-Hodgman clip of a's corners against b's four edges, in
float64, in coordinates relative to a's centre (exact for float32 inputs), vectorised over pairs; pairs whose circumscribed
circles are disjoint are 0 without a clip.  The project's kernel computes the same quantity by another method (a boundary
integral in a's frame), so agreement is not by construction."""
import numpy as np

ZERO_AREA = 1e-14  # a box with w * h below this has IoU 0 with everything (the kernel's and mmcv's rule)


def _corners(b, origin):
    """(k, 5) float64 boxes -> (k, 4, 2) corners relative to `origin` (k, 2), counter-clockwise for positive sizes."""
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    lx = np.array([-0.5, 0.5, 0.5, -0.5])[None, :] * b[:, 2:3]
    ly = np.array([-0.5, -0.5, 0.5, 0.5])[None, :] * b[:, 3:4]
    x = (b[:, 0] - origin[:, 0])[:, None] + lx * c[:, None] - ly * s[:, None]
    y = (b[:, 1] - origin[:, 1])[:, None] + lx * s[:, None] + ly * c[:, None]
    return np.stack([x, y], axis=2)


def _clip_area(S, C):
    """area of (convex quadrilateral S) and (counter-clockwise convex quadrilateral C), both (k, 4, 2) float64 -> (k,)."""
    k = S.shape[0]
    rows = np.arange(k)
    P = np.zeros((k, 9, 2))
    P[:, :4] = S
    cnt = np.full(k, 4, dtype=np.int64)
    for i in range(4):
        p0 = C[:, i]
        e = C[:, (i + 1) % 4] - p0
        d = P - p0[:, None, :]
        side = e[:, None, 0] * d[:, :, 1] - e[:, None, 1] * d[:, :, 0]  # >= 0: inside this edge's half-plane
        Q = np.zeros_like(P)
        m = np.zeros(k, dtype=np.int64)
        for j in range(8):
            act = j < cnt
            if not act.any():
                break
            kp = np.where(act, cnt - 1, 0) if j == 0 else np.full(k, j - 1, dtype=np.int64)
            cur, prv = P[:, j], P[rows, kp]
            sc, sp = side[:, j], side[rows, kp]
            r = rows[act & ((sc >= 0) != (sp >= 0))]
            if r.size:
                t = sp[r] / (sp[r] - sc[r])
                Q[r, m[r]] = prv[r] + t[:, None] * (cur[r] - prv[r])
                m[r] += 1
            r = rows[act & (sc >= 0)]
            if r.size:
                Q[r, m[r]] = cur[r]
                m[r] += 1
        P, cnt = Q, m
    area = np.zeros(k)
    for j in range(8):
        act = j < cnt
        if not act.any():
            break
        nx = np.where(j + 1 < cnt, j + 1, 0)
        a, b = P[:, j], P[rows, nx]
        area += np.where(act, a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0], 0.0)
    return np.where(cnt >= 3, 0.5 * np.abs(area), 0.0)


def _as_boxes(x):
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] != 5:
        raise ValueError("boxes must be (k, 5)")
    return x


def _live(x):
    """the zero-area rule, on the product in the boxes' own precision (float32 inputs: the kernel's float32 product)."""
    return ~(x[:, 2] * x[:, 3] < ZERO_AREA)


def intersection_pairs(a, b):
    """a, b (k, 5): intersection area of a[i] and b[i], (k,) float64.  0 where either box has zero area."""
    a, b = _as_boxes(a), _as_boxes(b)
    ok = _live(a) & _live(b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    out = np.zeros(a.shape[0])
    idx = np.nonzero(ok)[0]
    for c0 in range(0, idx.size, 200000):
        r = idx[c0:c0 + 200000]
        out[r] = _clip_area(_corners(a[r], a[r, :2]), _corners(b[r], a[r, :2]))
    return out


def iou_pairs(a, b):
    """a, b (k, 5) -> IoU of a[i] and b[i], (k,) float64."""
    inter = intersection_pairs(a, b)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    union = a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3] - inter
    return np.where(inter > 0, inter / np.where(inter > 0, union, 1.0), 0.0)


def intersection(a, b):
    """a (n, 5), b (m, 5) -> (n, m) float64 intersection areas."""
    a, b = _as_boxes(a), _as_boxes(b)
    n, m = a.shape[0], b.shape[0]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    # boxes whose circumscribed circles are disjoint do not meet
    ra, rb = 0.5 * np.hypot(a64[:, 2], a64[:, 3]), 0.5 * np.hypot(b64[:, 2], b64[:, 3])
    out = np.zeros((n, m))
    for i0 in range(0, n, 1024):
        sl = slice(i0, i0 + 1024)
        d2 = (a64[sl, 0:1] - b64[None, :, 0]) ** 2 + (a64[sl, 1:2] - b64[None, :, 1]) ** 2
        near = d2 <= ((ra[sl, None] + rb[None, :]) * (1 + 1e-9)) ** 2
        i, j = np.nonzero(near)
        if i.size:
            out[i0 + i, j] = intersection_pairs(a[i0 + i], b[j])
    return out


def iou(a, b):
    """a (n, 5), b (m, 5), float32 (or float64, then taken as they are) -> (n, m) float64 IoU."""
    inter = intersection(a, b)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    union = (a[:, 2] * a[:, 3])[:, None] + (b[:, 2] * b[:, 3])[None, :] - inter
    return np.where(inter > 0, inter / np.where(inter > 0, union, 1.0), 0.0)


def greedy_nms(boxes, scores, thr, classes=None):
    """Greedy NMS in descending score, ties by lower index first: a box is dropped when a kept box of higher rank (and of its
    class, when classes are given) has IoU > thr with it.  Returns (kept indices in that order, margin): margin is the smallest
    |IoU - thr| over every pair (kept box, box of lower rank and the same class), i.e. every comparison the result rests on."""
    boxes = _as_boxes(boxes)
    n = boxes.shape[0]
    scores = np.asarray(scores)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    if n == 0:
        return order, np.inf
    sb = boxes[order]
    m = iou(sb, sb)
    if classes is not None:
        c = np.asarray(classes)[order]
        same = c[:, None] == c[None, :]
    dead = np.zeros(n, dtype=bool)
    keep, margin = [], np.inf
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        row = m[i, i + 1:]
        if classes is not None:
            row = row[same[i, i + 1:]]
            dead[i + 1:][same[i, i + 1:]] |= row > thr
        else:
            dead[i + 1:] |= row > thr
        if row.size:
            margin = min(margin, float(np.abs(row - thr).min()))
    return order[np.array(keep, dtype=np.int64)], margin


# ------------------------------------------------------------------------------------------------------------------ generators
# Every pair generator returns (a, b) float32 with a of shape (groups * p, 5) and b of shape (groups * q, 5): inside a group all
# p * q pairs are of the generator's kind; pairs across groups are boxes in general position (mostly disjoint).
PI32 = np.float32(np.pi)
# typical (w, l) of the ten nuScenes classes (the dataset's published mean sizes): 0.4 m cones and 0.7 m pedestrians to 12 m buses
CLASS_SIZES = np.array([[1.95, 4.60], [2.50, 6.90], [2.80, 6.40], [2.95, 11.00], [2.90, 12.30], [2.50, 0.50], [0.77, 2.10],
                        [0.60, 1.70], [0.67, 0.73], [0.41, 0.41]], dtype=np.float32)


def _base(rng, k, offset=0.0, span=50.0):
    return np.stack([offset + rng.uniform(-span, span, k), offset + rng.uniform(-span, span, k), 0.3 + rng.uniform(0, 10, k),
                     0.3 + rng.uniform(0, 5, k), rng.uniform(-np.pi, np.pi, k)], axis=1).astype(np.float32)


def _jitter(rng, x, rel):
    """x + U(-1, 1) * rel * (1 m for the centre, the value itself for w, h, yaw), in float32 like a decoder's output."""
    scale = np.concatenate([np.ones_like(x[:, :2]), x[:, 2:]], axis=1)
    r = np.asarray(rel, dtype=np.float64).reshape(-1, 1)  # one value, or one per box
    return (x + (rng.uniform(-1, 1, x.shape) * r * scale).astype(np.float32)).astype(np.float32)


def _groups(x, reps):
    return np.repeat(x, reps, axis=0)


def random_overlapping(seed, groups, p, q):
    rng = np.random.default_rng(seed)
    a, b = _base(rng, groups * p), _base(rng, groups * q)
    c0 = rng.uniform(-50, 50, (groups, 2)).astype(np.float32)
    a[:, :2] = _groups(c0, p) + rng.uniform(-2, 2, (groups * p, 2)).astype(np.float32)
    b[:, :2] = _groups(c0, q) + rng.uniform(-2, 2, (groups * q, 2)).astype(np.float32)
    return a, b


def identical(seed, groups, p, q):
    x = _base(np.random.default_rng(seed), groups)
    return _groups(x, p), _groups(x, q)


def near_duplicate(seed, groups, p, q, rel=1e-5, offset=0.0):
    rng = np.random.default_rng(seed)
    x = _base(rng, groups, offset)
    return _jitter(rng, _groups(x, p), rel), _jitter(rng, _groups(x, q), rel)


def near_duplicate_far(seed, groups, p, q):
    """centres around x, y = 3000 m, jitter 1e-4"""
    return near_duplicate(seed, groups, p, q, rel=1e-4, offset=3000.0)


def yaw_plus_pi(seed, groups, p, q):
    x = _base(np.random.default_rng(seed), groups)
    y = x.copy()
    y[:, 4] = x[:, 4] + PI32
    return _groups(x, p), _groups(y, q)


def swapped_axes(seed, groups, p, q):
    """the same rectangle written as (h, w, yaw + pi/2)"""
    x = _base(np.random.default_rng(seed), groups)
    y = x.copy()
    y[:, 2], y[:, 3], y[:, 4] = x[:, 3], x[:, 2], x[:, 4] + PI32 / np.float32(2)
    return _groups(x, p), _groups(y, q)


def grid_aligned(seed, groups, p, q):
    """axis-aligned boxes on integer coordinates, yaw in {0, pi/2, pi, 3pi/2}: every edge parallel to one of the other box"""
    rng = np.random.default_rng(seed)
    c0 = rng.integers(-40, 41, (groups, 2))

    def draw(k, reps, quarter):
        return np.concatenate([_groups(c0, reps) + rng.integers(-2, 3, (k, 2)), rng.integers(1, 5, (k, 2)),
                               rng.integers(0, 4 if quarter else 1, (k, 1)) * (np.pi / 2)], axis=1).astype(np.float32)
    return draw(groups * p, p, False), draw(groups * q, q, True)


def nested_corner(seed, groups, p, q):
    """a smaller box of the same yaw inside, sharing one corner and two edges with the larger one"""
    rng = np.random.default_rng(seed)
    x = _base(rng, groups)
    a = _groups(x, p)
    o = _groups(x, q)
    f = rng.uniform(0.2, 0.9, groups * q).astype(np.float32)
    b = o.copy()
    b[:, 2], b[:, 3] = o[:, 2] * f, o[:, 3] * f
    c, s = np.cos(o[:, 4]), np.sin(o[:, 4])
    dx, dy = (o[:, 2] - b[:, 2]) / 2, (o[:, 3] - b[:, 3]) / 2
    sx, sy = rng.choice([-1.0, 1.0], groups * q).astype(np.float32), rng.choice([-1.0, 1.0], groups * q).astype(np.float32)
    b[:, 0] = o[:, 0] + sx * dx * c - sy * dy * s
    b[:, 1] = o[:, 1] + sx * dx * s + sy * dy * c
    return a, b.astype(np.float32)


def thin_near_duplicate(seed, groups, p, q):
    """aspect ratio 100 (10-20 m by 0.1-0.2 m), copies moved by 1e-4 in every coordinate"""
    rng = np.random.default_rng(seed)
    x = _base(rng, groups)
    x[:, 2] = rng.uniform(10, 20, groups)
    x[:, 3] = rng.uniform(0.1, 0.2, groups)

    def move(y):
        return (y + rng.uniform(-1e-4, 1e-4, y.shape).astype(np.float32)).astype(np.float32)
    return move(_groups(x, p)), move(_groups(x, q))


def class_sized_in_range(seed, groups, p, q):
    """what a converged decoder hands the NMS: the reference's class sizes, centres over the +-55 m nuScenes range, copies
    jittered by 10^U(-7, -2) relative"""
    rng = np.random.default_rng(seed)
    x = _base(rng, groups, span=55.0)
    x[:, 2:4] = CLASS_SIZES[rng.integers(0, len(CLASS_SIZES), groups)] * rng.uniform(0.9, 1.1, (groups, 2)).astype(np.float32)
    return (_jitter(rng, _groups(x, p), 10.0 ** rng.uniform(-7, -2, groups * p)),
            _jitter(rng, _groups(x, q), 10.0 ** rng.uniform(-7, -2, groups * q)))


def wide_yaw(seed, groups, p, q):
    """ground-truth yaw after augmentation is not wrapped: yaw over +-7 rad, the copy a multiple of pi away from it (an odd one:
    the opposite heading, the same rectangle) where that stays inside +-7, jittered by 1e-5"""
    rng = np.random.default_rng(seed)
    x = _base(rng, groups)
    x[:, 4] = rng.uniform(-7, 7, groups)
    a, b = _jitter(rng, _groups(x, p), 1e-5), _jitter(rng, _groups(x, q), 1e-5)
    turned = b[:, 4] + (rng.integers(-4, 5, groups * q) * np.pi).astype(np.float32)
    b[:, 4] = np.where(np.abs(turned) <= 7, turned, b[:, 4])
    return a, b.astype(np.float32)


def touching(seed, groups, p, q):
    """boxes that share a stretch of an edge or one corner and nothing else (IoU 0): coordinates on a 1/8 m lattice, yaw 0 on
    both, so the contact is exact in float32; then the same pairs turned together by a random yaw about a's centre, where the
    contact holds to rounding"""
    rng = np.random.default_rng(seed)
    k = groups
    a = np.concatenate([rng.integers(-320, 321, (k, 2)) / 8.0, rng.integers(4, 41, (k, 2)) / 4.0, np.zeros((k, 1))], axis=1)
    A, B = _groups(a, p), _groups(a, q)
    n = groups * q
    wb, hb = rng.integers(4, 41, n) / 4.0, rng.integers(4, 41, n) / 4.0
    sx, sy = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    corner = rng.random(n) < 0.3
    along = rng.random(n) < 0.5                                      # edge contact: along x (above / below) or along y
    slide = rng.integers(-3, 4, n) / 8.0
    offx, offy = (B[:, 2] + wb) / 2, (B[:, 3] + hb) / 2
    cx = np.where(corner | ~along, B[:, 0] + sx * offx, B[:, 0] + slide)
    cy = np.where(corner | along, B[:, 1] + sy * offy, B[:, 1] + slide)
    b = np.stack([cx, cy, wb, hb, np.zeros(n)], axis=1)
    # second half of the groups: both boxes turned by the group's yaw about a's centre
    yaw = np.where(np.arange(k) >= k // 2, rng.uniform(-np.pi, np.pi, k), 0.0)
    ya, yb = _groups(yaw, p), _groups(yaw, q)
    d = b[:, :2] - B[:, :2]
    b[:, 0] = B[:, 0] + np.cos(yb) * d[:, 0] - np.sin(yb) * d[:, 1]
    b[:, 1] = B[:, 1] + np.sin(yb) * d[:, 0] + np.cos(yb) * d[:, 1]
    b[:, 4] = yb
    A = A.copy()
    A[:, 4] = ya
    return A.astype(np.float32), b.astype(np.float32)


def zero_width(seed, groups, p, q):
    """one side of the pair (or both) has w = 0, h = 0 or w * h far below 1e-14, on top of a live box"""
    rng = np.random.default_rng(seed)
    x = _base(rng, groups)
    a, b = _groups(x, p).copy(), _groups(x, q).copy()
    for arr in (a, b):
        kind = rng.integers(0, 4, arr.shape[0])
        arr[kind == 0, 2] = 0.0
        arr[kind == 1, 3] = 0.0
        arr[kind == 2, 2:4] = 1e-8
    return a, b


def _nd(rel):
    def gen(seed, groups, p, q):
        return near_duplicate(seed, groups, p, q, rel=rel)
    gen.__name__ = f"near_duplicate_{rel:g}"
    return gen


PAIR_GENERATORS = {g.__name__: g for g in (
    random_overlapping, identical, _nd(1e-7), _nd(1e-6), _nd(1e-5), _nd(1e-4), _nd(1e-3), _nd(1e-2), near_duplicate_far, yaw_plus_pi,
    swapped_axes, grid_aligned, nested_corner, thin_near_duplicate, class_sized_in_range, wide_yaw, touching, zero_width)}


def _spread_centres(rng, k, span, min_dist):
    """k centres in [-span, span]^2, no two closer than min_dist (rejection sampling)"""
    out = np.zeros((0, 2))
    while out.shape[0] < k:
        c = rng.uniform(-span, span, 2)
        if out.shape[0] == 0 or np.min(np.hypot(*(out - c).T)) >= min_dist:
            out = np.vstack([out, c])
    return out


def clustered_scene(seed, objects=50, copies=18):
    """What five decoder stages leave: `objects` car-sized objects that do not overlap one another, each proposed `copies` times
    with a relative jitter of 10^U(-7, -2), every sixth copy with the opposite heading; random scores.
    Returns boxes (n, 5) float32, scores (n,) float32, object id (n,)."""
    rng = np.random.default_rng(seed)
    c = _spread_centres(rng, objects, 50.0, 8.0)  # the longest diagonal is 5.6 m
    obj = np.concatenate([c, rng.uniform(1.5, 2.5, (objects, 1)), rng.uniform(3.5, 5.0, (objects, 1)),
                          rng.uniform(-np.pi, np.pi, (objects, 1))], axis=1).astype(np.float32)
    n = objects * copies
    boxes = _jitter(rng, _groups(obj, copies), 10.0 ** rng.uniform(-7, -2, n))
    flip = (np.arange(n) % copies) % 6 == 5
    boxes[flip, 4] += PI32
    return boxes, rng.uniform(0, 1, n).astype(np.float32), np.repeat(np.arange(objects), copies)


def mixed_scene(seed, n):
    """n boxes: clusters of 2-6 near-duplicates (jitter 10^U(-7, -2)) and loners that overlap their neighbours here and there,
    over an area that grows with n; random scores."""
    rng = np.random.default_rng(seed)
    span = max(4.0, 2.2 * np.sqrt(n))
    out = []
    while sum(x.shape[0] for x in out) < n:
        x = _base(rng, 1, span=span)
        x[:, 2:4] = [rng.uniform(1.5, 2.5), rng.uniform(3.5, 5.0)]
        k = int(rng.integers(2, 7)) if rng.random() < 0.4 else 1
        out.append(_jitter(rng, _groups(x, k), 10.0 ** rng.uniform(-7, -2, k)) if k > 1 else x)
    boxes = np.concatenate(out)[:n].astype(np.float32)
    boxes = boxes[rng.permutation(n)]
    return boxes, rng.uniform(0, 1, n).astype(np.float32)
