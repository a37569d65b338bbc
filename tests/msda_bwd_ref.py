"""Float64 definition of the gradient of multi-scale deformable attention (include/srfdet3d.h, `srf_msda_bwd`), as explicit loops over
(head, level, point, corner) on whole columns of queries, and the cases the GPU test shares with its CPU condition check.

With g = grad_out[q,h,:], a the softmax, px, py the forward's position, (x0, y0) its floor, lx = px - x0, ly = py - y0 and the corners
v00, v01, v10, v11 (zero outside the map):

    t[l,p]            = <g, (1-ly)(1-lx) v00 + (1-ly) lx v01 + ly (1-lx) v10 + ly lx v11>
    grad_logits[l,p]  = a[l,p] (t[l,p] - sum_j a[j] t[j])
    grad_offs[l,p].x  = a[l,p] <g, (1-ly)(v01 - v00) + ly (v11 - v10)>
    grad_offs[l,p].y  = a[l,p] <g, (1-lx)(v10 - v00) + lx (v11 - v01)>
    grad_value[corner] += a[l,p] w_corner g

A sample whose position is not inside (-1, H_l) x (-1, W_l) (NaN, +-inf included) has t = 0, a zero offset gradient and adds nothing; a
position on an integer takes its floor cell.  Besides the gradients the function returns what an error bound needs (all >= 0):

    Mv, Av, Nv  per grad_value element: sum |a w g| of its adds; sum a |g| over every add a float32 evaluation might make (below); their count
    Mo, Ao      per grad_offs element: a sum_c |g| ((1-ly)(|v01| + |v00|) + ly (|v11| + |v10|)) (x; y alike); a sum_c |g| (|v| over the corners)
    Ml, Al      per grad_logits element: a (Mt + sum_j a[j] Mt[j]) with Mt = sum_c |g| sum w |v|; the same with At = sum_c |g| (|v| over corners)
    px_max, py_max   max |px|, |py| over the samples counted
    kink        (B Q, heads, L, P) bool: the float64 position lies within 8 u (|px| + |py| + 1) of an integer (the box edges -1, W, H are
                integers) without being on it: a float32 evaluation may take the neighbouring cell or the other side of the edge, and
                the offset gradient, which is not continuous there, legitimately jumps.
    counted     number of samples with a position within that slack of the open box
    on_grid     (B Q, heads, L, P) bool: px or py exactly an integer (where grid_sample's backward takes another one-sided derivative)
Av, Nv, At also count, for a sample within the slack of an integer or of the box, the corners of the cell next door: t and the adds are
continuous in the position, so there a float32 evaluation is off by at most slack * |v| per corner.

`fault` plants one wrong implementation, for the check that the bound would show it: "corners" (v01 and v10 swapped), "sign" (grad_offs.x
negated), "start" (levels after the first start one row early), "softmax" (the - sum_j a[j] t[j] term dropped)."""
import numpy as np

from msda_ref import PYRAMID, make_case, softmax64

U32 = 2.0 ** -24

# name: (heads, d, shapes, B, Q (None: S), P, value pitch, grad_out pitch, offsets and logits (and their gradients) as views of one buffer)
# The six shapes of tests/test_gpu_msda.py; the L = 1, P = 1 map at Q = 24: at Q = 35 the planted single logit of -inf makes that row's
# softmax NaN, with 24 rows every reference gradient is finite.
CASES = {
    "d16_pyramid": (8, 16, PYRAMID, 2, None, 4, 128, 128, True),
    "d32_pyramid_pitched": (8, 32, PYRAMID, 2, None, 4, 320, 264, False),
    "d16_one_map_p1": (8, 16, [(5, 7)], 1, 24, 1, 132, 128, True),
    "d32_one_map_q3": (8, 32, [(5, 7)], 2, 3, 4, 256, 256, False),
    "d16_pyramid_p1_q3": (8, 16, PYRAMID, 1, 3, 1, 128, 140, False),
    "d16_two_levels_p3": (8, 16, [(4, 3), (2, 1)], 1, 40, 3, 128, 128, True),
}
_REF = {}


def case_inputs(name):
    """The float32 inputs of a case: `make_case` of tests/msda_ref.py plus a deterministic random grad_out (B Q, heads d)."""
    heads, d, shapes, B, Q, P, _, _, _ = CASES[name]
    S = sum(h * w for h, w in shapes)
    Q = S if Q is None else Q
    seed = sorted(CASES).index(name) + 11
    case = make_case(heads, d, shapes, B, Q, P, seed=seed)
    case["grad_out"] = np.random.default_rng(seed + 1000).standard_normal((B * Q, heads * d)).astype(np.float32)
    return case


def reference(name):
    """(inputs, float64 reference) of a case, computed once and left unchanged."""
    if name not in _REF:
        heads, _, shapes, _, _, P, _, _, _ = CASES[name]
        case = case_inputs(name)
        _REF[name] = (case, msda_bwd_ref(case["value"], shapes, case["ref"], case["offs"], case["logits"], heads, P, case["grad_out"]))
    return _REF[name]


def msda_bwd_ref(value, shapes, ref, offs, logits, heads, points, grad_out, fault=None):
    """value (B S, heads d), shapes [(H, W)], ref (B Q, L, 2), offs (B Q, heads, L, P, 2), logits (B Q, heads, L, P), grad_out
    (B Q, heads d): any float arrays -> dict (see the module text)."""
    value = np.asarray(value, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    gout = np.asarray(grad_out, dtype=np.float64)
    L, P = len(shapes), int(points)
    S = sum(h * w for h, w in shapes)
    rows = ref.shape[0]
    B = value.shape[0] // S
    Q = rows // B
    d = value.shape[1] // heads
    offs = np.asarray(offs, dtype=np.float64).reshape(rows, heads, L, P, 2)
    logits = np.asarray(logits, dtype=np.float64).reshape(rows, heads, L * P)
    starts = np.concatenate(([0], np.cumsum([h * w for h, w in shapes])[:-1]))
    if fault == "start":
        starts = starts - (np.arange(L) > 0)
    a = np.zeros((rows, heads, L * P))
    for r in range(rows):
        for h in range(heads):
            a[r, h] = softmax64(logits[r, h])
    batch = np.arange(rows) // Q
    gv, Mv, Av = (np.zeros_like(value) for _ in range(3))
    Nv = np.zeros(value.shape, dtype=np.int64)
    go, Mo, Ao = (np.zeros((rows, heads, L, P, 2)) for _ in range(3))
    t, Mt, At = (np.zeros((rows, heads, L * P)) for _ in range(3))
    kink = np.zeros((rows, heads, L, P), dtype=bool)
    on_grid = np.zeros((rows, heads, L, P), dtype=bool)
    px_max = py_max = 0.0
    counted = 0
    for h in range(heads):
        cs = np.arange(h * d, (h + 1) * d)
        g = gout[:, cs]
        for l, (H, W) in enumerate(shapes):
            base = batch * S + starts[l]
            for p in range(P):
                j = l * P + p
                w_a = a[:, h, j]
                with np.errstate(invalid="ignore", over="ignore"):
                    px = ref[:, l, 0] * W + offs[:, h, l, p, 0] - 0.5
                    py = ref[:, l, 1] * H + offs[:, h, l, p, 1] - 0.5
                    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
                    finite = np.isfinite(px) & np.isfinite(py)
                fx, fy = np.where(finite, px, 0.0), np.where(finite, py, 0.0)
                slack = 8 * U32 * (np.abs(fx) + np.abs(fy) + 1)
                near = finite & (fy > -1 - slack) & (fy < H + slack) & (fx > -1 - slack) & (fx < W + slack)
                counted += int(near.sum())
                if near.any():
                    px_max, py_max = max(px_max, np.abs(fx[near]).max()), max(py_max, np.abs(fy[near]).max())
                ddx, ddy = np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy))
                kink[:, h, l, p] = near & (((ddx > 0) & (ddx <= slack)) | ((ddy > 0) & (ddy <= slack)))
                on_grid[:, h, l, p] = near & ((ddx == 0) | (ddy == 0))
                # what a float32 evaluation might touch: the corners of every cell within the slack of the position
                nx, ny, ns = np.where(near, fx, 0.0), np.where(near, fy, 0.0), np.where(near, slack, 0.0)
                xs = [np.floor(nx - ns), np.floor(nx - ns) + 1, np.floor(nx + ns), np.floor(nx + ns) + 1]
                ys = [np.floor(ny - ns), np.floor(ny - ns) + 1, np.floor(ny + ns), np.floor(ny + ns) + 1]
                for iy, yy in enumerate(ys):
                    new_y = np.ones(rows, dtype=bool)
                    for k in range(iy):
                        new_y &= ys[k] != yy
                    for ix, xx in enumerate(xs):
                        new_x = np.ones(rows, dtype=bool)
                        for k in range(ix):
                            new_x &= xs[k] != xx
                        ok = near & new_y & new_x & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                        if not ok.any():
                            continue
                        vrow = (base + yy * W + xx).astype(np.int64)[ok]
                        At[ok, h, j] += (np.abs(g[ok]) * np.abs(value[vrow[:, None], cs])).sum(-1)
                        np.add.at(Av, (vrow[:, None], cs[None, :]), w_a[ok, None] * np.abs(g[ok]))
                        np.add.at(Nv, (vrow[:, None], cs[None, :]), 1)
                # the definition
                x0, y0 = np.floor(np.where(inside, px, 0.0)), np.floor(np.where(inside, py, 0.0))
                lx, ly = np.where(inside, px, 0.0) - x0, np.where(inside, py, 0.0) - y0
                v, wc = [], [(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx]
                for q, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    yy, xx = y0 + oy, x0 + ox
                    ok = inside & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                    vrow = np.where(ok, base + yy * W + xx, 0).astype(np.int64)
                    v.append(np.where(ok[:, None], value[vrow[:, None], cs], 0.0))
                    if ok.any():
                        term = (w_a * wc[q])[ok, None] * g[ok]
                        np.add.at(gv, (vrow[ok][:, None], cs[None, :]), term)
                        np.add.at(Mv, (vrow[ok][:, None], cs[None, :]), np.abs(term))
                if fault == "corners":
                    v[1], v[2] = v[2], v[1]
                ag = np.abs(g)
                t[:, h, j] = (g * sum(wc[q][:, None] * v[q] for q in range(4))).sum(-1)
                Mt[:, h, j] = (ag * sum(wc[q][:, None] * np.abs(v[q]) for q in range(4))).sum(-1)
                hx, hy = (1 - lx)[:, None], (1 - ly)[:, None]
                go[:, h, l, p, 0] = w_a * (g * (hy * (v[1] - v[0]) + ly[:, None] * (v[3] - v[2]))).sum(-1) * (-1 if fault == "sign" else 1)
                go[:, h, l, p, 1] = w_a * (g * (hx * (v[2] - v[0]) + lx[:, None] * (v[3] - v[1]))).sum(-1)
                Mo[:, h, l, p, 0] = w_a * (ag * (hy * (np.abs(v[1]) + np.abs(v[0])) + ly[:, None] * (np.abs(v[3]) + np.abs(v[2])))).sum(-1)
                Mo[:, h, l, p, 1] = w_a * (ag * (hx * (np.abs(v[2]) + np.abs(v[0])) + lx[:, None] * (np.abs(v[3]) + np.abs(v[1])))).sum(-1)
                Ao[:, h, l, p, :] = (w_a * (ag * sum(np.abs(v[q]) for q in range(4))).sum(-1))[:, None]
    dot = (a * t).sum(-1, keepdims=True) * (0 if fault == "softmax" else 1)
    gl = a * (t - dot)
    Ml = a * (Mt + (a * Mt).sum(-1, keepdims=True))
    Al = a * (At + (a * At).sum(-1, keepdims=True))
    return dict(grad_value=gv, grad_offs=go.reshape(rows, -1), grad_logits=gl.reshape(rows, -1), Mv=Mv, Av=Av, Nv=Nv, Mo=Mo.reshape(rows, -1),
                Ao=Ao.reshape(rows, -1), Ml=Ml.reshape(rows, -1), Al=Al.reshape(rows, -1), px_max=float(px_max), py_max=float(py_max),
                kink=kink, on_grid=on_grid, counted=counted)


def logit_spread(logits, heads):
    """T of the bound: the largest |l - max| of a (row, head) among the logits whose float32 weight is not flushed (|l - max| <= 104)."""
    lg = np.asarray(logits, dtype=np.float64).reshape(logits.shape[0], heads, -1)
    with np.errstate(invalid="ignore"):
        t = np.abs(lg - lg.max(-1, keepdims=True))
    return float(np.nanmax(np.where(t <= 104, t, 0.0)))


def bounds(name):
    """The GPU test's bound per element of the three gradients, from the reference alone (derivation: tests/test_gpu_msda_bwd.py).
    -> dict(grad_value, grad_offs, grad_logits: arrays; T)."""
    case, ref = reference(name)
    heads = CASES[name][0]
    T = logit_spread(case["logits"], heads)

    def gamma(k):
        return k * U32 / (1 - k * U32)

    pos = 6 * U32 * (ref["px_max"] + ref["py_max"] + 1)
    return dict(grad_value=gamma(2 * T + 25 + ref["Nv"]) * ref["Mv"] + (pos + 1e-30) * ref["Av"],
                grad_offs=gamma(2 * T + 31) * ref["Mo"] + (pos + 1e-30) * ref["Ao"],
                grad_logits=gamma(4 * T + 71) * ref["Ml"] + (pos + 1e-30) * ref["Al"], T=T)
