"""Float64 definition of multi-scale deformable attention (include/srfdet3d.h, `srf_msda_fwd`), as explicit loops over
(query, head, level, point, corner), and the planted inputs the GPU test shares with its CPU condition check.

    a[q,h,:,:]  = softmax over the L P logits of (q, h)                      (max-subtracted)
    px = ref_x W_l + dx - 0.5,  py = ref_y H_l + dy - 0.5                    (align_corners=False)
    out[q,h,:]  = sum_{l,p} a[q,h,l,p] * bilinear_zero_pad(value_l[b, ., ., h, :], py, px)

A corner outside the map contributes 0; a sample whose position is not inside (-1, H_l) x (-1, W_l) contributes 0 (the comparisons are
false for NaN and +-inf).  Besides the output the function returns what an error bound needs:
    D[q,h,:] = sum a w |v|                       every product of the sum, in magnitude
    A[q,h,:] = sum a (|v| summed over the four corners)      what a perturbed POSITION can move (|dw / dposition| <= 1 per corner)
    pmax     = max |px|, max |py| over the samples counted
A and pmax also count samples that lie within `slack` (a float32 rounding of the position) outside the open box: a float32 evaluation may
see them inside, where they contribute at most slack * |v|."""
import numpy as np

U32 = 2.0 ** -24


def softmax64(x):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - np.max(x))
        return e / e.sum()


def msda_ref(value, shapes, ref, offs, logits, heads, points):
    """value (B S, heads d), shapes [(H, W)], ref (B Q, L, 2), offs (B Q, heads, L, P, 2), logits (B Q, heads, L, P): any float arrays.
    -> dict(out, D, A: (B Q, heads d) float64; px_max, py_max: float)."""
    value = np.asarray(value, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    L, P = len(shapes), int(points)
    S = sum(h * w for h, w in shapes)
    rows = ref.shape[0]
    B = value.shape[0] // S
    Q = rows // B
    d = value.shape[1] // heads
    offs = np.asarray(offs, dtype=np.float64).reshape(rows, heads, L, P, 2)
    logits = np.asarray(logits, dtype=np.float64).reshape(rows, heads, L * P)
    starts = np.concatenate(([0], np.cumsum([h * w for h, w in shapes])[:-1]))
    out = np.zeros((rows, heads, d))
    Dm = np.zeros((rows, heads, d))
    Am = np.zeros((rows, heads, d))
    px_max = py_max = 0.0
    for r in range(rows):
        b = r // Q
        for h in range(heads):
            a = softmax64(logits[r, h])
            cs = slice(h * d, (h + 1) * d)
            for l, (H, W) in enumerate(shapes):
                base = b * S + starts[l]
                for p in range(P):
                    w_a = a[l * P + p]
                    dx, dy = offs[r, h, l, p]
                    with np.errstate(invalid="ignore", over="ignore"):
                        px = ref[r, l, 0] * W + dx - 0.5
                        py = ref[r, l, 1] * H + dy - 0.5
                    inside = py > -1 and py < H and px > -1 and px < W
                    slack = 8 * U32 * (abs(px) + abs(py) + 1) if np.isfinite(px) and np.isfinite(py) else 0.0
                    near = py > -1 - slack and py < H + slack and px > -1 - slack and px < W + slack
                    if not inside:
                        out[r, h] += w_a * 0.0          # 0 for a finite weight, NaN for a NaN one
                    if not near:
                        continue
                    px_max, py_max = max(px_max, abs(px)), max(py_max, abs(py))
                    x0, y0 = int(np.floor(px)), int(np.floor(py))
                    lx, ly = px - x0, py - y0
                    # A: the four corners; a position within `slack` of an integer also counts the corners of the cell next door
                    cols = sorted({int(np.floor(px - slack)), int(np.floor(px - slack)) + 1, int(np.floor(px + slack)), int(np.floor(px + slack)) + 1})
                    rws = sorted({int(np.floor(py - slack)), int(np.floor(py - slack)) + 1, int(np.floor(py + slack)), int(np.floor(py + slack)) + 1})
                    for yy in rws:
                        for xx in cols:
                            if 0 <= yy < H and 0 <= xx < W:
                                Am[r, h] += w_a * np.abs(value[base + yy * W + xx, cs])
                    if not inside:
                        continue
                    for yy, xx, wc in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)),
                                       (y0 + 1, x0 + 1, ly * lx)):
                        if yy < 0 or yy >= H or xx < 0 or xx >= W:
                            continue
                        v = value[base + yy * W + xx, cs]
                        out[r, h] += w_a * wc * v
                        Dm[r, h] += w_a * wc * np.abs(v)
    return dict(out=out.reshape(rows, heads * d), D=Dm.reshape(rows, heads * d), A=Am.reshape(rows, heads * d), px_max=px_max,
                py_max=py_max)


# ---- planted inputs ------------------------------------------------------------------------------------------------------------------
PYRAMID = [(16, 12), (8, 6), (4, 3), (2, 1)]


def make_case(heads, d, shapes, B, Q, P, seed):
    """float32 inputs: random queries, then the planted ones of the issue written over the first rows (as many as fit).  Returns
    dict(value (B S, C), ref (B Q, L, 2), offs (B Q, heads, L, P, 2), logits (B Q, heads, L, P)) as float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    rows = B * Q
    value = rng.standard_normal((B * S, heads * d)).astype(np.float32)
    ref = rng.uniform(0.0, 1.0, (rows, L, 2)).astype(np.float32)
    offs = (rng.standard_normal((rows, heads, L, P, 2)) * 2.0).astype(np.float32)
    logits = rng.standard_normal((rows, heads, L, P)).astype(np.float32)
    Hs = np.array([h for h, _ in shapes], dtype=np.float32)
    Ws = np.array([w for _, w in shapes], dtype=np.float32)

    def at(r, px, py):
        """row r: every sample of level l at pixel position (px[l], py[l]) exactly: ref = 0.5 / size (exact products for the power-of-two
        and small sizes used here are not needed: the offset is set to position + 0.5 - float32(ref * size), computed in float32)."""
        ref[r, :, 0], ref[r, :, 1] = 0.5, 0.5
        bx = (ref[r, :, 0] * Ws).astype(np.float32)
        by = (ref[r, :, 1] * Hs).astype(np.float32)
        offs[r, :, :, :, 0] = (np.asarray(px, dtype=np.float32) + np.float32(0.5) - bx)[None, :, None]
        offs[r, :, :, :, 1] = (np.asarray(py, dtype=np.float32) + np.float32(0.5) - by)[None, :, None]

    plants = []
    plants.append(lambda r: offs.__setitem__((r,), 0.0))                                        # zero offsets
    plants.append(lambda r: at(r, np.minimum(1, Ws - 1), np.minimum(1, Hs - 1)))                # integer positions
    for sx, sy in ((-1.0, 0.0), (0.0, -1.0), (-1.0, -1.0), (-0.5, 0.0), (0.0, -0.5), (-0.5, -0.5)):
        plants.append(lambda r, sx=sx, sy=sy: at(r, np.full(L, sx), np.full(L, sy)))            # low edges and the low corner
    for kx, ky in ((1, 0), (0, 1), (1, 1)):
        plants.append(lambda r, kx=kx, ky=ky: at(r, Ws * kx, Hs * ky))                          # exactly W_l / H_l
        plants.append(lambda r, kx=kx, ky=ky: at(r, (Ws - 0.5) * kx, (Hs - 0.5) * ky))          # W_l - 0.5 / H_l - 0.5
    plants.append(lambda r: at(r, np.full(L, -0.5), Hs - 0.5))                                  # mixed corners
    plants.append(lambda r: at(r, Ws - 0.5, np.full(L, -0.5)))
    plants.append(lambda r: at(r, Ws + 3.0, np.zeros(L)))                                       # fully outside on one axis only
    plants.append(lambda r: at(r, np.zeros(L), -4.0 * np.ones(L)))
    plants.append(lambda r: offs.__setitem__((r, slice(None), slice(None), 0, 0), 1e30))        # huge, infinite and NaN offsets
    plants.append(lambda r: offs.__setitem__((r, slice(None), slice(None), 0, 1), np.inf))
    plants.append(lambda r: offs.__setitem__((r, slice(None), slice(None), 0, 0), -np.inf))
    plants.append(lambda r: offs.__setitem__((r, slice(None), slice(None), 0, 1), np.nan))
    plants.append(lambda r: logits.__setitem__((r,), 0.25))                                     # all-equal logits
    plants.append(lambda r: logits.__setitem__((r, slice(None), 0, 0), logits[r, :, 0, 0] + 1e4))   # spread by 1e4
    plants.append(lambda r: logits.__setitem__((r, slice(None), L - 1, P - 1), -1e4))
    plants.append(lambda r: logits.__setitem__((r, 0, 0, 0), -np.inf))                          # one logit of -inf
    for r, plant in enumerate(plants[:rows]):
        plant(r)
    return dict(value=value, ref=ref, offs=offs, logits=logits)
