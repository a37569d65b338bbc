"""Float64 definitions of the decoder-stage kernels of csrc/decoder.hip as include/srfdet3d.h words them -- `srf_linear`'s chain,
`srf_self_attention(_batched)`, `srf_dynconv_mid`, `srf_stage_tail`, `srf_apply_deltas`, `srf_dpg_mix` -- with the magnitude sums an error
bound needs, the first-order error of a LayerNorm step, the planted inputs the GPU tests share with their CPU condition checks, and
`call_linear` / `call_stage_tail`, which reach the arguments of the raw entry points that the `ops` wrappers fix (any legal pitch, the
caller's outputs and workspace, each LayerNorm's own eps).

    chain(v) = [LayerNorm(ln1, eps1)] -> [ReLU if relu1] -> [+ residual] -> [LayerNorm(ln2, eps2)] -> [ReLU if relu2],  v = x w^T + bias
    LayerNorm(v)_i = g_i (v_i - mean v) / sqrt(var v + eps) + b_i,  var = the biased variance of the row

Every reference takes `mutate`: a named, deliberate defect (a dropped K chunk, the unbiased variance, a swapped head, ...) that the CPU
checks of tests/test_decoder_ref.py use to prove that the bound of a case is tight enough to show that defect."""
import numpy as np

U32 = 2.0 ** -24


def gamma(k):
    return k * U32 / (1 - k * U32)


# --------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_ref(v, ln, unbiased=False):
    """v (M, N) float64, ln = (g, b, eps) -> dict(out, t = v - mean, s = sqrt(var + eps) (M, 1), rstd = 1 / s,
    z = t / s, g, v_abs_mean = mean |v| (M, 1))."""
    g, b, eps = np.asarray(ln[0], np.float64), np.asarray(ln[1], np.float64), float(ln[2])
    n = v.shape[1]
    t = v - v.mean(1, keepdims=True)
    var = (t * t).sum(1, keepdims=True) / ((n - 1) if unbiased and n > 1 else n)
    s = np.sqrt(var + eps)
    return dict(out=t / s * g + b, t=t, s=s, rstd=1.0 / s, z=t / s, g=g, v_abs_mean=np.abs(v).mean(1, keepdims=True))


def layernorm_bound(step, e_in, adds):
    """First-order bound on the error of a float32 LayerNorm step whose input row carries the elementwise error e_in (M, N).
    `step` is layernorm_ref's dict; `adds` is the number of additions on the longest path of the row sum (values per lane + shuffle
    steps).  With t = v - mean, s = sqrt(var + eps), n the row length:

      propagation   d mean <= mean(e);  d t_i <= e_i + mean(e);  d var = (2 / n) sum_j t_j dv_j (the mean's shift drops out: sum t = 0),
                    so d s <= sum_j |t_j| e_j / (n s);  d (t_i / s) <= (e_i + mean(e)) / s + (|t_i| / s) (sum_j |t_j| e_j / (n s)) / s.
                    Term by term this is at most (E / s) (2 + |t_i| / s) with E = max e: Cauchy-Schwarz, sum |t_j| <= n s.
      the step      mean: `adds` additions and the division by n                       d mean <= gamma(adds + 1) mean |v|
                    t_i = v_i - mean: one rounding                                      u |t_i|
                    var: t_i t_i (one rounding; the two roundings of t_i's own subtraction move it by 2 u), `adds` additions, / n, + eps;
                    sqrtf and 1 / x, two u each (one ulp)                               d rstd / rstd <= ((adds + 5) / 2 + 4) u
                    (t_i rstd) g_i + b_i: three roundings                               2 u |g_i t_i / s| + u |out_i|
    """
    t, s, g = np.abs(step["t"]), step["s"], np.abs(step["g"])
    n = t.shape[1]
    ds = (t * e_in).sum(1, keepdims=True) / (n * s)
    prop = (e_in + e_in.mean(1, keepdims=True)) / s + (t / s) * ds / s
    own = (gamma(adds + 1) * step["v_abs_mean"] + U32 * t) / s + (t / s) * (((adds + 5) / 2 + 4) * U32 + 2 * U32)
    return g * (prop + own) + U32 * np.abs(step["out"])


# ------------------------------------------------------------------------------------------------------------------ linear
def linear_ref(x, w, bias=None, ln1=None, relu1=False, residual=None, ln2=None, relu2=False, mutate=None):
    """x (M, K), w (N, K), bias (N), ln = (g, b, eps), residual (M, N): any float arrays -> dict
         out      (M, N) float64, the chain of the header
         mag      (M, N) sum_k |x| |w| + |bias|: every term of the product, in magnitude
         pre      (M, N) x w^T + bias
         ln1, ln2 layernorm_ref's dict of each LayerNorm that runs (rstd, the normalised values z, ...), else None
         res_in   (M, N) the value the residual is added to (or None)
    mutate: None | ("chunk", k0) drop x[:, k0:k0+32] from the product | ("slab", p) drop x[:, 256 p:256 (p + 1)] | "bias" skipped |
    "unbiased" variance | "eps" eps1 and eps2 swapped | "residual_first" the residual added before relu1 instead of after it."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    if isinstance(mutate, tuple):
        lo = mutate[1] if mutate[0] == "chunk" else 256 * mutate[1]
        x = x.copy()
        x[:, lo:lo + (32 if mutate[0] == "chunk" else 256)] = 0.0
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, np.float64)
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)
    pre = x @ w.T + (0.0 if mutate == "bias" else b)
    if mutate == "eps":
        e1, e2 = (ln2[2] if ln2 is not None else 1e-3), (ln1[2] if ln1 is not None else 1e-5)
        ln1 = None if ln1 is None else (ln1[0], ln1[1], e1)
        ln2 = None if ln2 is None else (ln2[0], ln2[1], e2)
    v = pre
    s1 = s2 = res_in = None
    if ln1 is not None:
        s1 = layernorm_ref(v, ln1, mutate == "unbiased")
        v = s1["out"]
    res = None if residual is None else np.asarray(residual, np.float64)
    if mutate == "residual_first" and res is not None:
        v = v + res
    if relu1:
        v = np.maximum(v, 0.0)
    if res is not None and mutate != "residual_first":
        res_in = v
        v = v + res
    if ln2 is not None:
        s2 = layernorm_ref(v, ln2, mutate == "unbiased")
        v = s2["out"]
    if relu2:
        v = np.maximum(v, 0.0)
    return dict(out=v, mag=mag, pre=pre, ln1=s1, ln2=s2, res_in=res_in, residual=res)


def call_linear(x, w, bias=None, ln1=None, relu1=False, residual=None, ln2=None, relu2=False, y=None, ws=None, ws_bytes=None):
    """`srf_linear` on torch *views*: ldx, ldw, ldr and ldy are whatever row strides x, w, residual and y have (inner stride 1), ln =
    (g, b, eps) tensors with each LayerNorm's own eps, y the caller's (M, N) view (a fresh tensor when None).  The workspace is
    `srf_linear_workspace_bytes` long and filled with NaN before the call unless the caller brings one.  -> (return code, y, ws)."""
    import torch
    from srfdet3d_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0]
    for t in (x, w, residual, y):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1)
    L = _lib.lib()
    if y is None:
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    if ws is None:
        need = L.srf_linear_workspace_bytes(M, N, K)
        ws = torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device=x.device)
        ws_bytes = need if ws_bytes is None else ws_bytes
    elif ws_bytes is None:
        ws_bytes = ws.numel() * ws.element_size()
    p = ops._ptr
    g1, b1, e1 = (None, None, 0.0) if ln1 is None else (p(ln1[0]), p(ln1[1]), float(ln1[2]))
    g2, b2, e2 = (None, None, 0.0) if ln2 is None else (p(ln2[0]), p(ln2[1]), float(ln2[2]))
    rc = L.srf_linear(p(x), M, K, x.stride(0), p(w), N, w.stride(0), p(bias), g1, b1, e1, int(bool(relu1)), p(residual),
                      residual.stride(0) if residual is not None else 0, g2, b2, e2, int(bool(relu2)), p(y), y.stride(0), p(ws), ws_bytes,
                      ops._stream())
    return rc, y, ws


def coherent(rng, rows, cols, row_scale=None):
    """(rows, cols) float32 whose entries share their row's sign and size: a[r] (1 + 0.5 noise).  A product of two such matrices has
    sum |x| |w| of the size of |sum x w|, so a rounding bound gamma_K sum |x| |w| stays a small fraction of the result itself (with
    zero-mean operands the sum of magnitudes is sqrt(K) times the result and a K-long float32 chain cannot be held to 1e-3 of it)."""
    a = rng.standard_normal(rows) if row_scale is None else row_scale
    return (a[:, None] * (1.0 + 0.5 * rng.standard_normal((rows, cols)))).astype(np.float32)


def linear_inputs(M, K, N, chain, seed, integers):
    """The planted operands of one srf_linear case.  integers: x in [-3, 3], w in [-2, 2], integer bias and residual -- every partial
    sum an integer far below 2^24.  Else x[m] = c_m (1 + 0.5 noise) with 0.5 <= |c_m| <= 1.5, w[n] = a_n (1 + 0.5 noise) / K with a ~ N(0, 1):
    x w^T ~ c_m a_n, row variances of order 1.  LayerNorm gains in [0.75, 1.25], eps1 = 1e-5, eps2 = 1e-3."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    if integers:
        x = rng.integers(-3, 4, (M, K)).astype(f32)
        w = rng.integers(-2, 3, (N, K)).astype(f32)
        bias = rng.integers(-5, 6, N).astype(f32)
        res = rng.integers(-9, 10, (M, N)).astype(f32)
    else:
        c = rng.uniform(0.5, 1.5, M) * rng.choice([-1.0, 1.0], M)
        x = coherent(rng, M, K, c)
        w = (coherent(rng, N, K) / K).astype(f32)
        bias = (0.5 * rng.standard_normal(N)).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32)
    ln = lambda eps: ((0.75 + 0.5 * rng.random(N)).astype(f32), (0.1 * rng.standard_normal(N)).astype(f32), eps)
    ln1, ln2 = ln(1e-5), ln(1e-3)
    kw = dict(bias=bias if "bias" in chain else None, ln1=ln1 if "ln1" in chain else None, relu1="relu1" in chain,
              residual=res if "res" in chain else None, ln2=ln2 if "ln2" in chain else None, relu2="relu2" in chain)
    return x, w, kw


# --------------------------------------------------------------------------------------------------------------- attention
def attention_ref(qkv, B, P, E, H, mutate=None):
    """qkv (B P, 3 E) rows [q | k | v], sample-major -> dict
         out   (B P, E) float64: softmax(q_h k_h^T / sqrt(d)) v_h per head among the P rows of each sample, d = E / H
         D     (B P, E) sum_j a_j |v_j|
         T     (B P, H) largest |s - max s| of the row
         S     (B P, H) largest sum_i |q_i| |k_i| / sqrt(d) over the row's keys
    mutate: None | "last_key" dropped | "first_twice" (the first key of the last 128-key tile counted twice) | "scale" (1 / sqrt(2 d)) |
    "heads" (the outputs of heads 0 and 1 swapped)."""
    qkv = np.asarray(qkv, np.float64).reshape(B, P, 3, H, E // H)
    d = E // H
    scale = 1.0 / np.sqrt(2 * d if mutate == "scale" else d)
    out, Dm = np.zeros((B, P, H, d)), np.zeros((B, P, H, d))
    T, S = np.zeros((B, P, H)), np.zeros((B, P, H))
    for b in range(B):
        for h in range(H):
            q, k, v = qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h]
            if mutate == "last_key":
                k, v = k[:-1], v[:-1]
            if mutate == "first_twice":
                j = (P - 1) // 128 * 128
                k, v = np.concatenate((k, k[j:j + 1])), np.concatenate((v, v[j:j + 1]))
            s = q @ k.T * scale
            m = s.max(1, keepdims=True)
            a = np.exp(s - m)
            a /= a.sum(1, keepdims=True)
            out[b, :, h], Dm[b, :, h] = a @ v, a @ np.abs(v)
            T[b, :, h] = np.abs(s - m).max(1)
            S[b, :, h] = (np.abs(q) @ np.abs(k).T * scale).max(1)
    if mutate == "heads":
        out[:, :, [0, 1]] = out[:, :, [1, 0]]
    return dict(out=out.reshape(B * P, E), D=Dm.reshape(B * P, E), T=T.reshape(B * P, H), S=S.reshape(B * P, H))


def attention_inputs(B, P, E, H, wide, seed):
    """qkv (B P, 3 E) float32.  Unit scale: standard normal.  wide: in every (sample, head) the last key is planted along the query of
    row P // 2 (a late key that dominates that row: the running maximum moves at the very end), then q is scaled so that the widest row
    of the case has max |s - max s| = 60 (P = 1: nothing to spread)."""
    rng = np.random.default_rng(seed)
    d = E // H
    qkv = rng.standard_normal((B, P, 3, H, d))
    if wide and P > 1:
        r0 = P // 2
        qn = qkv[:, r0, 0] / np.linalg.norm(qkv[:, r0, 0], axis=-1, keepdims=True)
        qkv[:, P - 1, 1] = 3.0 * np.sqrt(d) * qn * (1.0 + 0.05 * rng.standard_normal((B, H, d)))
        s = np.einsum("bphd,bkhd->bhpk", qkv[:, :, 0], qkv[:, :, 1]) / np.sqrt(d)
        qkv[:, :, 0] *= 60.0 / (s.max(-1) - s.min(-1)).max()
    return qkv.reshape(B * P, 3 * E).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- DynamicConv
def dynconv_mid_ref(feats, params, ln1, ln2, mutate=None):
    """feats (R, S, C), params (R, 2 C D) = [W1 (C x D) | W2 (D x C)] per proposal, ln = (g, b, eps) ->
    relu(LN_C(relu(LN_D(feats W1)) W2)) (R, S, C) float64 with, per product, sum |a| |b| and, per LayerNorm, layernorm_ref's dict.
    mutate: None | "transposed" (W1 read as D x C and W2 as C x D, transposed) | "ln1_rows" (LayerNorm 1 skipped for rows >= 48: ReLU
    of the raw product) | "neighbour" (proposal r reads the weights of proposal r + 1, the last one those of the first)."""
    feats, params = np.asarray(feats, np.float64), np.asarray(params, np.float64)
    R, S, C = feats.shape
    D = params.shape[1] // (2 * C)
    if mutate == "neighbour":
        params = np.roll(params, -1, axis=0)
    w1, w2 = params[:, :C * D].reshape(R, C, D), params[:, C * D:].reshape(R, D, C)
    if mutate == "transposed":
        w1 = params[:, :C * D].reshape(R, D, C).transpose(0, 2, 1)
        w2 = params[:, C * D:].reshape(R, C, D).transpose(0, 2, 1)
    p1 = feats @ w1
    mag1 = np.abs(feats) @ np.abs(w1)
    s1 = layernorm_ref(p1.reshape(R * S, D), ln1)
    x1 = np.maximum(s1["out"], 0.0).reshape(R, S, D)
    if mutate == "ln1_rows":
        x1[:, 48:] = np.maximum(p1[:, 48:], 0.0)
    p2 = x1 @ w2
    mag2 = x1 @ np.abs(w2)
    s2 = layernorm_ref(p2.reshape(R * S, C), ln2)
    return dict(out=np.maximum(s2["out"], 0.0).reshape(R, S, C), mag1=mag1, mag2=mag2, ln1=s1, ln2=s2, x1=x1, w2_abs=np.abs(w2))


def dynconv_inputs(R, S, C, D, seed):
    """feats[r, s] = c (1 + 0.5 noise), W1[r][:, j] = a_j (1 + 0.5 noise) / C, W2[r][:, j] = a'_j (1 + 0.5 noise) * 2 / D (see `coherent`):
    both products have row variances of order 1.  -> feats (R, S, C), params (R, 2 C D), ln1 (D), ln2 (C) as float32."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    c = rng.uniform(0.5, 1.5, R * S) * rng.choice([-1.0, 1.0], R * S)
    feats = coherent(rng, R * S, C, c).reshape(R, S, C)
    w1 = np.stack([coherent(rng, D, C).T / C for _ in range(R)])                  # (R, C, D)
    w2 = np.stack([coherent(rng, C, D).T * 2.0 / D for _ in range(R)])            # (R, D, C)
    params = np.concatenate((w1.reshape(R, -1), w2.reshape(R, -1)), 1).astype(f32)
    ln = lambda n, eps: ((0.75 + 0.5 * rng.random(n)).astype(f32), (0.1 * rng.standard_normal(n)).astype(f32), eps)
    return feats.astype(f32), params, ln(D, 1e-5), ln(C, 1e-3)


# -------------------------------------------------------------------------------------------------------------- apply_deltas
GEOM = ((1.5, 2.0, 3.0, 0.5, 1.0, 4.0), (-54.0, -40.0, -5.0, 54.0, 62.4, 3.0), float(np.log(100000.0 / 16)))   # asymmetric on purpose
GEOM_SHIPPED = ((1.0,) * 6, (-54.0, -54.0, -5.0, 54.0, 54.0, 3.0), float(np.log(100000.0 / 16)))
AD_MUTATIONS = ("no_clamp", "no_clip", "weights_swapped", "axis", "row_shift")


def geom64(geom):
    """(weights6, lo, ext, clamp) in float64 of the float32 values the ABI receives; ext = hi - lo of those, not rounded again."""
    w = np.asarray(geom[0], np.float32).astype(np.float64)
    r = np.asarray(geom[1], np.float32).astype(np.float64)
    return w, r[:3], r[3:] - r[:3], float(np.float32(geom[2]))


def apply_deltas_ref(deltas, boxes, weights6, pc_range, clamp, mutate=None):
    """plugin/heads.py::apply_deltas_lidar in float64: deltas (R, Dd) on boxes (R, Dd) [centres in metres, log sizes, ...] ->
         out     (R, Dd): clip((d / w exp(b_size) + b_ctr - lo) / ext, 0, 1) | log(exp(min(d / w, clamp)) exp(b_size)) | the deltas from column 6
         qsize   (R, 3) |d / w| size      ctr (R, 3) |ctr|      ctr_lo (R, 3) |ctr - lo|      n (R, 3) |ctr - lo| / ext, before the clip
         ds      (R, 3) |d / w| of the size columns, before the clamp      size (R, 3), w (6), ext (3)
    mutate: None | "no_clamp" | "no_clip" | "weights_swapped" (w[3 + i] used for w[i] and back) | "axis" (x's lo and ext used for y) |
    "row_shift" (row r refined with the box of row r + 1, the last row with the first)."""
    d, b = np.asarray(deltas, np.float64), np.asarray(boxes, np.float64)
    w, lo, ext, clamp = geom64((weights6, pc_range, clamp))
    if mutate == "weights_swapped":
        w = np.concatenate((w[3:], w[:3]))
    if mutate == "axis":
        lo, ext = lo[[0, 0, 2]], ext[[0, 0, 2]]
    if mutate == "row_shift":
        b = np.roll(b, -1, axis=0)
    q = d[:, :6] / w
    size = np.exp(b[:, 3:6])
    ctr = q[:, :3] * size + b[:, :3]
    n = (ctr - lo) / ext
    ds = q[:, 3:]
    new = np.log(np.exp(ds if mutate == "no_clamp" else np.minimum(ds, clamp)) * size)
    out = np.concatenate((n if mutate == "no_clip" else np.clip(n, 0.0, 1.0), new, d[:, 6:]), 1)
    return dict(out=out, qsize=np.abs(q[:, :3]) * size, ctr=np.abs(ctr), ctr_lo=np.abs(ctr - lo), n=np.abs(n), ds=np.abs(ds), size=size,
                w=np.abs(w), ext=ext)


def planted_box_rows(geom):
    """Two (deltas[:6], boxes[:6]) rows that together carry every edge of the refinement; every planted delta is d = target * w with w a
    power of two wherever the target must be hit exactly (weights 0.5, 1, 4 or 1 of the size columns), every planted centre delta is 0:
      row A  sizes: ds = 0.9 clamp | ds == clamp | ds one float32 above clamp;   centres: on lo | on lo + ext | 3 m below lo;  log sizes -2, 2, 0.3
      row B  sizes: ds = -20 | ds = 50 (far above) | ds = 1;                     centres: 5 m above hi | inside | on lo;       log sizes 2, -2, -0.7"""
    f32 = np.float32
    w, r, c = np.asarray(geom[0], f32), np.asarray(geom[1], f32), f32(geom[2])
    above = np.nextafter(c, f32(np.inf))
    dA = np.array([0, 0, 0, f32(0.9) * c * w[3], c * w[4], above * w[5]], f32)
    bA = np.array([r[0], r[4], r[2] - f32(3), -2, 2, 0.3], f32)
    dB = np.array([0, 0, 0, f32(-20) * w[3], f32(50) * w[4], w[5]], f32)
    bB = np.array([r[3] + f32(5), 1.25, r[2], 2, -2, -0.7], f32)
    return (dA, bA), (dB, bB)


def apply_deltas_inputs(R, Dd, geom, seed):
    """deltas ~ N(0, 1), centres in metres across the range, log sizes in [-2, 2], the other columns N(0, 1); row R - 1 is planted row A
    and row R - 2 planted row B of `planted_box_rows` (R == 1: A for an even seed, B for an odd one).  -> deltas, boxes (R, Dd) float32."""
    rng = np.random.default_rng(seed)
    r = np.asarray(geom[1], np.float64)
    deltas = rng.standard_normal((R, Dd))
    boxes = np.concatenate((r[:3] + rng.random((R, 3)) * (r[3:] - r[:3]), rng.uniform(-2, 2, (R, 3)), rng.standard_normal((R, Dd - 6))), 1)
    deltas, boxes = deltas.astype(np.float32), boxes.astype(np.float32)
    A, B = planted_box_rows(geom)
    rows = [(R - 1, A), (R - 2, B)] if R >= 2 else [(0, A if seed % 2 == 0 else B)]
    for row, (d, b) in rows:
        deltas[row, :6], boxes[row, :6] = d, b
    return deltas, boxes


# ---------------------------------------------------------------------------------------------------------------- stage tail
TAIL_MUTATIONS = ("ffn_slice", "no_residual", "no_b2", "unbiased", "tower_ln", "eps_swapped", "tower_relu", "head_col",
                  "tail_row") + AD_MUTATIONS
EPS_N3, EPS_CLS, EPS_REG = 1e-3, 1e-2, 1e-5


def stage_tail_ref(params, boxes, geom, mutate=None):
    """The chain of `srf_stage_tail` in float64, from `linear_ref`, `layernorm_ref` and `apply_deltas_ref`:
         h = relu(obj W1^T + b1);  obj_out = LN3(h W2^T + b2 + obj);  a tower = layers of relu(LN(x W^T));
         logits = cls_tower(obj_out) Wl^T + bl;  deltas = reg_tower(obj_out) Wd^T + bd;  pred = apply_deltas(deltas, boxes)
    params: obj (R, 128), w1 (F, 128), b1, w2 (128, F), b2, n3 = (g, b, eps), cls / reg = [(W, g, b), ...], eps_cls / eps_reg (4 each: the
    ABI's arrays, of which a tower uses its first n), wl (ncls, 128), bl, wd (Dd, 128), bd.
    -> dict(obj_out, logits, deltas, pred, hid, ffn, cls, reg, head_cls, head_reg: linear_ref's dict of every step, ad: apply_deltas_ref's).
    mutate: "ffn_slice" hidden units 128..255 dropped | "no_residual" | "no_b2" | "unbiased" variance in norm3 | "tower_ln" cls layer 0
    normalised with reg layer 0's gamma / beta | "eps_swapped" eps_cls[l] <-> eps_reg[l] | "tower_relu" no ReLU after the last layer of a
    tower | "head_col" bl[c + 1] added to logits column c | "tail_row" the rows of the second 32-row tile shifted by one (row r shows
    row r + 1, the tile's last row its first) in every output | every mutation of apply_deltas_ref."""
    p = params
    obj = np.asarray(p["obj"], np.float64)
    hid = linear_ref(obj, p["w1"], p["b1"], relu1=True)
    h = hid["out"]
    if mutate == "ffn_slice":
        h = h.copy()
        h[:, 128:256] = 0.0
    ffn = linear_ref(h, p["w2"], p["b2"], residual=None if mutate == "no_residual" else obj, ln2=p["n3"],
                     mutate={"no_b2": "bias", "unbiased": "unbiased"}.get(mutate))
    eps_c, eps_r = (p["eps_reg"], p["eps_cls"]) if mutate == "eps_swapped" else (p["eps_cls"], p["eps_reg"])

    def tower(layers, eps, first_ln=None):
        x, steps = ffn["out"], []
        for l, (W, g, b) in enumerate(layers):
            if l == 0 and first_ln is not None:
                g, b = first_ln
            steps.append(linear_ref(x, W, None, ln1=(g, b, eps[l]), relu1=not (mutate == "tower_relu" and l == len(layers) - 1)))
            x = steps[-1]["out"]
        return x, steps

    swap = p["reg"][0][1:] if mutate == "tower_ln" and p["cls"] and p["reg"] else None
    cf, cls_steps = tower(p["cls"], eps_c, swap)
    rf, reg_steps = tower(p["reg"], eps_r)
    head_cls = linear_ref(cf, p["wl"], np.roll(p["bl"], -1) if mutate == "head_col" else p["bl"])
    head_reg = linear_ref(rf, p["wd"], p["bd"])
    ad = apply_deltas_ref(head_reg["out"], boxes, *geom, mutate=mutate if mutate in AD_MUTATIONS else None)
    out = dict(obj_out=ffn["out"], logits=head_cls["out"], deltas=head_reg["out"], pred=ad["out"])
    if mutate == "tail_row":
        for k in ("obj_out", "logits", "pred"):
            out[k] = out[k].copy()
            out[k][32:64] = np.roll(out[k][32:64], -1, axis=0)
    return dict(out, hid=hid, ffn=ffn, cls=cls_steps, reg=reg_steps, head_cls=head_cls, head_reg=head_reg, ad=ad)


def stage_tail_inputs(R, F, n_cls, n_reg, ncls, Dd, seed, geom=GEOM, beta=2.0, plant=None, fan=8):
    """The planted operands of one srf_stage_tail case -> (params of stage_tail_ref, boxes (R, Dd)), float32.
    Every product has `coherent` operands: obj[m] = c_m (1 + 0.5 noise) with 0.5 <= |c_m| <= 1.5, W1 = coherent / 128, W2 = coherent 2 / F,
    biases 0.5 noise.  Every LayerNorm has gamma in [0.75, 1.25] and beta = `beta` + 0.1 noise: the positive offset keeps the operand of
    each later product sign-coherent -- with beta around 0 the sum |x| |w| of a tower layer is about 18 times its result and the
    worst-case bound grows about five-fold per layer.  Tower and head weights are coherent too, but `fan` = 8 entries of a row out of
    128, scaled by 1 / fan: a dense coherent row is a_n (1 + 0.5 noise) / 128, its product with a positive x is a_n (mean x + 4 %), and
    the LayerNorm that follows removes mean x -- whatever tells two rows of x apart, or two gamma vectors of the layer before, shrinks
    about 45-fold per layer and is below the bound after two layers, so neither a shifted row nor a wrong LayerNorm vector in layer 0
    would show in a deep tower.  With 8 entries the row-specific part of a product is a quarter of it and survives four layers; the
    zeros leave sum |x| |w| = |sum x w| as it was.  eps: norm3 1e-3, every cls layer 1e-2, every reg layer 1e-5 (distinct, and large
    enough to tell apart).  Boxes: centres in metres across the range, log sizes in [-2, 2].
    plant (default: R >= 31): the fused kernel takes a delta only from its head, so an exact delta is reached per column, through bd and a
    zeroed head row: rows 1, 3, 4 and 5 of Wd are zero, bd[1] = 0 (ctr_y = the box's y exactly) and, in every row,
        seed even   bd[3] = 50 w3 (far above), bd[4] = clamp w4 (ds == clamp), bd[5] = (clamp + one float32) w5
        seed odd    bd[3] = 0.9 clamp w3 (below), bd[4] = 50 w4 (far above), bd[5] = -20 w5
    (w3, w4, w5 are powers of two in both geometries: d / w is the target exactly).  The last four box rows carry the centres:
    R - 1: x 30 m below lo, y on lo, log sizes (-2, 2, -2);  R - 2: x 30 m above hi, y on lo + ext, log sizes (2, -2, 2);  R - 3: y 3 m below
    lo;  R - 4: y 3 m above hi."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    C = 128
    c = rng.uniform(0.5, 1.5, R) * rng.choice([-1.0, 1.0], R)
    vec = lambda n: (0.5 * rng.standard_normal(n)).astype(f32)
    ln = lambda: ((0.75 + 0.5 * rng.random(C)).astype(f32), (beta + 0.1 * rng.standard_normal(C)).astype(f32))
    p = dict(obj=coherent(rng, R, C, c), w1=(coherent(rng, F, C) / C).astype(f32), b1=vec(F), w2=(coherent(rng, C, F) * 2.0 / F).astype(f32),
             b2=vec(C), n3=ln() + (EPS_N3,))

    def sparse(rows):            # `fan` live entries per row, at random places
        keep = np.argsort(rng.random((rows, C)), axis=1) < fan
        return (coherent(rng, rows, C) * keep / fan).astype(f32)

    p["cls"] = [(sparse(C),) + ln() for _ in range(n_cls)]
    p["reg"] = [(sparse(C),) + ln() for _ in range(n_reg)]
    p["eps_cls"], p["eps_reg"] = [EPS_CLS] * 4, [EPS_REG] * 4
    p["wl"], p["bl"] = sparse(ncls), vec(ncls)
    p["wd"], p["bd"] = sparse(Dd), vec(Dd)
    r = np.asarray(geom[1], np.float64)
    boxes = np.concatenate((r[:3] + rng.random((R, 3)) * (r[3:] - r[:3]), rng.uniform(-2, 2, (R, 3)), rng.standard_normal((R, Dd - 6))), 1)
    boxes = boxes.astype(f32)
    if (R >= 31) if plant is None else plant:
        w, rr, cl = np.asarray(geom[0], f32), np.asarray(geom[1], f32), f32(geom[2])
        p["wd"][[1, 3, 4, 5]] = 0.0
        p["bd"][1] = 0.0
        p["bd"][3:6] = ((f32(50) * w[3], cl * w[4], np.nextafter(cl, f32(np.inf)) * w[5]) if seed % 2 == 0 else
                        (f32(0.9) * cl * w[3], f32(50) * w[4], f32(-20) * w[5]))
        boxes[R - 1, [0, 1, 3, 4, 5]] = (rr[0] - f32(30), rr[1], -2, 2, -2)
        boxes[R - 2, [0, 1, 3, 4, 5]] = (rr[3] + f32(30), rr[4], 2, -2, 2)
        boxes[R - 3, 1], boxes[R - 4, 1] = rr[1] - f32(3), rr[4] + f32(3)
    return p, boxes


def stage_tail_device(params, boxes, dev):
    """The operands of a case on the device.  obj_in and boxes_m are the first R rows of NaN-filled buffers of R + 32 rows: a read of a row
    >= R that reaches a result shows up as NaN.  Every other tensor is exactly as long as its data."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)

    def padded(a):
        buf = torch.full((a.shape[0] + 32, a.shape[1]), float("nan"), dtype=torch.float32, device=dev)
        buf[:a.shape[0]] = t(a)
        return buf

    d = {k: t(params[k]) for k in ("w1", "b1", "w2", "b2", "wl", "bl", "wd", "bd")}
    d["n3"] = (t(params["n3"][0]), t(params["n3"][1]), float(params["n3"][2]))
    d["cls"] = [tuple(t(a) for a in layer) for layer in params["cls"]]
    d["reg"] = [tuple(t(a) for a in layer) for layer in params["reg"]]
    d["eps_cls"], d["eps_reg"] = list(params["eps_cls"]), list(params["eps_reg"])
    d["obj_buf"], d["boxes_buf"], d["R"] = padded(params["obj"]), padded(boxes), params["obj"].shape[0]
    return d


def call_stage_tail(d, geom, split, R=None, ws_bytes=None, sentinel=12345.0):
    """The raw `srf_stage_tail` call on the tensors of `stage_tail_device`.  obj_out, logits and pred are the first R rows of sentinel-filled
    buffers of R + 3 rows; with split the workspace is exactly `srf_stage_tail_workspace_bytes` long and NaN-filled before the call
    (ws_bytes: the size told to the entry point instead), without it NULL and 0; each LayerNorm gets its own eps.
    -> (return code, obj_out, logits, pred), the three full buffers."""
    import torch
    from srfdet3d_amd import _lib, ops
    L = _lib.lib()
    R = d["R"] if R is None else R
    dev = d["w1"].device
    F, ncls, Dd = d["w1"].shape[0], d["wl"].shape[0], d["wd"].shape[0]
    outs = [torch.full((R + 3, n), sentinel, dtype=torch.float32, device=dev) for n in (128, ncls, Dd)]
    ws, told = None, 0
    if split:
        need = L.srf_stage_tail_workspace_bytes(R, 128, F)
        assert need % 4 == 0
        ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev)
        told = need if ws_bytes is None else ws_bytes
    p, arr = ops._ptr, ops._ptr_array
    col = lambda layers, i: arr([layer[i] for layer in layers])
    rc = L.srf_stage_tail(
        p(d["obj_buf"]), R, 128, F, p(d["w1"]), p(d["b1"]), p(d["w2"]), p(d["b2"]), p(d["n3"][0]), p(d["n3"][1]), d["n3"][2],
        len(d["cls"]), col(d["cls"], 0), col(d["cls"], 1), col(d["cls"], 2), _lib.hf(d["eps_cls"]),
        len(d["reg"]), col(d["reg"], 0), col(d["reg"], 1), col(d["reg"], 2), _lib.hf(d["eps_reg"]),
        p(d["wl"]), p(d["bl"]), ncls, p(d["wd"]), p(d["bd"]), Dd, p(d["boxes_buf"]), _lib.hf(geom[0]), _lib.hf(geom[1]), float(geom[2]),
        p(outs[0]), p(outs[1]), p(outs[2]), None if ws is None or ws.numel() == 0 else p(ws), told, ops._stream())
    torch.cuda.synchronize()
    return (rc, *outs)


# ------------------------------------------------------------------------------------------------------------------- dpg_mix
DPG_MUTATIONS = ("expert_major", "no_half", "sigmoid_cols", "first_expert_twice")


def dpg_mix_ref(wl, wi, boxes_w, feats_w, B, E, P, mutate=None):
    """`srf_dpg_mix` as the header words it, in float64: wl, wi (B, E P) expert-major logits (wi may be None), boxes_w (E P, D),
    feats_w (E P, C) -> w = softmax over the E experts of wl or (wl + wi) / 2;  boxes[b, p] = sum_e w[b, e, p] boxes_w[e P + p] with a sigmoid
    on columns 0..2;  feats[b, p] = sum_e w feats_w[e P + p].  -> dict
         boxes (B, P, D), feats (B, P, C)
         pre     (B, P, D) the box sums before the sigmoid
         mag_b, mag_f   sum_e w |src| of each element
         T       (B, P) max |v - max v| over the experts whose logit is finite;  V (B, P) max |v| over those
    mutate: "expert_major" (the logits indexed (b, p, e)) | "no_half" (wl + wi without the division) | "sigmoid_cols" (sigmoid on columns
    0..3) | "first_expert_twice" (expert 0 counted twice, in the softmax and in the sums)."""
    d = lambda a: np.asarray(a, np.float64)
    lay = (lambda a: d(a).reshape(B, P, E).transpose(0, 2, 1)) if mutate == "expert_major" else (lambda a: d(a).reshape(B, E, P))
    v = lay(wl)
    if wi is not None:
        v = (v + lay(wi)) / (1.0 if mutate == "no_half" else 2.0)
    bw, fw = d(boxes_w).reshape(E, P, -1), d(feats_w).reshape(E, P, -1)
    if mutate == "first_expert_twice":
        v, bw, fw = np.concatenate((v, v[:, :1]), 1), np.concatenate((bw, bw[:1])), np.concatenate((fw, fw[:1]))
    m = v.max(1, keepdims=True)
    a = np.exp(v - m)
    a /= a.sum(1, keepdims=True)
    pre, feats = np.einsum("bep,epd->bpd", a, bw), np.einsum("bep,epd->bpd", a, fw)
    boxes = pre.copy()
    k = 4 if mutate == "sigmoid_cols" else 3
    boxes[..., :k] = 1.0 / (1.0 + np.exp(-pre[..., :k]))
    fin = np.isfinite(v)
    mag = lambda src: np.einsum("bep,epd->bpd", a, np.abs(src))
    return dict(boxes=boxes, feats=feats, pre=pre, mag_b=mag(bw), mag_f=mag(fw),
                T=np.where(fin, np.abs(v - m), 0.0).max(1), V=np.where(fin, np.abs(v), 0.0).max(1))


def dpg_mix_inputs(B, E, P, D, C, second, wide, seed):
    """wl (and wi when `second`) 2 N(0, 1), boxes_w and feats_w N(0, 1).  wide: the logits scaled so that the widest (b, p) has
    max |v - max v| = 60, then expert e = p % E of sample 0 set to -inf in wl at p = 0, 3, 6 (never every expert of a (b, p))."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    wl = 2.0 * rng.standard_normal((B, E, P))
    wi = 2.0 * rng.standard_normal((B, E, P)) if second else None
    if wide:
        v = wl if wi is None else (wl + wi) / 2
        k = 60.0 / (v.max(1) - v.min(1)).max()
        wl *= k
        if wi is not None:
            wi *= k
    wl = wl.astype(f32)
    if wide:
        for pp in range(0, min(P, 7), 3):
            wl[0, pp % E, pp] = -np.inf
    wi = None if wi is None else wi.astype(f32).reshape(B, E * P)
    return wl.reshape(B, E * P), wi, rng.standard_normal((E * P, D)).astype(f32), rng.standard_normal((E * P, C)).astype(f32)
