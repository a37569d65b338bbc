"""Float64 definitions of the decoder-stage kernels of csrc/decoder.hip as include/srfdet3d.h words them -- `srf_linear`'s chain,
`srf_self_attention(_batched)`, `srf_dynconv_mid` -- with the magnitude sums an error bound needs, the first-order error of a LayerNorm
step, the planted inputs the GPU tests share with their CPU condition checks, and `call_linear`, which reaches the arguments of
`srf_linear` that `ops.linear` fixes (any legal pitch, the caller's Y and workspace, each LayerNorm's own eps).

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
