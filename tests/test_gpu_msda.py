"""`ops.msda` (csrc/msda.hip) against the float64 definition of tests/msda_ref.py on the same float32 inputs cast up.

Bound, counted from the kernel's own operation order (u = 2^-24, gamma_k = k u / (1 - k u)):

    |y - y64| <= gamma_k D + c u (max |px| + max |py| + 1) A + 1e-30 A

    D = sum a w |v|, A = sum a (|v| over the corners), both from the reference.

  relative errors of one product a w v of the sum, k = 2 T + 87:
    softmax   t = l - m: 1 rounding, so exp sees t (1 + u): e^t moves by |t| u <= T u; expf itself 2 u (1 ulp)             T + 2
              s = the L P terms added in order: 15 additions on terms that carry T + 2 each                                 T + 17
              1 / s, e * (1 / s)                                                                                             2
    bilinear  hy * hx (one product), a * (hy hx)                                                                             2
    sum       64 fused multiply-adds, one rounding each; the first term goes through all of them                            64
  T is the largest |l - m| of the case among the logits whose weight is not flushed (|l - m| <= 104: below e^-104 < 2^-150 a float32
  weight is 0, and the float64 weight is under 1e-45 of the row's largest: the 1e-30 A term).
  absolute errors, c = 4:
    position  px = fma(ref_x, W, dx) - 0.5: the fma rounds once, <= u (|px| + 0.5), the subtraction <= u |px|; the same for py.  The sample
              is continuous and piecewise linear in the position with slope <= sum |v| over the corners (of the cell next door too when
              the position rounds across an integer: the reference's A counts those), so across a floor boundary and across the
              inside test as well:                                                                     2 u (|px| + |py| + 0.5) A
    fractions ly = py - floor(py) is exact except in (-1, 0), where it rounds by <= u; hy = 1 - ly rounds by <= u: the two bilinear
              factors are off by <= u each in ABSOLUTE terms, a corner weight by <= 2 u                                     2 u A
    together 2 (|px| + |py|) + 3 <= 4 (|px| + |py| + 1).
Condition on the inputs, checked on the CPU with the reference alone: the bound stays below 1e-3 max D on every case, so a wrong corner,
level start, head slice or point order (errors of 1e-2 max D and more) cannot hide under it."""
import numpy as np
import pytest
import torch

import msda_ref as R
from srfdet3d_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

# name: (heads, d, shapes, B, Q (None: S), P, value pitch, out pitch, offsets and logits as views of one buffer)
CASES = {
    "d16_pyramid": (8, 16, R.PYRAMID, 2, None, 4, 128, 128, True),
    "d32_pyramid_pitched": (8, 32, R.PYRAMID, 2, None, 4, 320, 264, False),
    "d16_one_map_p1": (8, 16, [(5, 7)], 1, None, 1, 132, 128, True),
    "d32_one_map_q3": (8, 32, [(5, 7)], 2, 3, 4, 256, 256, False),
    "d16_pyramid_p1_q3": (8, 16, R.PYRAMID, 1, 3, 1, 128, 140, False),
    "d16_two_levels_p3": (8, 16, [(4, 3), (2, 1)], 1, 40, 3, 128, 128, True),
}
_REF = {}


def reference(name):
    """(inputs, float64 reference) of a case, computed once and left unchanged."""
    if name not in _REF:
        heads, d, shapes, B, Q, P, _, _, _ = CASES[name]
        S = sum(h * w for h, w in shapes)
        case = R.make_case(heads, d, shapes, B, S if Q is None else Q, P, seed=len(_REF) + 11)
        _REF[name] = (case, R.msda_ref(case["value"], shapes, case["ref"], case["offs"], case["logits"], heads, P))
    return _REF[name]


def bound(name):
    case, ref = reference(name)
    heads, _, shapes, _, _, P, _, _, _ = CASES[name]
    lg = case["logits"].astype(np.float64).reshape(case["logits"].shape[0], heads, -1)
    with np.errstate(invalid="ignore"):
        t = np.abs(lg - lg.max(-1, keepdims=True))
    T = float(np.nanmax(np.where(t <= 104, t, 0.0)))
    k = 2 * T + 87
    gamma = k * U / (1 - k * U)
    return gamma * ref["D"] + 4 * U * (ref["px_max"] + ref["py_max"] + 1) * ref["A"] + 1e-30 * ref["A"], k


def run(name):
    case, _ = reference(name)
    heads, d, shapes, B, Q, P, value_ld, out_ld, shared = CASES[name]
    L = len(shapes)
    ns = heads * L * P
    dev = torch.device("cuda")
    rows = case["ref"].shape[0]
    vbuf = torch.full((case["value"].shape[0], value_ld), float("nan"), device=dev)
    vbuf[:, :heads * d] = torch.from_numpy(case["value"]).to(dev)
    obuf = torch.full((rows, out_ld), -7.0, device=dev)
    offs = torch.from_numpy(case["offs"]).reshape(rows, 2 * ns).to(dev)
    logits = torch.from_numpy(case["logits"]).reshape(rows, ns).to(dev)
    if shared:
        buf = torch.cat((offs, logits), dim=1).contiguous()
        offs, logits = buf[:, :2 * ns], buf[:, 2 * ns:]
    ref = torch.from_numpy(case["ref"]).to(dev)
    out = ops.msda(vbuf[:, :heads * d], shapes, ref, offs, logits, heads, P, out=obuf[:, :heads * d])
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf.data_ptr()
    assert (obuf[:, heads * d:] == -7.0).all()          # nothing is written beyond the row's channels
    return obuf[:, :heads * d].clone()


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_is_tight_enough_to_show_a_wrong_index(name):
    _, ref = reference(name)
    bd, k = bound(name)
    ok = np.isfinite(ref["out"])
    top = ref["D"][ok].max()
    print(name, "k", k, "max bound", bd[ok].max(), "max D", top, "ratio", bd[ok].max() / top)
    assert top > 0.1 and bd[ok].max() < 1e-3 * top


@pytest.mark.parametrize("name", sorted(CASES))
def test_msda_meets_the_definition(name):
    _, ref = reference(name)
    bd, k = bound(name)
    got = run(name).double().cpu().numpy()
    nan_ref = np.isnan(ref["out"])
    assert (np.isnan(got) == nan_ref).all()              # a softmax over nothing but -inf is NaN on both sides, and nowhere else
    ok = ~nan_ref
    err = np.abs(got - ref["out"])
    ratio = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))
    print(name, "k", k, "max |y - y64|", err[ok].max(), "max bound", bd[ok].max(), "max err / bound", ratio[ok].max(), "max D", ref["D"][ok].max())
    assert (err[ok] <= bd[ok]).all()
    again = run(name)
    assert torch.equal(again.view(torch.int32), torch.from_numpy(got.astype(np.float32)).view(torch.int32).to(again.device))  # identical bits


def test_refusals_on_the_gpu():
    dev = torch.device("cuda")
    value, ref = torch.zeros(35, 128, device=dev), torch.zeros(35, 1, 2, device=dev)
    offs, logits = torch.zeros(35, 64, device=dev), torch.zeros(35, 32, device=dev)
    assert ops.msda(value, [(5, 7)], ref, offs, logits, 8, 4).shape == (35, 128)
    with pytest.raises(RuntimeError, match="msda_supported"):
        ops.msda(torch.zeros(35, 64, device=dev), [(5, 7)], ref, offs, logits, 8, 4)          # head_dim 8
    with pytest.raises(ValueError):
        ops.msda(value, [(5, 6)], ref, offs, logits, 8, 4)                                     # 35 rows are no multiple of S = 30
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.msda(value, [(5, 7)], ref.cpu(), offs, logits, 8, 4)
    assert ops.msda(value[:0], [(5, 7)], ref[:0], offs[:0], logits[:0], 8, 4).shape == (0, 128)   # nothing to do
