"""The implicit-im2col convolution of the three dense GEMM families at its edges: srf_conv_gemm_nhwc (csrc/conv.hip, "f32"),
srf_conv_gemm_nhwc_split (csrc/gemm_split.hip, "split") and srf_conv_gemm_nhwc_bf16 (csrc/gemm_bf16.hip, "bf16") against
tests/conv_gemm_ref.py, which tests/test_conv_gemm_ref.py pins to torch's float64 convolution on the CPU.

Every family is called through its own C entry point: `ops.conv_gemm_nhwc` takes the split kernel from GEMM_SPLIT_MIN_TILES tiles up
only, so through it a small case would run the f32 kernel under three names.

(a) geometry -- non-square and even kernels, padding 0 / > k/2 / >= k, a map smaller than the kernel, strides 3 and > k, image boundaries
    inside a tile, workgroups past the grid, odd / > 128 / > 256 output channels -- on integers, where the answer is exact: torch.equal;
(b) the 128 x 128 tile of the f32 family with a stride, and the same bits from the 64 x 64 tile;
(c) pitched x and y in conv mode; (d) a NaN stays in the windows that cover it; (e) per-output rounding bounds on real-valued data;
(f) the empty batch."""
import os

import numpy as np
import pytest
import torch

import bf16_ref as R
import conv_gemm_ref as C
from srfdet3d_amd import _lib, ops
from srfdet3d_amd.ops import _ptr, _stream

pytestmark = pytest.mark.gpu

FAMILIES = ("f32", "split", "bf16")
_ENTRY = {"f32": ("srf_conv_gemm_nhwc", ops.pack_conv_gemm_weights), "split": ("srf_conv_gemm_nhwc_split", ops.pack_conv_gemm_split_weights),
          "bf16": ("srf_conv_gemm_nhwc_bf16", ops.pack_conv_gemm_bf16_weights)}
# srf_conv_gemm_nhwc launches its 128 x 128 tile from this many live 128 x 128 tiles up, the 64 x 64 tile below (csrc/conv.hip)
BIG_FORM_FROM = 384


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _conv(fam, x, w, stride, pad, scale=None, shift=None, relu=False, y=None):
    """x: an (N, H, W, Cin) channel slice of a channels-last GPU buffer, w (Cout, Cin, kh, kw) on the GPU -> y (a slice to write into, or
    a new tensor that starts as NaN: an output the kernel leaves out cannot pass for a value)."""
    name, pack = _ENTRY[fam]
    packed = pack(w)
    assert packed is not None
    N, H, W, Cin = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    if y is None:
        y = torch.full((N, Ho, Wo, Cout), float("nan"), device=x.device)
    assert tuple(y.shape) == (N, Ho, Wo, Cout)
    rc = getattr(_lib.lib(), name)(_ptr(x), N, H, W, Cin, ops.nhwc_ld(x), _ptr(packed), Cout, kh, kw, stride, pad, _ptr(scale), _ptr(shift),
                                   int(relu), _ptr(y), ops.nhwc_ld(y), _stream())
    assert rc == 0, (name, rc)
    return y


def _same(got, want):
    """bit-for-bit on values: `want` (float64 numpy) holds f32 values"""
    return got.shape == want.shape and torch.equal(got.cpu().double(), torch.from_numpy(want))


# ---- (a) geometry, exact on integers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "scale-shift"])
@pytest.mark.parametrize("case", C.GEOMETRY, ids=C.case_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_geometry_is_exact_on_integers(dev, fam, case, epilogue):
    """Operands of <= 8 significant bits (bf16 values), ~8 non-zero terms per output, integer scale / shift: under
    conv_gemm_ref.exact_condition every partial sum of any summation order is an exact integer and so is the epilogue's fma, so each
    family returns THE integer.  With and without the ReLU."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    x, w, scale, shift, acc, mag = C.int_reference(case, epilogue)
    assert C.exact_condition(acc, mag, scale, shift)
    xd, wd, sc, sh = _t(x, dev), _t(w, dev), _t(scale, dev), _t(shift, dev)
    for relu in (False, True):
        want = R.epilogue(acc, scale, shift, relu)
        got = _conv(fam, xd, wd, stride, pad, sc, sh, relu)
        assert _same(got, want), (fam, relu, int((got.cpu().double() != torch.from_numpy(want)).sum()))
    if pad >= kh and pad >= kw and epilogue:       # the outermost ring of outputs sees nothing but padding: relu(shift), exactly
        ring = torch.ones(got.shape[:3], dtype=torch.bool)
        ring[:, 1:-1, 1:-1] = False
        assert torch.equal(got.cpu()[ring], torch.from_numpy(shift).relu().expand(int(ring.sum()), Cout))


# ---- (b) the 128 x 128 strided form of the f32 family ------------------------------------------------------------------------
def test_the_big_case_is_on_the_128_tile_and_its_twin_is_not():
    """392 live tiles against 294: on either side of the threshold of srf_conv_gemm_nhwc, which this test reads in the source, so a
    change of the threshold says here that the cases below no longer reach both forms."""
    assert C.live_tiles(C.BIG) == 392 and C.live_tiles(C.BIG, C.BIG_TWIN_COUT) == 294
    assert C.live_tiles(C.BIG, C.BIG_TWIN_COUT) < BIG_FORM_FROM <= C.live_tiles(C.BIG)
    with open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "csrc", "conv.hip")) as f:
        assert f"if (live < {BIG_FORM_FROM})" in f.read()
    assert max(C.live_tiles(c) for c in C.GEOMETRY) < BIG_FORM_FROM        # every f32 run of (a) is on the 64 x 64 tile


@pytest.mark.parametrize("fam", FAMILIES)
def test_strided_3x3_at_392_tiles_is_exact_on_integers(dev, fam):
    """(3, 127, 129, 32) -> 512, 3x3 / stride 2 / pad 1: 64 x 65 outputs per image, M = 12480 = 97.5 row blocks (the last one half
    full, image boundaries in the middle of tiles), 4 column tiles.  The f32 family runs its <2, 2, 3, true> form here and nowhere
    else in the suite with a stride; the other two families run the same rows for the integer equality."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = C.BIG
    x, w, scale, shift, acc, mag = C.int_reference(C.BIG, True)
    assert C.exact_condition(acc, mag, scale, shift) and acc.shape == (3, 64, 65, 512)
    xd, wd = _t(x, dev), _t(w, dev)
    assert _same(_conv(fam, xd, wd, stride, pad), acc)
    assert _same(_conv(fam, xd, wd, stride, pad, _t(scale, dev), _t(shift, dev), True), R.epilogue(acc, scale, shift, True))


def test_both_tiles_of_the_f32_family_give_the_same_bits(dev):
    """The same input with the first 384 of the 512 output channels (294 live tiles: the 64 x 64 form) on real-valued data: every
    output is one k-ordered fma chain whichever tile owns it (the header of srf_conv_gemm_nhwc)."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = C.BIG
    x, w, scale, shift = C.real_case(C.BIG)
    n = C.BIG_TWIN_COUT
    xd = _t(x, dev)
    big = _conv("f32", xd, _t(w, dev), stride, pad, _t(scale, dev), _t(shift, dev), True)
    twin = _conv("f32", xd, _t(w[:n], dev), stride, pad, _t(scale[:n], dev), _t(shift[:n], dev), True)
    assert torch.isfinite(big).all() and 0.2 < (big > 0).float().mean().item() < 1.0
    assert torch.equal(big[..., :n], twin)
    big = _conv("f32", xd, _t(w, dev), stride, pad)
    assert torch.equal(big[..., :n], _conv("f32", xd, _t(w[:n], dev), stride, pad)) and (big < 0).any()


# ---- (c) pitched operands in conv mode ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,x_off,x_extra,y_off,y_extra", [(C.PITCHED[0], 4, 8, 4, 8), (C.PITCHED[1], 12, 4, 5, 6)],
                         ids=[C.case_id(c) for c in C.PITCHED])
@pytest.mark.parametrize("fam", FAMILIES)
def test_pitched_operands_in_conv_mode(dev, fam, case, x_off, x_extra, y_off, y_extra):
    """x = channels [x_off, x_off + Cin) of a wider channels-last buffer whose other channels hold 1000 (a 16-byte aligned, non-zero
    offset; x_ld > Cin), y = channels [y_off, y_off + Cout) of a buffer of sentinels: the slice is the reference, every other element
    keeps the sentinel -- the neighbours of the slice's edges included."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    x, w, scale, shift, acc, mag = C.int_reference(case, True)
    Ho, Wo = C.out_size(case)
    xbuf = torch.full((N, H, W, x_off + Cin + x_extra), 1000.0, device=dev)
    xbuf[..., x_off:x_off + Cin] = _t(x, dev)
    xs = xbuf[..., x_off:x_off + Cin]
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() != xbuf.data_ptr() and ops.nhwc_ld(xs) > Cin
    SENT = -77.0
    for relu in (False, True):
        ybuf = torch.full((N, Ho, Wo, y_off + Cout + y_extra), SENT, device=dev)
        _conv(fam, xs, _t(w, dev), stride, pad, _t(scale, dev), _t(shift, dev), relu, y=ybuf[..., y_off:y_off + Cout])
        assert _same(ybuf[..., y_off:y_off + Cout], R.epilogue(acc, scale, shift, relu))
        assert torch.all(ybuf[..., :y_off] == SENT) and torch.all(ybuf[..., y_off + Cout:] == SENT)
    assert torch.all(xbuf[..., :x_off] == 1000.0) and torch.all(xbuf[..., x_off + Cin:] == 1000.0)


# ---- (d) locality of a NaN -----------------------------------------------------------------------------------------------------
NAN_CASE = (2, 9, 11, 32, 40, 3, 3, 2, 1)


@pytest.mark.parametrize("where", [(1, 3, 5, 7), (1, 0, 0, 31), (0, 8, 10, 0)], ids=["interior", "first-corner", "last-corner"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_a_nan_stays_in_the_windows_that_cover_it(dev, fam, where):
    """One NaN in otherwise finite data, 3x3 / stride 2 / pad 1: NaN exactly in the outputs whose window holds that pixel (four for the
    interior pixel, one for a corner), in all Cout channels; every other output finite and the bits of the run without the NaN.  The
    taps outside the map are zeros that meet no NaN: padding next to it does not spread it.  The corners are the first pixel of the
    second image and the last pixel of the first: a row predicate that lets a window run into the neighbouring image carries the NaN
    across."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = NAN_CASE
    x, w, _, _ = C.real_case(NAN_CASE)
    xd, wd = _t(x, dev), _t(w, dev)
    clean = _conv(fam, xd, wd, stride, pad)
    assert torch.isfinite(clean).all()
    mask = np.zeros((N, H, W), dtype=bool)
    mask[where[:3]] = True
    hit = torch.from_numpy(C.covers(mask, kh, kw, stride, pad))
    assert int(hit.sum()) == (4 if where[1] == 3 else 1)
    xd[where] = float("nan")
    got = _conv(fam, xd, wd, stride, pad).cpu()
    assert torch.equal(torch.isnan(got), hit[..., None].expand_as(got))
    assert torch.equal(got[~hit], clean.cpu()[~hit])


# ---- (e) rounding, per output, on real-valued data -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REAL, ids=C.case_id)
@pytest.mark.parametrize("fam", FAMILIES)
def test_every_output_is_within_the_derived_bound_of_float64(dev, fam, case):
    """Post-ReLU activations, randn weights, positive scale / shift, ReLU -- and the bare accumulator -- against float64 per output:
    conv_gemm_ref.bound_f32 (f32; bf16 against the float64 of its ROUNDED operands) / bound_split, derived there from u = 2^-24 and
    K = kh kw Cin.  Two launches give the same bits."""
    N, H, W, Cin, Cout, kh, kw, stride, pad = case
    K = kh * kw * Cin
    x, w, scale, shift, acc, mag = C.real_reference(case, rounded=fam == "bf16")
    bound = C.bound_split if fam == "split" else C.bound_f32
    xd, wd = _t(x, dev), _t(w, dev)
    for sc, sh, relu in ((None, None, False), (scale, shift, True)):
        want = R.epilogue(acc, sc, sh, relu)
        tol = bound(K, mag, want, sc, sh)
        got_t = _conv(fam, xd, wd, stride, pad, _t(sc, dev), _t(sh, dev), relu)
        got = got_t.cpu().double().numpy()
        assert got.shape == want.shape
        err = np.abs(got - want)
        print(f"\n[{fam} {C.case_id(case)}{' epilogue' if relu else ''}] max err / bound = {(err / np.maximum(tol, 1e-300)).max():.3g}, "
              f"max err / max sum|x||w| = {err.max() / mag.max():.3g}, max bound / max sum|x||w| = {tol.max() / mag.max():.3g}")
        assert np.isfinite(got).all() and (err <= tol).all(), (err / np.maximum(tol, 1e-300)).max()
        assert torch.equal(_conv(fam, xd, wd, stride, pad, _t(sc, dev), _t(sh, dev), relu), got_t)
    if fam == "bf16":     # the reduced-precision kernel really ran: it is NOT within the f32 bound of the unrounded operands
        _, _, _, _, acc_u, mag_u = C.real_reference(case)
        assert (np.abs(got - R.epilogue(acc_u, scale, shift, True)) > C.bound_f32(K, mag_u, want, scale, shift)).any()


# ---- (f) the empty batch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_an_empty_batch_is_ok_and_writes_nothing(dev, fam):
    name, pack = _ENTRY[fam]
    N, H, W, Cin, Cout, kh, kw, stride, pad = C.GEOMETRY[7]
    x, w, scale, shift = C.int_case(C.GEOMETRY[7])
    Ho, Wo = C.out_size(C.GEOMETRY[7])
    xd, packed, sc, sh = _t(x, dev), pack(_t(w, dev)), _t(scale, dev), _t(shift, dev)
    y = torch.full((1, Ho, Wo, Cout), -77.0, device=dev)
    rc = getattr(_lib.lib(), name)(_ptr(xd), 0, H, W, Cin, Cin, _ptr(packed), Cout, kh, kw, stride, pad, _ptr(sc), _ptr(sh), 1, _ptr(y), Cout,
                                   _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(y == -77.0)
