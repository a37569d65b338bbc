"""Training-time 3x3 convolutions of the camera branch on the library's Winograd kernel (config 4 of BASELINE.json trains
VoVNet stages 4-5, the image FPN, `img_convs` and the head: tools/train.py:220-234, vovnet.py:354-374).

torch's autograd runs these layers on MIOpen: its fp32 3x3 algorithm is the VALU Winograd F(2x3) kernel for the forward AND the
data gradient (142 launches, 68 of the 340 ms of kernel time of a bs = 2 step: profiles/r03_train_step_kernels_before.md), wrapped
in NCHW <-> NHWC transposes for the weight gradient.  Here

* forward        y = conv(x, W) + b              -> `srf_wino43` (F(4x4, 3x3) on the f32 MFMA) on the channels-last tensor;
* data gradient  dx = conv(dy, rot180(W)^T)      -> the SAME kernel: a stride-1 3x3 convolution of dy with the weights rotated
                                                    by 180 degrees and their in / out channel axes swapped (packed once per step);
* weight grad    dW = sum_p dy[p] x[p + tap]     -> aten.convolution_backward with only the weight mask set (MIOpen's NHWC
                                                    implicit-GEMM kernels; both operands are already channels-last, so the
                                                    transposes around them disappear);
* bias grad      db = sum_p dy[p].

Tensors stay logical NCHW with channels_last strides, which every torch op of the module path preserves (BatchNorm in eval
mode -- `norm_eval=True` -- ReLU, cat, max_pool2d, nearest interpolate), so nothing is copied between the layers.
"""
import os
import weakref
from collections import namedtuple

import torch
from torch import nn

from . import derived, mfma_mode, ops

# The SRF_TRAIN_* switches: A/B switches for tests and benchmarks, "1" when unset, read on every call (tests flip them mid-process).
_SWITCHES = {
    "CONV": "0: no route of this file is taken -- every layer runs as torch's own module",
    "FUSED": "0: conv -> eval BatchNorm -> ReLU as three autograd nodes (`conv2d`, `bn_eval`, relu), not `_ConvAffineRelu` / `_OSAChain`",
    "OSA": "0: the layers of an OSA block as `_ConvAffineRelu` nodes, not one `_OSAChain`",
    "ESE": "0: the eSE module as torch ops, not `_ESEApply`",
    "CONV1X1": "0: the bias-carrying 1x1 layers as torch's `linear` on the pixel view, not `_Conv1x1`",
    "WGRAD": "0: weight gradients on the library route (aten.convolution_backward, one GEMM for 1x1), not `srf_conv_wgrad_nhwc`; "
             "2: on `srf_conv_wgrad_nhwc` whatever share of its tiles a layer fills",
}
# SRF_TRAIN_CONV_DEBUG (read once, at import): (input shape, Cout, events) of every weight-gradient call, for `debug_report`
_DEBUG = [] if os.environ.get("SRF_TRAIN_CONV_DEBUG") else None


def switch(name, _env={k: "SRF_TRAIN_" + k for k in _SWITCHES}):
    return os.environ.get(_env[name], "1")   # KeyError: not a switch of this file


def enabled():
    return switch("CONV") != "0"


def debug_report():
    torch.cuda.synchronize()
    rows = {}
    for shp, co, e0, e1 in _DEBUG or []:
        r = rows.setdefault((shp, co), [0, 0.0])
        r[0] += 1
        r[1] += e0.elapsed_time(e1)
    return sorted(((k, n, ms / n) for k, (n, ms) in rows.items()), key=lambda t: -t[2] * t[1])


# ---- the gate --------------------------------------------------------------------------------------------------------
# "This tensor trains on the library's kernels": autograd is recording and x is an f32 GPU tensor -- plus, per route, the switches that
# must be on and what else the route asks of x.  The differences are as they grew; each is pinned by tests/test_gpu_train_gate.py.
_Route = namedtuple("_Route", "switches no_autocast dim4 channels_last")
_ROUTES = {
    "wino43":    _Route(("CONV",),        True,  True,  False),   # `eligible`: NCHW tensors too (`_Wino43Conv` keeps the caller's format)
    "conv1x1":   _Route(("CONV",),        True,  True,  True),    # `eligible_1x1`
    "depthwise": _Route(("CONV",),        False, True,  False),   # `eligible_depthwise`: does not look at autocast
    "fused":     _Route(("CONV",),        True,  True,  True),    # `fused_eligible` (its caller consults FUSED: the "dense" row)
    "osa":       _Route(("OSA", "FUSED"), True,  True,  True),    # `osa_eligible`: CONV is left to its caller
    "ese":       _Route(("CONV", "ESE"),  True,  True,  True),    # `ese_eligible`
    "bn_eval":   _Route(("CONV",),        True,  False, False),   # `bn_eval`: does not look at dim()
    "dense":     _Route(("FUSED",),       True,  False, False),   # `dense._train_fusable`: FUSED but not CONV
}


def trains(route, x):
    switches, no_autocast, dim4, channels_last = _ROUTES[route]
    for s in switches:
        if switch(s) == "0":
            return False
    return (torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and (not dim4 or x.dim() == 4)
            and (not channels_last or x.stride(1) == 1) and (not no_autocast or not torch.is_autocast_enabled()))


def _plain_conv(conv, k):
    """nn.Conv2d itself, k x k / stride 1 / padding k // 2, dense."""
    return (type(conv) is nn.Conv2d and conv.kernel_size == (k, k) and conv.stride == (1, 1) and conv.padding == (k // 2, k // 2)
            and conv.dilation == (1, 1) and conv.groups == 1)


# ---- shape limits of a layer, as functions of integers (the kernels' own limits: ops.py) ------------------------------------------
MAX_COUT = 1024   # channels of one block of srf_nhwc_affine_relu_bwd's column sums (csrc/nhwc.hip:592); `_Conv1x1` keeps the same bound


def wino_layer_ok(N, H, W, Cin, Cout):
    """A 3x3 layer on srf_wino43 forward (Cin -> Cout) and backward (Cout -> Cin: Cout % 8 too); below 32 input channels it stays on torch."""
    return ops.wino43_channels_ok(Cin, Cout) and Cout % 8 == 0 and Cin >= 32 and ops.wino43_range_ok(N * H * W, max(Cin, Cout))


def gemm_layer_ok(N, H, W, Cin, Cout):
    """A 1x1 layer on the library's GEMMs in three directions: K = Cin forward, K = Cout backward, both tensors in the weight gradient's range."""
    return (ops.gemm_k_ok(Cin) and ops.gemm_k_ok(Cout) and Cout <= MAX_COUT and H * W > 1 and ops.below_2gb(N * H * W, max(Cin, Cout)))


def fused_layer_ok(k, N, H, W, Cin, Cout):
    """conv k x k -> eval BatchNorm -> ReLU as a layer of `_ConvAffineRelu` or `_OSAChain`."""
    if k == 3:
        return wino_layer_ok(N, H, W, Cin, Cout) and Cout <= MAX_COUT and ops.wino43_tiles_ok(N, H, W)
    return k == 1 and gemm_layer_ok(N, H, W, Cin, Cout)


# ---- the bf16-product mode (csrc/gemm_bf16.hip forward and data gradient, csrc/wgrad_bf16.hip weight gradient) ---------------------
class mfma_dtype(mfma_mode.MfmaMode):
    """Within `with train_conv.mfma_dtype(torch.bfloat16):` the convolutions of `_Wino43Conv`, `_ConvAffineRelu`, `_OSAChain` and `_Conv1x1`
    run on ONE bf16 product per f32 product in all three directions: f32 tensors, both operands rounded to bf16 once, exact products, f32
    accumulation -- forward on `srf_conv_gemm_nhwc_bf16` (3x3; no Winograd in this mode) / `srf_conv1x1_nhwc_bf16`, the data gradient on
    the same kernels with the rotated / transposed weight, the weight gradient on `srf_conv_wgrad_nhwc_bf16`.  All three see the same
    bf16(W).  Everything else is unchanged and f32: the folded-BatchNorm / ReLU epilogue, `srf_nhwc_affine_relu_bwd`, `bn_eval_grads`,
    `_ESEApply`, the depthwise node and the gate.  A node records the mode in its forward pass and its backward pass follows that record
    (`loss.backward()` runs after the context has closed).  Off by default; `mfma_dtype(None)` switches an outer context off.

    A layer whose forward or data gradient the bf16 kernels cannot take (`bf16_layer_ok`, operand alignment) keeps today's route for
    both; a weight gradient the new kernel refuses goes through `_weight_grad`.
    routes: a list that receives one dict(layer=, direction="fwd" | "dgrad" | "wgrad", route="bf16" | "f32", why=) per executed
    direction; `launches` counts the directions that ran on the bf16 kernels.  Process-wide while open, as `nhwc.mfma_dtype`."""


def bf16_layer_ok(k, N, H, W, Cin, Cout):
    """A k x k layer on the bf16-product GEMMs forward (K = Cin) and backward (K = Cout), as dense tensors: both channel counts in chunks
    of 32, a 128-row tile of either tensor and (3x3: one image of either) inside the kernels' 32-bit ranges."""
    C = max(Cin, Cout)
    return (k in (1, 3) and N > 0 and ops.gemm_k_ok(Cin) and ops.gemm_k_ok(Cout) and ops.gemm_rows_ok(C) and (k == 1 or ops.below_2gb(H * W, C)))


class _LayerMode:
    """What a node keeps of the mode that was active in its forward pass: the context (its report outlives it) and why the layer's
    forward and data gradient stay f32 (None: they run on the bf16 kernels)."""
    __slots__ = ("mode", "layer", "why")

    def __init__(self, mode, layer, why):
        self.mode, self.layer, self.why = mode, layer, why

    @property
    def bf16(self):
        return self.why is None

    def report(self, direction, why=False):
        self.mode.report(self.layer, self.why if why is False else why, direction=direction)


class _NoMode:
    """What it keeps of a forward pass outside the mode: every direction on its f32 route, nothing to report."""
    bf16 = False

    def report(self, direction, why=False):
        pass


_F32 = _NoMode()


def _layer_mode(k, xn, Cout, out=None):
    """At a layer's forward pass: `_F32` outside the mode, else its record (and the report's "fwd" row)."""
    m = mfma_dtype.active()
    if m is None:
        return _F32
    N, H, W, Cin = xn.shape
    lm = _LayerMode(m, f"{Cin}->{Cout} {k}x{k} @{N}x{H}x{W}", ops.gemm_bf16_why_not(xn, Cout, out, im2col=k == 3, dgrad=True))
    lm.report("fwd")
    return lm


def _weight_grad_in(lm, gn, xn, weight, k):
    """The weight gradient of a node whose forward pass recorded lm: outside the mode `_weight_grad` as ever; in it `srf_conv_wgrad_nhwc_bf16`
    (whatever route the layer's other two directions took), unless the kernel refuses the operands."""
    if lm is not _F32:
        if ops.conv_wgrad_bf16_supported(gn, xn, k):
            lm.report("wgrad", None)
            return ops.conv_wgrad_nhwc_bf16(gn, xn, k)
        lm.report("wgrad", "channel counts or pitches that are no multiple of 4, alignment, or a tensor of 2 GB")
    return _weight_grad(gn, xn, weight, k)


# ---- one layer in its three directions ---------------------------------------------------------------------------------
def _nhwc(t):
    """logical NCHW tensor -> its (N, H, W, C) view over channels-last storage (a copy only if it was not channels-last)."""
    return t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)


def _layer_fwd(xn, w, scale=None, shift=None, relu=False, out=None, bf16=False):
    """A layer on the channels-last slice xn: w (Cout, Cin, 3, 3) on `srf_wino43`, (Cout, Cin[, 1, 1]) on the 1x1 GEMM; packed once per call.
    bf16 (the `mfma_dtype` mode): on `srf_conv_gemm_nhwc_bf16` / `srf_conv1x1_nhwc_bf16` instead, the weight rounded to bf16 as it is packed."""
    Cout = w.shape[0]
    if bf16:
        if w.dim() == 4 and w.shape[2] == 3:
            return ops.conv_gemm_nhwc(xn, None, Cout, (3, 3), 1, 1, scale, shift, relu, out=out, packed_bf16=ops.pack_conv_gemm_bf16_weights(w))
        return ops.conv1x1_nhwc(xn, None, Cout, scale, shift, relu, out=out, packed_bf16=ops.pack_conv1x1_nhwc_bf16_weights(w.reshape(Cout, -1)))
    if w.dim() == 4 and w.shape[2] == 3:
        return ops.wino43(xn, ops.pack_wino43_weights(w), Cout, scale, shift, relu, out=out)
    w2 = w.reshape(Cout, -1)
    return ops.conv1x1_nhwc(xn, lambda: ops.pack_conv1x1_nhwc_weights(w2), Cout, scale, shift, relu, out=out,
                            packed_split=lambda: ops.pack_conv1x1_nhwc_split_weights(w2))


def _layer_dgrad(gn, w, lm=_F32):
    """Its data gradient: the same kernels on the weight rotated by 180 degrees with the channel axes swapped (3x3), transposed (1x1).
    lm: what the node recorded of the mode in its forward pass (rounding commutes with the rotation and the transposition: bf16(W) again)."""
    if w.shape[2] == 3:
        wt = w.flip(2, 3).transpose(0, 1).contiguous()      # (Cin, Cout, 3, 3)
    else:
        wt = w.reshape(w.shape[0], w.shape[1]).t().contiguous()  # (Cin, Cout)
    lm.report("dgrad")
    if lm.bf16 and not ops.operand_ok(ops.nhwc_ld(gn), gn.data_ptr()):
        gn = gn.contiguous()
    return _layer_fwd(gn, wt, bf16=lm.bf16)


def _weight_grad(gn, xn, weight, k):
    """dW of a stride-1 convolution from the channels-last output gradient gn (N, H, W, Cout) and input xn (N, H, W, Cin).
    `srf_conv_wgrad_nhwc` (round 5: an f32 GEMM over the pixels on the bf16 MFMA, exact three-way split of both operands, pixel ranges
    added in a fixed order -- deterministic) where it applies; else (SRF_TRAIN_WGRAD=0, maps narrower than 32 pixels, tensors of 2 GB)
    the library route of rounds 3-4: aten.convolution_backward = MIOpen's float-atomic split-K kernels for 3x3, one rocBLAS GEMM for 1x1."""
    Co, Ci = weight.shape[0], weight.shape[1]
    if _DEBUG is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    cols = k * k * Ci if (k > 1 and Ci % 32 == 0) else Ci            # 3x3 layers: the column tiles run over the flattened (tap, channel) axis
    fill = (Co * cols) / float(((Co + 127) // 128) * ((cols + 127) // 128) * 128 * 128)   # share of the kernel's 128 x 128 tiles that is real
    # (192 -> 192, VoVNet stage 4, with every tap's channels in tiles of their own: 56 % -- 543 us against MIOpen's 465; flattened: 72 %;
    # every other trainable shape of config 4 is 1.1-3x faster on the kernel: profiles/r05_wgrad_bench.txt)
    want = switch("WGRAD")
    if want != "0" and (fill >= 0.6 or k == 1 or want == "2") and ops.conv_wgrad_supported(gn, xn, k):
        gw = ops.conv_wgrad_nhwc(gn, xn, k)
    elif k == 1:
        gw = (gn.reshape(-1, Co).t() @ xn.reshape(-1, Ci)).view(Co, Ci, 1, 1)
    else:
        gw = torch.ops.aten.convolution_backward(gn.permute(0, 3, 1, 2), xn.permute(0, 3, 1, 2), weight, None, (1, 1), (1, 1), (1, 1), False,
                                                 (0, 0), 1, (False, True, False))[1]
    if _DEBUG is not None:
        e1.record()
        _DEBUG.append(((xn.shape[0], Ci, xn.shape[1], xn.shape[2]), Co, e0, e1))
    return gw


def _bn_relu_bwd(gyn, yn, fold, mean, relu, need_gamma, need_beta, gy2=None):
    """The head of a fused layer's backward pass: `srf_nhwc_affine_relu_bwd` (ReLU mask, scale and the two column sums; gy2 is a second
    gradient of the same output, added on the way in), then d gamma / d beta where asked -> gz, sums, d gamma, d beta.
    u = (z - mean) inv gamma + beta:  d gamma = inv (sum gu z - mean sum gu),  sum gu z = (sum gu y - t0 sum gu) / s;  d beta = sum gu."""
    gz, sums = ops.nhwc_affine_relu_bwd(gyn, yn, fold[0], relu, gy2=gy2)
    pg = ops.bn_eval_grads(sums, fold, mean) if (need_gamma or need_beta) else None
    return gz, sums, pg[0] if need_gamma else None, pg[1] if need_beta else None


# ---- the nodes -------------------------------------------------------------------------------------------------------
def eligible(conv, x):
    """A trainable (or gradient-carrying) 3x3 / stride 1 / padding 1 convolution on an fp32 GPU tensor under autograd."""
    return (trains("wino43", x) and _plain_conv(conv, 3) and conv.padding_mode == "zeros" and (x.requires_grad or conv.weight.requires_grad)
            and wino_layer_ok(x.shape[0], x.shape[2], x.shape[3], conv.in_channels, conv.out_channels))


class _Wino43Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        xn = _nhwc(x)
        ctx.lm = lm = _layer_mode(3, xn, weight.shape[0])
        y = _layer_fwd(xn, weight.detach(), None, None if bias is None else bias.detach(), False, bf16=lm.bf16)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.keep_cl = x.stride(1) == 1
        y = y.permute(0, 3, 1, 2)             # logical NCHW, channels-last strides
        # The caller's memory format is kept: a channels-last input (the camera branch behind the frozen prefix, whose BatchNorms
        # are in eval mode and run as affine maps) gets a channels-last output without a copy; an NCHW-contiguous input (the BEV
        # backbone of the LiDAR-only configs, BatchNorm in TRAIN mode) gets NCHW back -- MIOpen's training batch-norm on a
        # channels-last tensor crashed the process behind a stride-2 convolution of the BEV FPN
        # (profiles/r03_fault_pytest_segfault_20261005.log).
        return y if ctx.keep_cl else y.contiguous()

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gyn = _nhwc(gy)
        gy_cl = gyn.permute(0, 3, 1, 2)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _layer_dgrad(gyn, weight.detach(), ctx.lm).permute(0, 3, 1, 2)
            if not ctx.keep_cl:
                gx = gx.contiguous()
        if ctx.needs_input_grad[1]:
            gw = _weight_grad_in(ctx.lm, gyn, _nhwc(x), weight, 3)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy_cl.sum(dim=(0, 2, 3))
        return gx, gw, gb


class _ConvAffineRelu(torch.autograd.Function):
    """conv (3x3 / stride 1 on `srf_wino43`, or 1x1 on the library's GEMM) -> BatchNorm2d in EVAL mode (`norm_eval=True`: an affine
    map with trainable gamma / beta) -> ReLU as ONE forward launch -- the inference kernel with the folded BatchNorm and the ReLU in
    its epilogue -- and a backward pass that starts with ONE streaming kernel (`srf_nhwc_affine_relu_bwd`: ReLU mask, scale, and
    the two column sums gamma / beta need).  As torch ops the same chain is conv, multiply, add, relu_ forward and
    threshold_backward, multiply and two strided column sums backward: eight passes over each layer's output instead of two.
    Only y is saved (not the convolution's own output z): sum gu z = (sum gu y - t sum gu) / s since z = (y - t) / s wherever the mask
    lets a gradient through -- which needs s away from 0: `conv_bn_act` takes this node only for layers whose min |s| >= 1e-3 max |s|
    (`gamma_well_conditioned`; anything else runs under plain autograd), and a frozen gamma needs no d gamma at all."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, mean, var, eps, relu):
        xn = _nhwc(x)
        fold = ops.bn_eval_fold(gamma.detach(), beta.detach(), mean, var, eps)     # s, t0, inv in one launch
        s, t0 = fold[0], fold[1]
        t = t0 if bias is None else t0 + bias.detach() * s
        ctx.lm = lm = _layer_mode(weight.shape[2], xn, weight.shape[0])
        yn = _layer_fwd(xn, weight.detach(), s, t, relu, bf16=lm.bf16)
        ctx.save_for_backward(x, weight, yn, fold, mean)
        ctx.relu, ctx.has_bias = bool(relu), bias is not None
        return yn.permute(0, 3, 1, 2)          # logical NCHW, channels-last strides

    @staticmethod
    def backward(ctx, gy):
        x, weight, yn, fold, mean = ctx.saved_tensors
        need = ctx.needs_input_grad
        gz, sums, ggamma, gbeta = _bn_relu_bwd(_nhwc(gy), yn, fold, mean, ctx.relu, need[3], need[4])
        gx = gw = gb = None
        if ctx.has_bias and need[2]:
            gb = sums[0] * fold[0]
        if need[0]:
            gx = _layer_dgrad(gz, weight.detach(), ctx.lm).permute(0, 3, 1, 2)
        if need[1]:
            gw = _weight_grad_in(ctx.lm, gz, _nhwc(x), weight, weight.shape[2])
        return gx, gw, gb, ggamma, gbeta, None, None, None, None


def fused_eligible(conv, bn, x):
    """conv -> eval-mode BatchNorm2d (-> ReLU) under autograd on a channels-last tensor, in the shapes `_ConvAffineRelu` covers."""
    if not (trains("fused", x) and derived.foldable_bn(bn, nn.BatchNorm2d)):
        return False
    N, _, H, W = x.shape
    if eligible(conv, x):
        return fused_layer_ok(3, N, H, W, conv.in_channels, conv.out_channels) and ops.wino43_supported(x.permute(0, 2, 3, 1), conv.out_channels)
    return eligible_1x1(conv, x) and fused_layer_ok(1, N, H, W, conv.in_channels, conv.out_channels)


GAMMA_GUARD_RATIO = 1e-3   # min |s| / max |s| of a layer below which `_ConvAffineRelu` is not used (s = gamma / sqrt(var + eps))
_GUARD = weakref.WeakKeyDictionary()   # BatchNorm2d -> ((gamma version, gamma pointer, var version), well conditioned?)


def _guard_key(bn):
    return (bn.weight._version, bn.weight.data_ptr(), bn.running_var._version)


def gamma_well_conditioned(bn):
    """`_ConvAffineRelu` rebuilds sum gu z from the saved OUTPUT, (sum gu y - t sum gu) / s: a channel with s = 0 has no such
    term at all (its true d gamma is not zero, so a zero-initialised or pruned channel could never recover) and a small |s|
    amplifies the rounding of two column sums by 1 / s.  The node is therefore used only for layers whose
    min |s| >= GAMMA_GUARD_RATIO max |s|; any other layer runs conv2d / bn_eval / relu under plain autograd, which is exact.
    The verdict is cached per (gamma version, pointer); when one is stale, the verdicts of ALL layers seen so far are refreshed
    in one batch -- two concatenations, two segment reductions and ONE device -> host copy per optimiser step, not one per layer."""
    ent = _GUARD.get(bn)
    if ent is not None and ent[0] == _guard_key(bn):
        return ent[1]
    dev = bn.weight.device
    mods = [m for m, e in list(_GUARD.items()) if m is not bn and m.weight.device == dev and e[0] != _guard_key(m)] + [bn]
    with torch.no_grad():
        lengths = [m.weight.numel() for m in mods]
        g = torch.cat([m.weight.detach().reshape(-1) for m in mods]).abs()
        v = torch.cat([m.running_var.reshape(-1) for m in mods])
        eps = torch.repeat_interleave(torch.tensor([float(m.eps) for m in mods], dtype=v.dtype), torch.tensor(lengths)).to(dev)
        s = g * torch.rsqrt(v + eps)
        lt = torch.tensor(lengths, device=dev)
        lo = torch.segment_reduce(s, "min", lengths=lt)
        hi = torch.segment_reduce(s, "max", lengths=lt)
        ok = ((hi > 0) & (lo >= GAMMA_GUARD_RATIO * hi) & torch.isfinite(hi)).tolist()     # the one synchronisation
    for m, o in zip(mods, ok):
        _GUARD[m] = (_guard_key(m), bool(o))
    return _GUARD[bn][1]


def conv_bn_act(conv, bn, relu, x):
    """The fused training route when it applies, else None (the caller then runs conv2d / bn_eval / relu)."""
    if fused_eligible(conv, bn, x) and (not bn.weight.requires_grad or gamma_well_conditioned(bn)):
        return _ConvAffineRelu.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bool(relu))
    return None


# What `_OSAChain` takes per layer behind (x, eps), in this order: `osa_chain` packs it, the node unpacks its arguments, their need flags
# and its gradients by it.
_OSALayer = namedtuple("_OSALayer", "weight gamma beta mean var")
_OSASaved = namedtuple("_OSASaved", "weight mean fold")   # what it saves per layer behind (cat, yc); fold = (3, C): s, t0, inv


def _records(flat, cls):
    n = len(cls._fields)
    return [cls(*flat[i:i + n]) for i in range(0, len(flat), n)]


class _OSAChain(torch.autograd.Function):
    """The body of a VoVNet OSA block (vovnet.py:208-230) -- L x [conv 3x3 -> eval BatchNorm -> ReLU] in a chain, then the 1x1 `concat`
    convolution over [x, y_0 .. y_{L-1}] -> eval BatchNorm -> ReLU -- as ONE autograd node over ONE channels-last buffer
    cat = [x | y_0 | .. | y_{L-1}]:

    * forward: every layer reads its input slice of `cat` and writes its output slice (the kernels take a pixel pitch), the concat
      convolution reads `cat` in place: no torch.cat, and `cat` is all that is saved (it holds every layer's input AND output);
    * backward: the concat convolution's data gradient g_cat has the same layout; layer i's output gradient is g_cat's slice PLUS the
      data gradient of layer i + 1 -- added inside the ReLU / BatchNorm backward pass (`srf_nhwc_affine_relu_bwd2`), read from the slice
      in place.  As separate `_ConvAffineRelu` nodes autograd made that sum with a strided add per layer (213 launches, 7.3 ms per
      step) after a contiguous copy of the slice (4.3 ms) and torch.cat had copied every output once more forward (2.9 ms):
      profiles/r05_train_step_kernels.md.
    Same arithmetic per layer as `_ConvAffineRelu` (same kernels, same d gamma / d beta formulas); the one difference is where the two
    gradients of an output are added (one f32 add either way)."""

    @staticmethod
    def forward(ctx, x, eps, *params):
        layers = _records(params, _OSALayer)       # L chain layers, then the concat convolution
        L = len(layers) - 1
        xn = _nhwc(x)
        N, H, W, Cin = xn.shape
        widths = [int(p.weight.shape[0]) for p in layers[:L]]
        Ctot = Cin + sum(widths)
        cat = torch.empty((N, H, W, Ctot), dtype=torch.float32, device=x.device)
        cat[..., :Cin].copy_(xn)
        saved = []
        ctx.lms = lms = []         # per layer: what it recorded of the `mfma_dtype` mode
        lo, hi = 0, Cin            # the input slice of the next layer
        for i, p in enumerate(layers):
            fold = ops.bn_eval_fold(p.gamma.detach(), p.beta.detach(), p.mean, p.var, eps[i])
            if i < L:
                xs, ys = cat[..., lo:hi], cat[..., hi:hi + widths[i]]
                lms.append(_layer_mode(3, xs, widths[i], ys))
                _layer_fwd(xs, p.weight.detach(), fold[0], fold[1], True, out=ys, bf16=lms[i].bf16)
                lo, hi = hi, hi + widths[i]
            else:
                lms.append(_layer_mode(1, cat, int(p.weight.shape[0])))
                yc = _layer_fwd(cat, p.weight.detach(), fold[0], fold[1], True, bf16=lms[i].bf16)
            saved += [p.weight, p.mean, fold]
        ctx.save_for_backward(cat, yc, *saved)
        ctx.Cin, ctx.widths = Cin, widths
        return yc.permute(0, 3, 1, 2)          # logical NCHW, channels-last strides

    @staticmethod
    def backward(ctx, gy):
        Cin, widths = ctx.Cin, ctx.widths
        L = len(widths)
        cat, yc = ctx.saved_tensors[:2]
        layers = _records(ctx.saved_tensors[2:], _OSASaved)
        need_x = ctx.needs_input_grad[0]
        need = _records(ctx.needs_input_grad[2:], _OSALayer)
        grads = [[None] * len(_OSALayer._fields) for _ in layers]     # d weight, d gamma, d beta, -, - of every layer

        # the concat convolution
        Ctot = cat.shape[3]
        p = layers[L]
        gz, _, grads[L][1], grads[L][2] = _bn_relu_bwd(_nhwc(gy), yc, p.fold, p.mean, True, need[L].gamma, need[L].beta)
        g_cat = _layer_dgrad(gz, p.weight.detach(), ctx.lms[L])
        if need[L].weight:
            grads[L][0] = _weight_grad_in(ctx.lms[L], gz, cat, p.weight, 1)
        del gz
        # the chain, last layer first
        carry = None
        out_hi = Ctot
        for i in range(L - 1, -1, -1):
            p = layers[i]
            out_lo = out_hi - widths[i]
            in_lo, in_hi = (0, Cin) if i == 0 else (out_lo - widths[i - 1], out_lo)
            gz, _, grads[i][1], grads[i][2] = _bn_relu_bwd(g_cat[..., out_lo:out_hi], cat[..., out_lo:out_hi], p.fold, p.mean, True,
                                                           need[i].gamma, need[i].beta, gy2=carry)
            if need[i].weight:
                grads[i][0] = _weight_grad_in(ctx.lms[i], gz, cat[..., in_lo:in_hi], p.weight, 3)
            carry = _layer_dgrad(gz, p.weight.detach(), ctx.lms[i]) if (i > 0 or need_x) else None
            out_hi = out_lo
        gx = carry.add_(g_cat[..., :Cin]).permute(0, 3, 1, 2) if need_x else None
        return (gx, None, *[g for rec in grads for g in rec])


class _ESEApply(torch.autograd.Function):
    """VoVNet's eSE module applied to an OSA block's output (vovnet.py:165-177, :225-228): y = out * hsigmoid(fc(mean(out))) (+ identity)
    as one autograd node on channels-last tensors.  Forward: pixel mean, the gate GEMV, one streaming pass (the inference kernels).
    Backward: ONE pass for the pixel sums of g * out (what the gate's gradient needs), the (N, C)-sized arithmetic of the gate, ONE pass
    d out = g * gate + d mean / HW; the identity's gradient is g itself.  As torch ops the same backward is two multiplies, a
    reduction, an expand and an add over the block's output -- five passes over 53 M elements per stage-4 block."""

    @staticmethod
    def forward(ctx, out, identity, weight, bias):
        xn = _nhwc(out)
        N, H, W, C = xn.shape
        mean = ops.nhwc_colmean(xn)
        gate = ops.ese_gate(mean, weight.detach(), bias.detach())
        y = ops.nhwc_affine(xn, scale=gate, residual=None if identity is None else _nhwc(identity))
        ctx.save_for_backward(out, mean, gate, weight, bias)
        ctx.has_identity = identity is not None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        out, mean, gate, weight, bias = ctx.saved_tensors
        gn, xn = _nhwc(g), _nhwc(out)
        N, H, W, C = xn.shape
        need = ctx.needs_input_grad
        d_out = d_w = d_b = None
        w2 = weight.detach().reshape(C, C)
        s = ops.nhwc_colsum_prod(gn, xn)                                   # (N, C): sum_p g * out = d gate
        pre = torch.addmm(bias.detach(), mean, w2.t())                     # fc(mean): the gate's argument
        dpre = s * ((pre > -3.0) & (pre < 3.0)).to(s.dtype) / 6.0          # hsigmoid = relu6(. + 3) / 6
        if need[2]:
            d_w = (dpre.t() @ mean).view_as(weight)
        if need[3]:
            d_b = dpre.sum(0)
        if need[0]:
            dmean = (dpre @ w2) / float(H * W)                            # back through the pixel mean
            d_out = ops.nhwc_affine(gn, scale=gate, shift=dmean).permute(0, 3, 1, 2)
        return d_out, (g if (ctx.has_identity and need[1]) else None), d_w, d_b


def ese_eligible(mod, x, identity):
    """The eSE module under autograd on a channels-last f32 GPU tensor (SRF_TRAIN_ESE=0: the torch ops)."""
    return (trains("ese", x) and x.shape[1] % 4 == 0 and 0 < x.shape[1] <= 1024 and x.shape[0] <= 65535
            and (x.requires_grad or mod.fc.weight.requires_grad)
            and (identity is None or (tuple(identity.shape) == tuple(x.shape) and identity.stride(1) == 1))
            and type(mod.fc) is nn.Conv2d and mod.fc.kernel_size == (1, 1) and mod.fc.bias is not None)


def ese_apply(mod, x, identity):
    return _ESEApply.apply(x, identity, mod.fc.weight, mod.fc.bias)


def osa_eligible(block, x):
    """An OSA block whose body can run as `_OSAChain`: plain 3x3 layers (no reduction / depthwise form), every layer and the concat
    convolution fit `_ConvAffineRelu`'s conditions (`fused_layer_ok`) with bias-free convolutions and eval-mode BatchNorms with
    well-conditioned gammas, and the input is channels-last under autograd.  SRF_TRAIN_OSA=0 keeps the per-layer nodes."""
    if not (trains("osa", x) and block.reduce is None and len(block.layers) >= 1):
        return False
    N, _, H, W = x.shape
    seqs = list(block.layers) + [block.concat]
    cin = ctot = x.shape[1]            # the running width of the chain, the width of `cat`
    for seq in seqs:
        mods = list(seq.children())
        if len(mods) != 3 or type(mods[0]) is not nn.Conv2d or not isinstance(mods[2], nn.ReLU) or mods[0].bias is not None:
            return False
        conv, bn = mods[0], mods[1]
        k, width = (1, ctot) if seq is seqs[-1] else (3, cin)
        if not (derived.foldable_bn(bn, nn.BatchNorm2d) and _plain_conv(conv, k) and conv.padding_mode == "zeros" and conv.in_channels == width
                and fused_layer_ok(k, N, H, W, width, conv.out_channels)):
            return False
        if k == 3:
            cin = conv.out_channels
            ctot += cin
        if bn.weight.requires_grad and not gamma_well_conditioned(bn):
            return False
    if not (x.requires_grad or any(p.requires_grad for seq in seqs for p in seq.parameters())):
        return False
    return ops.below_2gb(N * H * W, ctot)   # `cat` and the concat convolution's data gradient feed the weight gradients


def osa_chain(block, x):
    seqs = list(block.layers) + [block.concat]
    layers = [_OSALayer(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var) for conv, bn, _ in seqs]
    return _OSAChain.apply(x, tuple(float(seq[1].eps) for seq in seqs), *[t for p in layers for t in p])


class _DepthwiseNative(torch.autograd.Function):
    """Depthwise convolutions (the stride-2 stair of the proposal generator, srfdet_head.py:520-537) on torch's own depthwise
    kernels in BOTH directions.  The forward already kept MIOpen away (its choice is a naive reference kernel: 34 ms on the
    finest image level); under autograd the backward ran outside that context and MIOpen's weight gradient for the grouped
    convolution was one 59 ms CK batched-GEMM launch per step (profiles/r03_train_step_kernels_before.md)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, groups):
        ctx.save_for_backward(x, weight)
        ctx.cfg = (stride, padding, groups, bias is not None)
        with torch.backends.cudnn.flags(enabled=False):
            return torch.nn.functional.conv2d(x, weight, bias, stride, padding, 1, groups)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, padding, groups, has_bias = ctx.cfg
        with torch.backends.cudnn.flags(enabled=False):
            gx, gw, gb = torch.ops.aten.convolution_backward(gy.contiguous(), x, weight, [weight.shape[0]] if has_bias else None, stride, padding,
                                                             (1, 1), False, (0, 0), groups,
                                                             (ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]))
        return gx, gw, gb, None, None, None


def eligible_depthwise(conv, x):
    return (trains("depthwise", x) and type(conv) is nn.Conv2d and conv.groups > 1 and conv.groups == conv.in_channels == conv.out_channels
            and conv.dilation == (1, 1) and conv.padding_mode == "zeros" and (x.requires_grad or conv.weight.requires_grad))


def eligible_1x1(conv, x):
    # only for tensors that ARE channels-last already: an NCHW pipeline keeps torch's convolution (and its memory format)
    return (trains("conv1x1", x) and _plain_conv(conv, 1) and x.shape[2] * x.shape[3] > 1 and (x.requires_grad or conv.weight.requires_grad))


def conv2d(conv, x):
    """conv(x) with the training-time 3x3 layers routed through `_Wino43Conv` and the 1x1 layers through a plain GEMM on the
    (pixels, channels) view of the channels-last tensor (forward, data and weight gradient are then three rocBLAS GEMMs under
    torch's own autograd; MIOpen's channels-last choices for 1x1 layers cost 24 ms forward and one 59 ms weight-gradient launch
    per step: profiles/r03_train_step_kernels_before.md).  Every other case is the module itself."""
    if eligible(conv, x):
        return _Wino43Conv.apply(x, conv.weight, conv.bias)
    if eligible_depthwise(conv, x):
        return _DepthwiseNative.apply(x.contiguous(), conv.weight, conv.bias, conv.stride, conv.padding, conv.groups)
    if eligible_1x1(conv, x):
        if switch("CONV1X1") != "0" and gemm_layer_ok(x.shape[0], x.shape[2], x.shape[3], conv.in_channels, conv.out_channels):
            return _Conv1x1.apply(x, conv.weight, conv.bias)
        xn = _nhwc(x)
        N, H, W, C = xn.shape
        y = torch.nn.functional.linear(xn.reshape(N * H * W, C), conv.weight.view(conv.out_channels, C), conv.bias)
        return y.view(N, H, W, conv.out_channels).permute(0, 3, 1, 2)   # channels-last in, channels-last out
    return conv(x)


class _Conv1x1(torch.autograd.Function):
    """A bias-carrying 1x1 convolution without a BatchNorm behind it (the image FPN's lateral convolutions) on the library's GEMMs in all
    three directions: forward and data gradient on `srf_conv1x1_nhwc` (the split GEMM from 128 tiles up), the weight gradient on
    `srf_conv_wgrad_nhwc` (deterministic; as torch's `linear` it was one rocBLAS TN GEMM over 1.1 M pixels at 62 TFLOP/s)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xn = _nhwc(x)
        ctx.lm = lm = _layer_mode(1, xn, weight.shape[0])
        yn = _layer_fwd(xn, weight.detach(), None, None if bias is None else bias.detach(), False, bf16=lm.bf16)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return yn.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gn = _nhwc(gy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _layer_dgrad(gn, weight.detach(), ctx.lm).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            gw = _weight_grad_in(ctx.lm, gn, _nhwc(x), weight, 1)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gn.sum(dim=(0, 1, 2))
        return gx, gw, gb


def bn_eval(bn, y):
    """BatchNorm2d in eval mode under autograd (`norm_eval=True`: vovnet.py:371) as the affine map it is, y * s + t with
    s = gamma / sqrt(var + eps), t = beta - mean * s: the gradients of gamma and beta come out of two column sums instead of
    torch's channels-last batch-norm backward (0.36 ms per layer, 26 ms per step).  Anything else: the module."""
    if trains("bn_eval", y) and derived.foldable_bn(bn, nn.BatchNorm2d):
        s = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        t = bn.bias - bn.running_mean * s
        return y * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    return bn(bn_train_input(bn, y))


def bn_train_input(bn, y):
    """What a BatchNorm in TRAINING mode may be handed.  MIOpen's training batch-norm dies with a host segmentation fault on a
    channels-last tensor of batch size 1 with a 23 x 23 map -- (1, 128, 23, 23) with strides (67712, 1, 2944, 128), also (1, 64, 23, 23),
    forward alone included; 24 x 24 and 46 x 46 at batch size 1, the same tensor at batch size 2, the same shape NCHW-contiguous and eval
    mode are all fine (tools/bn_channels_last_probe.py, every case in its own process; profiles/r04_bn_channels_last_probe.txt).  That was the round-3 crash: a bs = 1 LiDAR-only training step whose BEV FPN extras
    (stride-2 Conv2d -> BatchNorm2d in train mode) received channels-last tensors from `_Wino43Conv`.  Guarded here, at the one
    place every module-path BatchNorm goes through: a non-contiguous 4-D GPU tensor is made NCHW-contiguous before a train-mode
    BatchNorm sees it (any batch size: the trigger is a library bug, not something to steer around case by case).  Eval-mode
    BatchNorms (the camera branch's `norm_eval=True`) never get here with a copy."""
    if (isinstance(bn, nn.modules.batchnorm._BatchNorm) and bn.training and y.is_cuda and y.dim() == 4 and not y.is_contiguous()):
        return y.contiguous()
    return y
