"""Channels-last (NHWC) inference of the camera branch on the hand-written kernels of csrc/conv.hip and csrc/nhwc.hip:
VoVNet (vovnet.py:269-374) or a bottleneck ResNet (mmdet `ResNet`, compat/resnet.py) -> FPN (configs/nus/srfdet_voxel_nusc_LC.py:55-64)
-> `img_convs` (srfdet_head.py:404-416).

The torch modules stay the owners of the parameters (state_dict names untouched); this file only EXECUTES them:

* every 3x3 / stride 1 convolution ("conv3x3") runs on `srf_wino3x3` (Winograd F(2x2, 3x3) on the f32 MFMA) with the eval BatchNorm
  (or the bias) and the ReLU as its epilogue;
* an OSA block owns ONE pixel-major buffer of Cin + 5 w channels: the block input sits in slice 0, each 3x3 branch ("layer") writes
  its slice, and the 1x1 `concat` convolution ("concat", `srf_conv1x1_nhwc`) reads the buffer as a plain matrix -- the
  torch.cat of vovnet.py:222 is never built;
* eSE ("ese"): pixel mean (epilogue of the concat convolution, `srf_conv1x1_nhwc_pooled`) -> fc + hard sigmoid (`srf_ese_gate`) -> gate multiply + identity add in one pass
  that writes straight into slice 0 of the next block's buffer (`srf_nhwc_affine`), as the stage's "pool" or a "copy" does for its first block;
* the stride-2 stem layers: stem_1 (3 -> 64, "stem") is a streaming kernel from the NCHW images to channels-last
  (`srf_stem_conv_nchw`), stem_3 ("strided") an implicit-im2col GEMM (`srf_conv_gemm_nhwc`); nothing of the branch runs on MIOpen.
* a bottleneck ResNet (`resnet_plan`): the 7x7 / stride 2 stem from the NCHW images ("stem7", `srf_stem_conv7_nchw`), the padded max pool
  ("pool_p1", `srf_nhwc_maxpool3s2_pad1`), then per bottleneck "conv1" (1x1 GEMM; `srf_conv_gemm_nhwc` where a caffe-style block strides
  it), "conv2" (Winograd at stride 1, `srf_conv_gemm_nhwc` at stride 2) or "dcn" (`conv_offset` on `srf_conv_gemm_nhwc`, then
  `srf_dcnv2_nhwc` on the NHWC tensors: no transposing copy), "down" (the downsample branch, affine only) and "conv3": the 1x1 GEMM
  whose epilogue folds bn3, adds the identity and applies the ReLU (`srf_conv1x1_nhwc_residual`).  f32 only: no bf16-product mode,
  no frozen-prefix training route, no BasicBlock nets.
A network is walked ONCE per call into these steps (`Step`; the quoted names are its kinds): the gate is "a plan exists and its shapes
fit", the forward runs that plan.  Nothing is kept between calls: `_foldable` depends on each BatchNorm's mode.

Opt-in, off by default: inside `mfma_dtype(torch.bfloat16)` (`SRFDet.img_mfma_dtype`) the GEMM-shaped layers of VoVNet and the FPN run
on the bf16-product kernels of csrc/gemm_bf16.hip instead (f32 tensors, operands rounded to bf16 once, f32 accumulation and epilogue).

Tensors handed to the rest of the model are logical NCHW views with channels_last strides, so every consumer that only
looks at shapes keeps working and the RoI gather finds its channels-last operand without a copy.
Taken only for fp32 CUDA inference with BatchNorm in eval mode (`dense.fusable` / `dense._foldable`); anything else goes
through the modules as written.
"""
import os
from collections import OrderedDict, namedtuple

import torch
from torch import nn

from . import derived, mfma_mode, ops
from .dense import _foldable, fusable

_SWITCHES = {"IMG_NHWC": "1", "WINO43": "1", "FPN_FORK": "2"}   # this file's switches, SRF_<name> in the environment, read at every call: name -> default


def switch(name):
    return os.environ.get("SRF_" + name, _SWITCHES[name])   # KeyError: not a switch of this file


def enabled():
    """SRF_IMG_NHWC=0 sends the camera branch through torch / MIOpen as in round 1 (A/B switch for tests and benchmarks)."""
    return switch("IMG_NHWC") != "0"


def takes(x=None, channels_last=False):
    """This tensor goes to the channels-last executor: the switch is on and x is an fp32 CUDA tensor outside autograd and autocast
    (`dense.fusable`), with channels-last strides when that is asked.  x=None: the switch alone (`SRFDetHead.img_level_consumer`)."""
    return enabled() and (x is None or (fusable(x) and (not channels_last or is_channels_last(x))))


def nhwc_view(x):
    """Logical (N, C, H, W) tensor with channels_last strides -> its (N, H, W, C) view."""
    return x.permute(0, 2, 3, 1)


def nchw_view(x):
    return x.permute(0, 3, 1, 2)


def is_channels_last(x):
    return x.dim() == 4 and x.stride(1) == 1 and x.shape[1] > 1


# kind -> the name of that operand's pack call in `ops` (looked up at the call); the packed images are held by `derived` under the kind's name
_PACK = {"wino": "pack_wino3x3_weights", "wino43": "pack_wino43_weights", "gemm": "pack_conv1x1_nhwc_weights",
         "gemm_direct": "pack_conv1x1_nhwc_direct_weights", "gemm_split": "pack_conv1x1_nhwc_split_weights",
         "gemm_bf16": "pack_conv1x1_nhwc_bf16_weights", "cgemm": "pack_conv_gemm_weights", "cgemm_split": "pack_conv_gemm_split_weights",
         "cgemm_bf16": "pack_conv_gemm_bf16_weights"}


def packed(conv, kind):
    """The `kind` operand of conv.weight, packed once and kept until the weight changes."""
    return derived.get(conv, kind, (conv.weight,), lambda: getattr(ops, _PACK[kind])(conv.weight.detach()))


def invalidate_caches(model):
    """Drops everything derived from the parameters and buffers of `model`'s modules (packed operands, BatchNorm folds, padded
    weights: derived.py).  Needed after an update the version counters cannot see, `p.data.mul_()` or old-style EMA; the detector
    calls it from `train()`, after `load_state_dict` and from `weights_changed()`, which also drops the graphs captured over these
    tensors -- on a model with live graphs call that, not this."""
    derived.invalidate(model)


# ---- the bf16-product mode of the image branch (csrc/gemm_bf16.hip) ------------------------------------------------------------
class mfma_dtype(mfma_mode.MfmaMode):
    """Within `with nhwc.mfma_dtype(torch.bfloat16):` the layers executed by `conv3x3`, `conv1x1` (plain, pool=, top=) and
    `conv_strided` -- so `vovnet_forward` and `fpn_forward` -- run on the bf16-product kernels: f32 tensors, both operands rounded to
    bf16 once, exact products, f32 accumulation and epilogue (`srf_conv1x1_nhwc_bf16*`; `srf_conv_gemm_nhwc_bf16` for every 3x3 layer,
    stride 1 included -- no Winograd in this mode: products of bf16-rounded transformed data are another, worse arithmetic).  Off by
    default; `mfma_dtype(None)` inside an active context switches it off again (the head's `img_convs` inside the neck's chains).

    A layer the family cannot take keeps its f32 route: input channels that are no multiple of 32 (VoVNet stem_1 with 3 input
    channels, which `srf_stem_conv_nchw` runs anyway), an operand that is not 16-byte aligned or whose pitch is no multiple of 4,
    tensors beyond the family's 32-bit ranges (one 128-row tile of x or y, one image of a conv layer's input, from 2^31 bytes).

    routes: a list that receives one dict(layer=, route="bf16" | "f32", why=) per executed layer -- the per-layer report, as
    bench.py's config.gemm_route is for the split rule.  `launches` counts the layers that ran on the bf16 kernels.  The switch is
    process-wide while the context is open (the executor is single-threaded); it is not an environment variable and nothing outside
    the context sees it."""


def mfma_active():
    return mfma_dtype.active() is not None


def _bf16_route(x, conv, out, form):
    """True when the active mode takes this layer; records the route.  form: "1x1" or "conv"."""
    m = mfma_dtype.active()
    if m is None:
        return False
    N, H, W, cin = x.shape
    k, st = conv.kernel_size[0], conv.stride[0]
    return m.report(f"{cin}->{conv.out_channels} {k}x{k}/s{st} @{N}x{H}x{W}", ops.gemm_bf16_why_not(x, conv.out_channels, out, im2col=form == "conv"))


def _is_conv(conv, k, stride=1):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (k, k) and conv.stride == (stride, stride)
            and conv.padding == (k // 2, k // 2) and conv.dilation == (1, 1) and conv.groups == 1)


def _affine_of(conv, bn):
    """(scale, shift) of the layer's epilogue: folded eval BatchNorm (and bias), or the bias alone."""
    if bn is not None:
        scale, shift = derived.fold_bn(bn)
        if conv.bias is not None:
            shift = shift + conv.bias * scale
        return scale, shift
    return None, conv.bias


def wino43_enabled():
    """SRF_WINO43=0 keeps every 3x3 layer on Winograd F(2x2, 3x3) (A/B switch for tests and benchmarks)."""
    return switch("WINO43") != "0"


def use_wino43(x, cout, out=None):
    """F(4x4, 3x3) (`srf_wino43`: direct FLOPs / 4, plus an HBM pass that writes the transformed input) where it is the faster
    of the two kernels: every layer from 96 input channels up.  Below that (VoVNet stem_2: 64 -> 64 on 464 x 800) the
    transform pass costs more than the saved MFMA time (tools/micro/wino43_bench.hip: 954 against 928 us)."""
    return wino43_enabled() and x.shape[3] >= 96 and ops.wino43_supported(x, cout, out)


def conv3x3(x, conv, bn=None, relu=False, out=None):
    """x: NHWC slice; conv: nn.Conv2d 3x3 / stride 1 / padding 1."""
    scale, shift = _affine_of(conv, bn)
    if _bf16_route(x, conv, out, "conv"):
        return ops.conv_gemm_nhwc(x, None, conv.out_channels, (3, 3), 1, 1, scale, shift, relu, out=out,
                                  packed_bf16=lambda: packed(conv, "cgemm_bf16"))
    if use_wino43(x, conv.out_channels, out):
        return ops.wino43(x, packed(conv, "wino43"), conv.out_channels, scale, shift, relu, out=out)
    return ops.wino3x3(x, packed(conv, "wino"), conv.out_channels, scale, shift, relu, out=out)


def conv1x1(x, conv, bn=None, relu=False, out=None, pool=False, top=None):
    scale, shift = _affine_of(conv, bn)
    # the operand orders are packed lazily: a layer only ever packs the one its launch selects
    return ops.conv1x1_nhwc(x, lambda: packed(conv, "gemm"), conv.out_channels, scale, shift, relu, out=out, pool=pool, top=top,
                            packed_direct=lambda: packed(conv, "gemm_direct"), packed_split=lambda: packed(conv, "gemm_split"),
                            packed_bf16=(lambda: packed(conv, "gemm_bf16")) if _bf16_route(x, conv, out, "1x1") else None)


def conv1x1_residual(x, conv, bn, res, relu=True, out=None):
    """conv3 of a bottleneck: relu(bn(conv(x)) + res) in the GEMM's epilogue; always on the f32-accurate families."""
    scale, shift = _affine_of(conv, bn)
    return ops.conv1x1_nhwc_residual(x, lambda: packed(conv, "gemm"), conv.out_channels, res, scale, shift, relu, out=out,
                                     packed_direct=lambda: packed(conv, "gemm_direct"), packed_split=lambda: packed(conv, "gemm_split"))


def wino_ok(conv, cin):
    return _is_conv(conv, 3) and ops.wino3x3_channels_ok(cin)


def _img_fits(H, W, ld):
    """One image of an (N, H, W, ld) f32 buffer inside the per-image range of srf_wino3x3 (`ops.wino3x3_range_ok`).  The gates hold
    EVERY buffer a 3x3 layer reads to this bound, also where the layer runs on srf_wino43, whose own range is wider: deliberately --
    which of the two kernels a layer takes is a switch and a threshold (`use_wino43`), the gate's verdict is neither."""
    return ops.wino3x3_range_ok(H * W, ld)


def strided_ok(conv, cin):
    return (isinstance(conv, nn.Conv2d) and conv.groups == 1 and conv.dilation == (1, 1) and conv.stride[0] == conv.stride[1]
            and conv.padding[0] == conv.padding[1] and ops.gemm_k_ok(cin))


def conv_strided(x, conv, bn=None, relu=False, out=None):
    """A convolution the Winograd kernel does not cover (stride 2) as an implicit-im2col GEMM on the f32 MFMA
    (`srf_conv_gemm_nhwc`): deterministic, where MIOpen's channels-last choice is an atomic split-K kernel."""
    scale, shift = _affine_of(conv, bn)
    return ops.conv_gemm_nhwc(x, lambda: packed(conv, "cgemm"), conv.out_channels, conv.kernel_size, conv.stride[0], conv.padding[0],
                              scale, shift, relu, out=out, packed_split=lambda: packed(conv, "cgemm_split"),
                              packed_bf16=(lambda: packed(conv, "cgemm_bf16")) if _bf16_route(x, conv, out, "conv") else None)


# One step of a plan.  kind: a quoted name at the head of the file, "lateral" (FPN), "out"; arg: "ese" adds the block's input, an FPN step ends in a ReLU, the name of an "out",
# a ResNet "conv3" adds the downsample branch
Step = namedtuple("Step", "kind conv bn arg", defaults=(None, None, None))
Slot = namedtuple("Slot", "H W width lo hi")     # a step writes channels [lo, hi) of an (N, H, W, width) buffer


def _cbr(mods):
    """(conv, bn) of a [conv, bn, relu] triple (an nn.Sequential built by vovnet._cbr, or three modules); None if it has another form."""
    mods = list(mods.children()) if isinstance(mods, nn.Module) else mods
    ok = len(mods) == 3 and isinstance(mods[0], nn.Conv2d) and _foldable(mods[1]) and isinstance(mods[2], nn.ReLU)
    return (mods[0], mods[1]) if ok else None


# ---- VoVNet ----------------------------------------------------------------------------------------------------------
def vovnet_plan(net):
    """The steps of VoVNet.forward, or None when the net has another structure than stem_1 .. stem_3 and stages of [pool,] plain OSA
    blocks whose layers the kernels take."""
    from .plugin.vovnet import OSAModule
    stem = list(net.stem.children())
    cbr = [_cbr(stem[i:i + 3]) for i in (0, 3, 6)]
    if len(stem) != 9 or None in cbr:
        return None
    (c0, b0), (c3, b3), (c6, b6) = cbr
    if not (c0.kernel_size == (3, 3) and c0.stride == (2, 2) and c0.padding == (1, 1) and c0.groups == 1
            and ops.stem_channels_ok(c0.in_channels, c0.out_channels) and wino_ok(c3, c3.in_channels) and c3.bias is None
            and _is_conv(c6, 3, 2) and ops.gemm_k_ok(c6.in_channels)):
        return None
    plan = [Step("stem", c0, b0), Step("conv3x3", c3, b3), Step("strided", c6, b6)]
    if "stem" in net._out_features:
        plan.append(Step("out", arg="stem"))
    for name in net.stage_names:
        blocks = list(getattr(net, name).children())
        if blocks and isinstance(blocks[0], nn.MaxPool2d):
            m = blocks.pop(0)
            if not (m.kernel_size == 3 and m.stride == 2 and m.padding == 0 and m.ceil_mode and m.dilation == 1):
                return None
            plan.append(Step("pool"))
        elif plan[-1].kind == "out":
            plan.append(Step("copy"))     # a finished tensor enters the block's buffer
        if not blocks or not all(isinstance(m, OSAModule) and m.reduce is None and len(m.layers) for m in blocks):
            return None
        for m in blocks:
            layers, cc = [_cbr(layer) for layer in m.layers], _cbr(m.concat)
            if (cc is None or None in layers or not all(wino_ok(c, c.in_channels) for c, _ in layers)
                    or not (_is_conv(cc[0], 1) and ops.gemm_k_ok(cc[0].in_channels) and ops.ese_channels_ok(cc[0].out_channels))):
                return None
            plan += [Step("layer", c, b) for c, b in layers] + [Step("concat", *cc), Step("ese", m.ese.fc, None, m.identity)]
        plan.append(Step("out", arg=name))
    return plan


def plan_shapes(plan, H, W):
    """Carries an (H, W) image through a VoVNet plan: every step with the Slot it writes, or None when a buffer that a 3x3 layer reads
    does not fit (`_img_fits`).  The one place where the size after a stride or a pool and the width of an OSA block's buffer are computed:
    every step but a block's "layer" opens a buffer, as wide as its own output plus the outputs of the layers that directly follow."""
    slots = []
    for i, s in enumerate(plan):
        last = slots[-1] if slots else None
        if s.kind == "out":
            slots.append(last)
        elif s.kind == "layer":
            slots.append(Slot(last.H, last.W, last.width, last.hi, last.hi + s.conv.out_channels))
        else:
            if s.kind in ("stem", "strided"):
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1       # 3x3, stride 2, padding 1
            elif s.kind == "pool":
                H, W = ops.pool3s2_out(H), ops.pool3s2_out(W)
            c = s.conv.out_channels if s.conv is not None else last.hi - last.lo
            n = next(j for j, t in enumerate(plan[i + 1:]) if t.kind != "layer")       # an OSA block's layers follow directly
            width = c + sum(t.conv.out_channels for t in plan[i + 1:i + 1 + n])
            if plan[i + 1].kind in ("conv3x3", "layer") and not _img_fits(H, W, width):
                return None
            slots.append(Slot(H, W, width, 0, c))
    return list(zip(plan, slots))


def _vovnet_steps(net, x):
    plan = vovnet_plan(net) if x.dim() == 4 else None
    return plan and plan_shapes(plan, x.shape[2], x.shape[3])


def vovnet_forward(net, x, upto=None, steps=None):
    """x (N, 3, H, W) f32 -> OrderedDict of the requested stage outputs (logical NCHW, channels_last strides).  upto = a stage name: stop after
    that stage and return (outputs so far, that stage's NHWC output) -- the frozen prefix of the backbone during training (`VoVNet.forward`)."""
    steps = steps or _vovnet_steps(net, x)
    if not steps:
        raise ValueError("nhwc.vovnet_forward: not a network or a shape the executor runs (vovnet_supported)")
    out = OrderedDict()
    buf = y = cin = t = mean = None       # the buffer being filled and the block input's width; what the last step wrote
    for s, slot in steps:
        alone = slot.width == slot.hi     # the step owns its tensor
        if s.kind == "stem":              # BatchNorm + ReLU in the same kernel
            y = ops.stem_conv_nchw(x.contiguous(), s.conv.weight, *_affine_of(s.conv, s.bn), True)
        elif s.kind == "conv3x3" or (s.kind == "strided" and alone):
            y = (conv3x3 if s.kind == "conv3x3" else conv_strided)(y, s.conv, s.bn, True)
        elif s.kind == "layer":
            y = conv3x3(y, s.conv, s.bn, True, out=buf[..., slot.lo:slot.hi])
        elif s.kind == "concat":
            t, mean = conv1x1(buf, s.conv, s.bn, True, pool=True)     # eSE average pool from the convolution's own epilogue
        elif s.kind == "out":
            if s.arg in net._out_features:
                out[s.arg] = nchw_view(y)
            if upto is not None and s.arg == upto:
                return out, y
        else:                             # into slice 0 of the buffer the next block fills: the torch.cat of vovnet.py:222 is never built
            new = torch.empty((x.shape[0], slot.H, slot.W, slot.width), dtype=torch.float32, device=x.device)
            dst = new if alone else new[..., :slot.hi]
            if s.kind == "strided":
                conv_strided(y, s.conv, s.bn, True, out=dst)
            elif s.kind == "pool":
                ops.nhwc_maxpool3s2_ceil(y, out=dst)
            elif s.kind == "copy":
                dst.copy_(y)
            else:                         # eSE: gate * concat (+ the block's input)
                gate = ops.ese_gate(mean, s.conv.weight, s.conv.bias)
                ops.nhwc_affine(t, scale=gate, residual=buf[..., :cin] if s.arg else None, out=dst)
            buf, y, cin = new, dst, slot.hi
    return out


def vovnet_supported(net, x):
    return fusable(x) and bool(_vovnet_steps(net, x))


def vovnet(net, x, upto=None):
    """`vovnet_forward` when the executor takes the call, else None: one plan for the verdict and the run."""
    steps = _vovnet_steps(net, x) if takes(x) else None
    return vovnet_forward(net, x, upto, steps) if steps else None


# ---- ResNet (bottleneck) ---------------------------------------------------------------------------------------------
def _pointwise_ok(conv):
    """A bias-free 1x1 convolution at stride 1 (the GEMM) or 2 (`conv_strided`) whose input the GEMM families read."""
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.padding == (0, 0) and conv.stride in ((1, 1), (2, 2))
            and conv.bias is None and strided_ok(conv, conv.in_channels))


def _dcn_ok(m):
    """A DCNv2 pack `srf_dcnv2_nhwc` runs from NHWC tensors with `conv_offset` on srf_conv_gemm_nhwc: 3x3, padding 1, no dilation, no bias."""
    co = m.conv_offset
    return (ops.dcn_enabled() and m.kernel_size == (3, 3) and m.padding == 1 and m.dilation == 1 and m.stride in (1, 2) and m.bias is None
            and ops.dcnv2_supported(1, m.in_channels, 2, 2, m.groups, m.deform_groups) and ops.gemm_k_ok(m.in_channels)
            and co.kernel_size == (3, 3) and co.stride == (m.stride, m.stride) and co.padding == (1, 1) and strided_ok(co, co.in_channels))


def resnet_plan(net):
    """The steps of compat.resnet.ResNet.forward for a net of `_Bottleneck` blocks, or None: BasicBlock nets, a BatchNorm that is not
    foldable, a bias where the module has none, channel counts the kernels refuse, a DCN with dilation (or any DCN with SRF_DCN=0)."""
    from .compat.dcn import ModulatedDeformConv2dPack
    from .compat.resnet import _Bottleneck
    c, m = net.conv1, net.maxpool
    if not (isinstance(c, nn.Conv2d) and c.kernel_size == (7, 7) and c.stride == (2, 2) and c.padding == (3, 3) and c.dilation == (1, 1)
            and c.groups == 1 and c.bias is None and _foldable(net.bn1) and isinstance(net.relu, nn.ReLU)
            and ops.stem7_channels_ok(c.in_channels, c.out_channels)
            and isinstance(m, nn.MaxPool2d) and m.kernel_size == 3 and m.stride == 2 and m.padding == 1 and not m.ceil_mode and m.dilation == 1):
        return None
    plan = [Step("stem7", c, net.bn1), Step("pool_p1")]
    for i, name in enumerate(net.res_layers):
        for blk in getattr(net, name):
            if not (isinstance(blk, _Bottleneck) and all(_foldable(bn) for bn in (blk.bn1, blk.bn2, blk.bn3)) and _pointwise_ok(blk.conv1)
                    and _pointwise_ok(blk.conv3) and blk.conv3.stride == (1, 1) and ops.quads_ok(blk.conv3.out_channels)):
                return None
            c2 = blk.conv2
            if isinstance(c2, ModulatedDeformConv2dPack):
                kind = "dcn" if _dcn_ok(c2) else None
            else:
                kind = "conv2" if c2.bias is None and (wino_ok(c2, c2.in_channels) or (_is_conv(c2, 3, 2) and ops.gemm_k_ok(c2.in_channels))) else None
            if kind is None:
                return None
            plan += [Step("conv1", blk.conv1, blk.bn1), Step(kind, c2, blk.bn2)]
            if blk.downsample is not None:
                down = list(blk.downsample.children())
                if not (len(down) == 2 and _pointwise_ok(down[0]) and _foldable(down[1])):
                    return None
                plan.append(Step("down", *down))
            plan.append(Step("conv3", blk.conv3, blk.bn3, blk.downsample is not None))     # arg: the identity is the downsample's output
        plan.append(Step("out", arg=i))
    return plan


def resnet_shapes(plan, H, W, N=1):
    """Carries an (H, W) image through a ResNet plan: every step with the Slot it writes (each step owns its tensor), or None when the
    stem's output of one image leaves its descriptor (`ops.stem7_range_ok`), a buffer a 3x3 layer reads does not fit (`_img_fits`), an input of
    srf_conv_gemm_nhwc (one image) or of srf_dcnv2_nhwc (the batch of N) reaches 2 GiB, or a DCN would read a map of fewer than 2 rows or
    columns."""
    slots, blk = [], None      # blk: (H, W) of the running block's input
    half = lambda h, s: (h - 1) // s + 1      # noqa: E731  7x7 / padding 3, 3x3 / padding 1, 1x1 / padding 0: one formula
    for s in plan:
        cin = s.conv.in_channels if s.conv is not None else None
        if s.kind == "out":
            slots.append(slots[-1])
            continue
        if s.kind == "pool_p1":
            H, W = ops.pool3s2p1_out(H), ops.pool3s2p1_out(W)
            slots.append(Slot(H, W, slots[-1].width, 0, slots[-1].hi))
            continue
        if s.kind == "conv1":
            blk = (H, W)
        src = blk if s.kind == "down" else (H, W)
        st = s.conv.stride if isinstance(s.conv.stride, int) else s.conv.stride[0]
        if s.kind == "stem7":
            st = 2
            if not ops.stem7_range_ok(half(H, 2) * half(W, 2), s.conv.out_channels):
                return None
        elif s.kind == "dcn":
            if not ops.dcnv2_supported(N, cin, *src, s.conv.groups, s.conv.deform_groups):
                return None
        elif s.conv.kernel_size == (3, 3) and not _img_fits(*src, cin):
            return None
        if s.kind in ("dcn", "conv2", "conv1", "down") and st != 1 and not ops.below_2gb(src[0] * src[1], cin):
            return None
        if s.kind == "dcn" and not ops.below_2gb(src[0] * src[1], cin):      # conv_offset reads the same input through srf_conv_gemm_nhwc
            return None
        out = (half(src[0], st), half(src[1], st))
        if s.kind != "down":
            H, W = out
        c = s.conv.out_channels
        slots.append(Slot(*out, c, 0, c))
    return list(zip(plan, slots))


def _resnet_steps(net, x):
    plan = resnet_plan(net) if x.dim() == 4 and x.shape[1] == net.conv1.in_channels else None
    return plan and resnet_shapes(plan, x.shape[2], x.shape[3], x.shape[0])


def _dcn(x, m, bn, relu):
    """DCNv2 on NHWC tensors, bn + ReLU as the epilogue: `forward_hip` of compat/dcn.py without its two transposing copies (the same
    `dcn` / `dcn_offset` entries of `derived`)."""
    scale, shift = derived.fold_bn(bn)
    KG = 9 * m.deform_groups
    co = m.conv_offset
    om = ops.conv_gemm_nhwc(x, m._packed("dcn_offset", co.weight), 3 * KG, (3, 3), m.stride, m.padding, None,
                            None if co.bias is None else co.bias.detach())
    return ops.dcnv2_nhwc(x, om[..., :2 * KG], om[..., 2 * KG:], m._packed("dcn", m.weight), m.out_channels, (3, 3), m.stride, m.padding,
                          m.dilation, m.deform_groups, True, scale, shift, relu)


def resnet_forward(net, x, steps=None):
    """x (N, Cin, H, W) f32 -> the tuple of stage outputs `ResNet.forward` returns (logical NCHW, channels_last strides).  Always on
    the f32 routes: there is no bf16-product residual form, so an active `mfma_dtype` is switched off for the walk."""
    steps = steps or _resnet_steps(net, x)
    if not steps:
        raise ValueError("nhwc.resnet_forward: not a network or a shape the executor runs (resnet_supported)")
    outs = []
    y = xin = idt = None        # what the last step wrote; the running block's input and its downsample branch
    with mfma_dtype(None):
        for s, _ in steps:
            if s.kind == "stem7":         # BatchNorm + ReLU in the same kernel
                y = ops.stem_conv7_nchw(x.contiguous(), s.conv.weight, *_affine_of(s.conv, s.bn), True)
            elif s.kind == "pool_p1":
                y = ops.nhwc_maxpool3s2_pad1(y)
            elif s.kind == "conv1":
                xin = y
                y = (conv1x1 if s.conv.stride == (1, 1) else conv_strided)(y, s.conv, s.bn, True)
            elif s.kind == "conv2":
                y = (conv3x3 if s.conv.stride == (1, 1) else conv_strided)(y, s.conv, s.bn, True)
            elif s.kind == "dcn":
                y = _dcn(y, s.conv, s.bn, True)
            elif s.kind == "down":
                idt = (conv1x1 if s.conv.stride == (1, 1) else conv_strided)(xin, s.conv, s.bn, False)
            elif s.kind == "conv3":
                y = conv1x1_residual(y, s.conv, s.bn, idt if s.arg else xin, True)
            elif s.arg in net.out_indices:      # "out"
                outs.append(nchw_view(y))
    return tuple(outs)


def resnet_supported(net, x):
    return fusable(x) and bool(_resnet_steps(net, x))


def resnet(net, x):
    """`resnet_forward` when the executor takes the call, else None: one plan for the verdict and the run."""
    steps = _resnet_steps(net, x) if takes(x) else None
    return resnet_forward(net, x, steps) if steps else None


# ---- SECONDCustom ----------------------------------------------------------------------------------------------------
def second_plan(net):
    """The steps of SECONDCustom.forward (second_custom.py:78-91): 3x3 / stride 1 layers on the Winograd kernels, the strided heads of
    the blocks on srf_conv_gemm_nhwc; None when a stage is no chain of conv -> eval BatchNorm -> ReLU the kernels take."""
    plan = []
    for stage in net.blocks:
        mods = list(stage.children())
        for j in range(0, len(mods), 3):
            cb = _cbr(mods[j:j + 3])
            kind = cb and ("conv3x3" if wino_ok(cb[0], cb[0].in_channels) else "strided" if cb[0].stride != (1, 1) and cb[0].kernel_size == (3, 3)
                           and cb[0].padding == (1, 1) and strided_ok(cb[0], cb[0].in_channels) else None)
            if not kind:
                return None
            plan.append(Step(kind, *cb))
        plan.append(Step("out"))
    return plan


def _second_steps(net, x):
    """The widest layer is held to `_img_fits` at the INPUT's size, the strides not followed: on the safe side, as the gate held it."""
    plan = second_plan(net) if x.dim() == 4 and ops.wino3x3_channels_ok(x.shape[1]) else None
    widest = plan and max([x.shape[1]] + [s.conv.out_channels for s in plan if s.conv is not None])
    return plan if plan and _img_fits(x.shape[2], x.shape[3], widest) else None


def second_forward(net, x, plan=None):
    plan = plan or _second_steps(net, x)
    if not plan:
        raise ValueError("nhwc.second_forward: not a network or a shape the executor runs (second_supported)")
    y = nhwc_view(x if is_channels_last(x) else ops.to_channels_last(x))
    outs = []
    for s in plan:
        if s.kind == "out":
            outs.append(nchw_view(y))
        else:
            y = (conv3x3 if s.kind == "conv3x3" else conv_strided)(y, s.conv, s.bn, True)
    return tuple(outs)


def second_supported(net, x):
    return fusable(x) and bool(_second_steps(net, x))


def second(net, x):
    """`second_forward` when the executor takes the call, else None."""
    plan = _second_steps(net, x) if takes(x) else None
    return second_forward(net, x, plan) if plan else None


# ---- FPN -------------------------------------------------------------------------------------------------------------
def fpn_plan(fpn, n_inputs):
    """The layers `fpn_forward` runs for `n_inputs` levels -- laterals (1x1 GEMM, top-down add in the epilogue), output convolutions
    (3x3 Winograd), extra stride-2 convolutions on the last output (srf_conv_gemm_nhwc) -- or None when the neck is another one."""
    n = len(fpn.lateral_convs)
    if (fpn.start_level != 0 or fpn.backbone_end_level != fpn.num_ins or n_inputs != n
            or (fpn.num_outs != n and not (fpn.num_outs > n and fpn.add_extra_convs == "on_output"))
            or fpn.upsample_cfg.get("mode", "nearest") != "nearest" or len(fpn.upsample_cfg) != 1):
        return None
    takes_it = dict(lateral=lambda c: _is_conv(c, 1) and ops.gemm_k_ok(c.in_channels) and ops.quads_ok(c.out_channels),
                    conv3x3=lambda c: wino_ok(c, c.in_channels), strided=lambda c: strided_ok(c, c.in_channels))
    plan = []
    for kind, cm in zip(["lateral"] * n + ["conv3x3"] * n + ["strided"] * (len(fpn.fpn_convs) - n), [*fpn.lateral_convs, *fpn.fpn_convs]):
        bn = getattr(cm, cm.norm_name) if cm.with_norm else None
        if ((cm.with_norm and not _foldable(bn)) or (cm.with_activation and not isinstance(cm.activate, nn.ReLU))
                or not takes_it[kind](cm.conv)):
            return None
        plan.append(Step(kind, cm.conv, bn, cm.with_activation))
    return plan


def fpn_supported(fpn, inputs):
    plan = fpn_plan(fpn, len(inputs))
    if plan is None or not all(fusable(x) and is_channels_last(x) for x in inputs):
        return False
    for x, lat in zip(inputs, plan):
        try:   # a channels-last view that is not a channel slice of a pixel-major buffer (or too large) goes to the module path
            ld = ops.nhwc_ld(nhwc_view(x))
        except RuntimeError:
            return False
        if not (ops.operand_ok(ld, x.data_ptr()) and _img_fits(x.shape[2], x.shape[3], max(ld, lat.conv.out_channels))):
            return False
    return True


def fpn(neck, inputs):
    """`fpn_forward` when the executor takes the call, else None (the forward reads the modules itself: the plan is built once)."""
    return fpn_forward(neck, inputs) if takes() and fpn_supported(neck, inputs) else None


def _cm(cm, x, fn):
    bn = getattr(cm, cm.norm_name) if cm.with_norm else None
    return fn(x, cm.conv, bn, cm.with_activation)


class ConsumedLevels(list):
    """Pyramid levels a per-level consumer (the head's `img_convs`) has already been applied to (see `level_consumer`)."""


class level_consumer:
    """Within this context the channels-last forward of THIS FPN instance hands every finished level to `fn(i, x_nhwc) ->
    y_nhwc` as part of that level's chain (lateral -> output convolution -> consumer).  graphs.GraphedImageBranch uses it to
    run the head's `img_convs` (srfdet_head.py:404-416) inside the camera graph, where the chains of the coarse levels are
    captured as parallel branches: their few-workgroup kernels (29 x 50 and 58 x 100 maps cover 65 % / 80 % of the CUs) run
    beside the lateral GEMMs and the finest level's kernels instead of after them.  The consumer is an attribute of the neck it
    is meant for (no module-global state: another FPN's forward is not affected); fn = None is a no-op context."""

    def __init__(self, fpn, fn):
        self.fpn, self.fn = fpn, fn

    def __enter__(self):
        if self.fn is not None:
            self.fpn._srf_level_consumer = self.fn
        return self

    def __exit__(self, *exc):
        if self.fn is not None:
            self.fpn._srf_level_consumer = None
        return False


_CHAIN_STREAMS = []


def _chain_stream(i):
    while len(_CHAIN_STREAMS) <= i:
        _CHAIN_STREAMS.append(torch.cuda.Stream())
    return _CHAIN_STREAMS[i]


def fpn_forward(fpn, inputs):
    # laterals from the top level down: the top-down step (`laterals[i - 1] += upsample(laterals[i])`) is the epilogue of the
    # lateral convolution of level i - 1 (srf_conv1x1_nhwc_topdown): no separate pass over the finer map
    n = len(fpn.lateral_convs)
    convs = list(fpn.fpn_convs)
    consumer = getattr(fpn, "_srf_level_consumer", None)
    if len(convs) > n:
        consumer = None   # extra levels hang off the last output: one chain
    # under a graph capture the chain of every coarse level forks off as soon as its lateral is final
    fork_from = int(switch("FPN_FORK"))   # first level whose chain forks; 0: none
    fork = consumer is not None and inputs[0].is_cuda and torch.cuda.is_current_stream_capturing() and fork_from > 0
    main = torch.cuda.current_stream() if fork else None

    def chain(i):
        o = _cm(convs[i], lats[i], conv3x3)
        if consumer is None:
            return o
        with mfma_dtype(None):     # the consumer is not part of the neck: the head's `img_convs` stay f32 in the bf16 mode
            return consumer(i, o)

    lats = [None] * n
    outs = [None] * n
    used = []
    for i in range(n - 1, -1, -1):
        cm = fpn.lateral_convs[i]
        bn = getattr(cm, cm.norm_name) if cm.with_norm else None
        lats[i] = conv1x1(nhwc_view(inputs[i]), cm.conv, bn, cm.with_activation, top=lats[i + 1] if i + 1 < n else None)
        if fork and i >= fork_from:
            s = _chain_stream(i)
            s.wait_stream(main)
            with torch.cuda.stream(s):
                outs[i] = chain(i)
            used.append(s)
    for i in range(n):
        if outs[i] is None:
            outs[i] = chain(i)
    for s in used:
        main.wait_stream(s)   # the join; `lats` and `outs` stay referenced until here, so no block is reused across streams
    for cm in convs[n:]:   # add_extra_convs='on_output': stride-2 3x3 on the previous output
        src = outs[-1]
        if fpn.relu_before_extra_convs and len(outs) > n:
            src = torch.relu(src)
        outs.append(_cm(cm, src, conv_strided))
    res = tuple(nchw_view(o) for o in outs)
    return ConsumedLevels(res) if consumer is not None else res
