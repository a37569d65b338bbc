"""spconv-shaped Python surface over the HIP rulebook / sparse-conv kernels.

Mirrors the operator boundary the reference uses: `SparseConvTensor(features, indices, spatial_shape,
batch_size)` with `.features/.indices/.dense()`, `SubMConv3d` / `SparseConv3d(in, out, kernel_size, stride, padding,
bias=False, indice_key)`, `SparseSequential`, and mmdet3d's `SparseBasicBlock` / `make_sparse_convmodule`
(reference call sites: mmdet3d_plugin/models/middle_encoders/sparse_encoder_custom.py:7-15, :73-107, :123-138,
:182-211).  Parameter names and shapes follow spconv 1.x / mmcv (`weight`: kD,kH,kW,Cin,Cout) so reference
checkpoints load by key; spconv 2.x layout (Cout,kD,kH,kW,Cin) is converted on load.

What is different from spconv, by design:
  * a SparseConvTensor is features on a `Level`, one active coordinate set, which owns its bitmap or hash table, a `Rulebook`
    (output-stationary neighbour table (K, A_out), pair counts, row plans) per SubM kernel size and, per strided conv, the rulebook
    and the Level it produces: the 16 un-keyed SubM convs of the basic blocks (rebuilt from scratch by the reference) share one;
  * in eval mode conv -> BatchNorm1d -> ReLU (and the residual add of SparseBasicBlock) run as ONE kernel.
"""
import functools
import math

import torch
from torch import nn

from . import derived, mfma_mode, ops
from .compat.cnn import build_norm_layer
from .compat.registry import CONV_LAYERS


def _triple(v):
    if isinstance(v, (list, tuple)):
        assert len(v) == 3
        return [int(x) for x in v]
    return [int(v)] * 3


# ---- the bf16-product mode of the sparse encoder (csrc/spconv_bf16.hip) --------------------------------------------------------
class mfma_dtype(mfma_mode.MfmaMode):
    """Within `with sparse.mfma_dtype(torch.bfloat16):` a `_SparseConv` of one of the five 64- / 128-output-channel shapes of
    `srf_spconv_fwd_bf16` (include/srfdet3d.h) runs on the bf16-product kernel: f32 tensors, inputs and weights rounded to bf16 once,
    exact products, f32 accumulation and the f32 epilogue (BatchNorm fold, residual, ReLU) -- defined by tests/spconv_bf16_ref.py.
    Every other layer keeps its f32 route: the 16- and 32-output-channel layers and any shape without that form, a shape that
    `ops.SPCONV_BF16_NOT_FASTER` lists, a layer in training mode or with gradients enabled.  Off by default; `mfma_dtype(None)` inside
    an active context switches it off again.

    routes: a list that receives one dict(layer=, route="bf16" | "f32", why=) per executed layer.  `launches` counts the layers that
    ran on the bf16 kernel.  Process-wide while the context is open, as `nhwc.mfma_dtype`; nothing outside the context sees it."""


def mfma_active():
    return mfma_dtype.active() is not None


class Rulebook:
    """The neighbour table `nbr` (K, A_out) of one kernel on one level, its pair counts, and the row plans its layers asked for."""

    def __init__(self, nbr, counts):
        self.nbr, self.counts, self._plans = nbr, counts, {}

    def plan(self, cin, cout, K, subm, rows_dev):
        """What a packed-weight layer passes as `tiles=`, built once per rulebook: balanced row ranges, shared by the SubM layers of a
        level (a 27-offset strided conv gains more from them than they cost: 64 -> 128 on the nuScenes encoder 92 -> 76 us; conv_out, 3
        offsets, runs on equal-height tiles); 32-channel layers: a mask-sorted row order, from ~100k rows up (Waymo's levels); or None."""
        if not (ops.spconv_tiles_wanted(cin, cout) and self.nbr.shape[1] > 0 and (subm or K == 27)):
            return None
        kind = "tiles" if cout != 32 else "order" if ops.spconv_order_wanted(cin, cout, rows=self.nbr.shape[1]) else None
        if kind is not None and kind not in self._plans:
            self._plans[kind] = getattr(ops, "spconv_" + kind)(self.nbr, rows_dev)
        return self._plans.get(kind)


class Level:
    """One active coordinate set `indices` (A, 4) int32 (b, z, y, x) and what is derived from it: its occupancy `bitmap` (ops.BitmapLevel)
    if the rows are sorted by (b, y, x, z), else a hash table built on first use; its rulebooks; the levels of its strided convs.  Static
    shapes (whole-frame hipGraph; `caps`: {indice_key of a strided conv: rows}): `indices` is padded with rows of -1 to a capacity,
    `rows_dev` is the device count of the real ones, every strided conv gives caps[indice_key] rows, nothing is read back to the host."""

    def __init__(self, indices, spatial_shape, batch_size, bitmap=None, table=None, rows_dev=None, caps=None):
        self.indices = indices if indices.dtype == torch.int32 else indices.int()
        self.spatial_shape, self.batch_size = [int(s) for s in spatial_shape], int(batch_size)
        self.bitmap, self.rows_dev, self.caps = bitmap, rows_dev, caps
        self._table, self._subm, self._strided = table, {}, {}

    @staticmethod
    def sorted(indices, spatial_shape, batch_size, static_caps=None):
        """Distinct active sites -> (their Level in (b, y, x, z) order with its bitmap, `order`: sorted row r is given row order[r]).
        static_caps: the capacities of the levels below plus "__rows__", the device count of the rows of `indices` that are no padding."""
        bitmap, order, sorted_idx = ops.bitmap_build(indices if indices.dtype == torch.int32 else indices.int(), spatial_shape,
                                                     batch_size, padded=static_caps is not None)
        caps = None if static_caps is None else {k: v for k, v in static_caps.items() if k != "__rows__"}
        return Level(sorted_idx, spatial_shape, batch_size, bitmap, rows_dev=(static_caps or {}).get("__rows__"), caps=caps), order

    def subm(self, ksize):
        """The SubM rulebook of this level, shared by all its layers of that kernel size."""
        rb = self._subm.get(tuple(ksize))
        if rb is None:
            if self.bitmap is not None:   # (static shapes: nobody reads the pair counts)
                rb = Rulebook(*ops.rulebook_subm_bitmap(self.indices, self.bitmap, ksize, want_counts=self.caps is None))
            else:
                if self._table is None:
                    self._table = ops.coord_table_build(self.indices, self.spatial_shape, self.batch_size)
                rb = Rulebook(*ops.rulebook_subm(self.indices, self.spatial_shape, ksize, self._table))
            self._subm[tuple(ksize)] = rb
        return rb

    def strided(self, indice_key, ksize, stride, pad):
        """-> (Rulebook, output Level) of a strided conv on this level."""
        key = (indice_key, tuple(ksize), tuple(stride), tuple(pad))
        if key not in self._strided:
            if self.bitmap is not None and self.caps is not None:
                out_idx, nbr, counts, bitmap, oshape, rows_dev = ops.rulebook_strided_bitmap(
                    self.indices, self.bitmap, ksize, stride, pad, out_capacity=self.caps[indice_key])
                out = Level(out_idx, oshape, self.batch_size, bitmap, rows_dev=rows_dev, caps=self.caps)
            elif self.bitmap is not None:
                out_idx, nbr, counts, bitmap, oshape = ops.rulebook_strided_bitmap(self.indices, self.bitmap, ksize, stride, pad)
                out = Level(out_idx, oshape, self.batch_size, bitmap)
            else:
                out_idx, nbr, counts, table, oshape = ops.rulebook_strided(self.indices, self.spatial_shape, self.batch_size, ksize, stride, pad)
                out = Level(out_idx, oshape, self.batch_size, table=table)
            self._strided[key] = Rulebook(nbr, counts), out
        return self._strided[key]

    def chain(self):
        """(indice_key, output Level) of every strided conv run from here down, in the order they ran."""
        for key, (_, out) in self._strided.items():
            yield key[0], out
            yield from out.chain()


class SparseConvTensor:
    def __init__(self, features, indices=None, spatial_shape=None, batch_size=None, level=None):
        self.features, self.level = features, level if level is not None else Level(indices, spatial_shape, batch_size)

    indices = property(lambda self: self.level.indices)
    spatial_shape = property(lambda self: self.level.spatial_shape)
    batch_size = property(lambda self: self.level.batch_size)

    def replace_feature(self, features):
        return SparseConvTensor(features, level=self.level)

    @staticmethod
    def sorted_by_bitmap(features, indices, spatial_shape, batch_size, static_caps=None):
        """Reorders distinct active sites into (b, y, x, z) order on a Level with a bitmap: every rulebook down the
        layer chain is then built by bitmap rank (ops.rulebook_*_bitmap) instead of hash tables, and every active
        set stays sorted.  The dense result of an encoder does not depend on the row order."""
        level, order = Level.sorted(indices, spatial_shape, batch_size, static_caps)
        return SparseConvTensor(torch.index_select(features, 0, order), level=level)  # int32 index: one launch

    def dense(self, channels_first=True):
        out = ops.densify(self.features, self.indices, self.batch_size, self.spatial_shape)
        return out if channels_first else out.permute(0, 2, 3, 4, 1)

    def dense_bev(self):
        """dense() viewed as (N, C * D, H, W) (sparse_encoder_custom.py:144-147).  GPU inference on a bitmap-ranked level: one pass that
        writes the map channels-last for the dense backbone (ops.densify_bev); same values, other strides."""
        lvl, C = self.level.bitmap, self.features.shape[1]
        if (lvl is not None and self.features.is_cuda and not (torch.is_grad_enabled() and self.features.requires_grad)
                and (C * self.spatial_shape[0]) % 4 == 0 and self.features.dtype == torch.float32):
            return ops.densify_bev(self.features, lvl, self.batch_size, self.spatial_shape)
        dense = self.dense()
        N, C, D, H, W = dense.shape
        return dense.view(N, C * D, H, W)

    @property
    def spatial_size(self):
        return int(torch.tensor(self.spatial_shape).prod())


_fold_bn = derived.fold_bn   # the name tests/test_host_modules.py takes the fold by


def _bn_foldable(bn):
    return derived.foldable_bn(bn, nn.BatchNorm1d)


class SparseModule(nn.Module):
    pass


class _SparseConv(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False,
                 indice_key=None, subm=False):
        super().__init__()
        assert groups == 1 and _triple(dilation) == [1, 1, 1], "only what the reference encoders use"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.subm, self.indice_key = subm, indice_key
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * math.prod(self.kernel_size)
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        w = state_dict.get(prefix + "weight")
        if w is not None and tuple(w.shape) != tuple(self.weight.shape) and w.dim() == 5 and \
                tuple(w.shape) == (self.out_channels, *self.kernel_size, self.in_channels):
            state_dict[prefix + "weight"] = w.permute(1, 2, 3, 4, 0).contiguous()  # spconv 2.x -> 1.x layout
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @functools.cached_property
    def _packable(self):   # (a shape rule of the library: asked once per layer, not twice per call)
        return ops.spconv_packed_supported(math.prod(self.kernel_size), self.in_channels, self.out_channels)

    def _route(self):
        """The kernel this call of the layer runs on -> (why not the bf16-product one: None when the active mode takes the layer, else why it
        keeps its f32 route, "" outside the mode; whether that f32 route is the packed-weight kernel)."""
        if mfma_dtype.active() is None:
            why = ""
        elif self.training or torch.is_grad_enabled():
            why = "training mode or gradients enabled"
        else:
            why = ops.spconv_bf16_why_not(math.prod(self.kernel_size), self.in_channels, self.out_channels)
        return why, why is not None and not self.training and self._packable

    def index(self, level, route=None):
        """-> (Rulebook, row plan or None, output Level): what this layer needs of the coordinates alone, built on first use, kept on `level`."""
        rb, out = (level.subm(self.kernel_size), level) if self.subm else level.strided(self.indice_key, self.kernel_size, self.stride, self.padding)
        plan = rb.plan(self.in_channels, self.out_channels, rb.nbr.shape[0], self.subm, out.rows_dev) if (route or self._route())[1] else None
        return rb, plan, out

    def forward(self, x, bn=None, relu=False, residual=None):
        """conv, optionally with an eval-mode BatchNorm1d, residual rows and ReLU fused into the same kernel."""
        why, packable = route = self._route()
        rb, plan, out = self.index(x.level, route)
        w = self.weight.view(-1, self.in_channels, self.out_channels)
        alpha = beta = None
        if bn is not None:
            alpha, beta = derived.fold_bn(bn)
            if self.bias is not None:
                beta = beta + self.bias * alpha
        elif self.bias is not None:
            alpha, beta = torch.ones_like(self.bias), self.bias
        mode = mfma_dtype.active()
        if mode is not None:
            mode.report(f"{self.in_channels}->{self.out_channels} k{rb.nbr.shape[0]} {'subm' if self.subm else 'strided'} @{rb.nbr.shape[1]}", why)
        if why is None:   # (an input of 2 GiB or more falls back to srf_spconv_fwd inside ops.spconv_fwd_bf16)
            packed_bf16 = derived.get(self, "spconv_bf16", (self.weight,), lambda: ops.pack_spconv_bf16_weights(w.detach()))
            feats = ops.spconv_fwd_bf16(x.features, w, rb.nbr, packed_bf16, alpha, beta, residual, relu, pair_counts=rb.counts,
                                        rows_dev=out.rows_dev)
            return SparseConvTensor(feats, level=out)
        packed = derived.get(self, "spconv", (self.weight,), lambda: ops.pack_spconv_weights(w.detach())) if packable else None
        feats = ops.spconv_fwd(x.features, w, rb.nbr, alpha, beta, residual, relu, pair_counts=rb.counts, packed=packed,
                               rows_dev=out.rows_dev, tiles=plan, subm=self.subm)
        return SparseConvTensor(feats, level=out)


@CONV_LAYERS.register_module("SubMConv3d")
class SubMConv3d(_SparseConv):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, indice_key,
                         subm=True)


@CONV_LAYERS.register_module("SparseConv3d")
class SparseConv3d(_SparseConv):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, indice_key,
                         subm=False)


class SparseSequential(SparseModule):
    """spconv SparseSequential: sparse modules see the SparseConvTensor, dense modules see `.features`.
    A `conv, BatchNorm1d(eval), ReLU` run is issued as one fused kernel."""

    def __init__(self, *mods, **named):
        super().__init__()
        for i, m in enumerate(mods):
            self.add_module(str(i), m)
        for n, m in named.items():
            self.add_module(n, m)

    def add(self, module, name=None):
        self.add_module(name if name is not None else str(len(self._modules)), module)

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def forward(self, x):
        mods = list(self._modules.values())
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, _SparseConv):
                bn = mods[i + 1] if i + 1 < len(mods) and _bn_foldable(mods[i + 1]) else None
                relu = bn is not None and i + 2 < len(mods) and isinstance(mods[i + 2], nn.ReLU)
                x = m(x, bn=bn, relu=relu)
                i += 1 + (bn is not None) + relu
            elif isinstance(m, SparseModule):
                x = m(x)
                i += 1
            else:
                x = x.replace_feature(m(x.features)) if isinstance(x, SparseConvTensor) else m(x)
                i += 1
        return x


class SparseBasicBlock(SparseModule):
    """mmdet3d SparseBasicBlock: conv1-bn1-relu-conv2-bn2-(+identity)-relu; attribute names conv1/bn1/conv2/bn2."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, conv_cfg=None, norm_cfg=None):
        super().__init__()
        assert downsample is None and stride == 1
        conv_type = (conv_cfg or dict(type="SubMConv3d"))["type"]
        cls = CONV_LAYERS.get(conv_type)
        self.conv1 = cls(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = build_norm_layer(norm_cfg, planes)[1]
        self.conv2 = cls(planes, planes, 3, padding=1, bias=False)
        self.bn2 = build_norm_layer(norm_cfg, planes)[1]
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        identity = x.features
        if _bn_foldable(self.bn1) and _bn_foldable(self.bn2):
            out = self.conv1(x, bn=self.bn1, relu=True)
            return self.conv2(out, bn=self.bn2, relu=True, residual=identity)
        out = self.conv1(x)
        out = out.replace_feature(self.relu(self.bn1(out.features)))
        out = self.conv2(out)
        return out.replace_feature(self.relu(self.bn2(out.features) + identity))


def make_sparse_convmodule(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0,
                           conv_type="SubMConv3d", norm_cfg=None, order=("conv", "norm", "act")):
    """mmdet3d.ops.make_sparse_convmodule: SparseSequential(conv(bias=False), BN1d, ReLU) in `order`."""
    assert isinstance(order, tuple) and len(order) <= 3 and set(order) | {"conv", "norm", "act"} == {"conv", "norm", "act"}
    layers = []
    for layer in order:
        if layer == "conv":
            cls = CONV_LAYERS.get(conv_type)
            if conv_type in ("SparseInverseConv3d", "SparseInverseConv2d", "SparseInverseConv1d"):
                raise NotImplementedError("inverse sparse convs are not on the SRFDet3D path")
            layers.append(cls(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False,
                              indice_key=indice_key))
        elif layer == "norm":
            layers.append(build_norm_layer(norm_cfg, out_channels)[1])
        elif layer == "act":
            layers.append(nn.ReLU(inplace=True))
    return SparseSequential(*layers)
