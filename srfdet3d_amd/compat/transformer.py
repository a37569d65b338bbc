"""Stand-ins for the slice of mmcv.cnn.bricks.transformer / mmcv.ops / mmdet.models.utils that `lidar_encoder_cfg` names
(srfdet_head.py:241-243): `MultiScaleDeformableAttention`, `FFN`, `BaseTransformerLayer`, `DetrTransformerEncoder`,
`build_transformer_layer_sequence`, and the head's own `PositionEmbeddingLearned` (srfdet_head.py:25-45).  Plain torch modules with
mmcv's state_dict names (mmcv 1.7 semantics, from memory as everywhere in SURVEY.md: mmcv is not installed).  Only what the eleven
configs use is built; anything else raises NotImplementedError naming it: pre-norm order, cross-attention, other attention types,
`key_padding_mask`, 4-component reference points.

The sampling core has three routes.  `multi_scale_deformable_attn_pytorch` is mmcv's pure-torch form (one grid_sample per level), in the
tensors' own dtype, with autograd, no host synchronisation: CPU tensors, SRF_MSDA=0, unsupported shapes, other dtypes.  On the GPU in
inference `BaseTransformerLayer.forward_rows` runs a whole layer on channels-last rows: srf_linear GEMMs around `ops.msda`
(csrc/msda.hip), six launches and one add per layer.  With gradients enabled on float32 GPU tensors the module's forward hands the
core to `ops.msda_autograd` (forward csrc/msda.hip, backward csrc/msda_bwd.hip; SRF_MSDA_TRAIN=0 keeps the torch core); the Linears,
the dropout and the LayerNorms around it stay torch modules under autograd.  Under SRF_DETERMINISTIC=1 a pass that records a gradient
for `value` raises on either training route: grad_value is float atomics in srf_msda_bwd and in grid_sample's backward alike."""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import derived, ops
from .cnn import BaseModule, ModuleList, build_activation_layer, build_norm_layer
from .registry import Registry

ATTENTION = Registry("attention")
FEEDFORWARD_NETWORK = Registry("feed-forward network")
TRANSFORMER_LAYER = Registry("transformer layer")
TRANSFORMER_LAYER_SEQUENCE = Registry("transformer layer sequence")


def build_attention(cfg):
    if cfg["type"] not in ATTENTION:
        raise NotImplementedError(f"attention type {cfg['type']}: only MultiScaleDeformableAttention is built (DESIGN.md section 7)")
    return ATTENTION.build(cfg)


def build_feedforward_network(cfg):
    return FEEDFORWARD_NETWORK.build(cfg)


def build_transformer_layer(cfg):
    return TRANSFORMER_LAYER.build(cfg)


def build_transformer_layer_sequence(cfg):
    return TRANSFORMER_LAYER_SEQUENCE.build(cfg)


class PositionEmbeddingLearned(nn.Module):
    """Absolute learned position embedding (srfdet_head.py:25-45): (bs, n, in) -> (bs, num_pos_feats, n)."""

    def __init__(self, input_channel, num_pos_feats=288):
        super().__init__()
        self.position_embedding_head = nn.Sequential(nn.Conv1d(input_channel, num_pos_feats, kernel_size=1), nn.BatchNorm1d(num_pos_feats),
                                                     nn.ReLU(inplace=True), nn.Conv1d(num_pos_feats, num_pos_feats, kernel_size=1))

    def forward(self, xyz):
        return self.position_embedding_head(xyz.transpose(1, 2).contiguous())


def multi_scale_deformable_attn_pytorch(value, value_spatial_shapes, sampling_locations, attention_weights):
    """mmcv's pure-torch sampling core.  value (bs, S, heads, d), value_spatial_shapes [(H, W)] (a host list or a tensor whose values are
    read on the host by the caller BEFORE any capture), sampling_locations (bs, Q, heads, L, P, 2) normalised, attention_weights
    (bs, Q, heads, L, P) after the softmax -> (bs, Q, heads d)."""
    bs, _, heads, d = value.shape
    _, Q, _, L, P, _ = sampling_locations.shape
    shapes = [(int(h), int(w)) for h, w in value_spatial_shapes]
    value_list = value.split([h * w for h, w in shapes], dim=1)
    grids = 2 * sampling_locations - 1
    sampled = []
    for lvl, (H, W) in enumerate(shapes):
        value_l = value_list[lvl].flatten(2).transpose(1, 2).reshape(bs * heads, d, H, W)
        grid_l = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(value_l, grid_l, mode="bilinear", padding_mode="zeros", align_corners=False))
    attention_weights = attention_weights.transpose(1, 2).reshape(bs * heads, 1, Q, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * attention_weights).sum(-1).view(bs, heads * d, Q)
    return out.transpose(1, 2).contiguous()


def _lin(lin, x, relu=False):
    """nn.Linear on (..., K); GPU inference goes through dense.linear_graph_safe (this library's ordered GEMM: nothing a captured graph
    replays differently), everything else through torch with autograd."""
    from ..dense import fusable, linear_graph_safe
    if fusable(x) and lin.in_features % 4 == 0 and lin.weight.dtype == torch.float32:
        return linear_graph_safe(lin, x.reshape(-1, x.shape[-1]), relu).view(*x.shape[:-1], lin.out_features)
    y = lin(x)
    return torch.relu(y) if relu else y


def _host_shapes(spatial_shapes):
    if isinstance(spatial_shapes, torch.Tensor):
        return [(int(h), int(w)) for h, w in spatial_shapes.tolist()]
    return [(int(h), int(w)) for h, w in spatial_shapes]


@ATTENTION.register_module()
class MultiScaleDeformableAttention(BaseModule):
    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1, batch_first=False,
                 norm_cfg=None, init_cfg=None):
        super().__init__(init_cfg)
        if embed_dims % num_heads != 0:
            raise ValueError(f"embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}")
        self.norm_cfg = norm_cfg
        self.dropout = nn.Dropout(dropout)
        self.batch_first = batch_first
        self.im2col_step = im2col_step
        self.embed_dims = embed_dims
        self.num_levels = num_levels
        self.num_heads = num_heads
        self.num_points = num_points
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.init_weights()

    def init_weights(self):
        """mmcv's: zero offset weight, the cos / sin ring scaled by its max-abs and by (point index + 1) as the offset bias, zero attention
        weights and bias, xavier-uniform projections with zero bias."""
        nn.init.constant_(self.sampling_offsets.weight, 0.0)
        thetas = torch.arange(self.num_heads, dtype=torch.float32) * (2.0 * math.pi / self.num_heads)
        grid_init = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid_init = (grid_init / grid_init.abs().max(-1, keepdim=True)[0]).view(self.num_heads, 1, 1, 2).repeat(1, self.num_levels,
                                                                                                                 self.num_points, 1)
        for i in range(self.num_points):
            grid_init[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias.copy_(grid_init.view(-1))
        nn.init.constant_(self.attention_weights.weight, 0.0)
        nn.init.constant_(self.attention_weights.bias, 0.0)
        for proj in (self.value_proj, self.output_proj):
            nn.init.xavier_uniform_(proj.weight)
            nn.init.constant_(proj.bias, 0.0)

    def qproj(self):
        """(weight (3 heads L P, C), bias): `sampling_offsets` and `attention_weights` as ONE GEMM operand, offsets first -- the row buffer
        `srf_msda_fwd` reads both from.  Held in derived.py as `msda_qproj`."""
        so, aw = self.sampling_offsets, self.attention_weights
        return derived.get(self, "msda_qproj", (so.weight, so.bias, aw.weight, aw.bias),
                           lambda: (torch.cat((so.weight, aw.weight)).contiguous(), torch.cat((so.bias, aw.bias)).contiguous()))

    def _train_node_ok(self, value, query, reference_points, bs, S, Q):
        """Gradients enabled, float32 GPU tensors, SRF_MSDA / SRF_MSDA_TRAIN on, no gradient wanted for the reference points (the node
        has none), a shape `srf_msda_fwd` / `srf_msda_bwd` take: the sampling core runs as `ops._MsdaFn`."""
        if not torch.is_grad_enabled() or not ops.msda_train_enabled() or reference_points.requires_grad:
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 for t in (value, query, reference_points)):
            return False
        return ops.msda_supported(bs, S, Q, self.num_heads, self.embed_dims // self.num_heads, self.num_levels, self.num_points)

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None, reference_points=None,
                spatial_shapes=None, level_start_index=None, **kwargs):
        if key_padding_mask is not None:
            raise NotImplementedError("MultiScaleDeformableAttention: key_padding_mask is not built (DESIGN.md section 7)")
        if value is None:
            value = query
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        bs, Q, _ = query.shape
        S = value.shape[1]
        shapes = _host_shapes(spatial_shapes)
        if sum(h * w for h, w in shapes) != S:
            raise ValueError(f"MultiScaleDeformableAttention: spatial_shapes {shapes} do not add up to {S} value rows")
        if reference_points.shape[-1] != 2:
            raise NotImplementedError(f"MultiScaleDeformableAttention: reference points with {reference_points.shape[-1]} components are "
                                      "not built, only (x, y) (DESIGN.md section 7)")
        heads, L, P = self.num_heads, self.num_levels, self.num_points
        value = _lin(self.value_proj, value)
        if ops.deterministic_enabled() and torch.is_grad_enabled() and value.requires_grad:
            # grad_value is float atomics on either route: srf_msda_bwd on the HIP node, grid_sample's backward on the torch core
            raise RuntimeError("MultiScaleDeformableAttention: SRF_DETERMINISTIC=1 and a gradient is recorded for `value`, but its only "
                               "kernels add with float atomics (srf_msda_bwd; torch's grid_sample backward on the torch core) and no "
                               "fixed-order srf_msda_bwd is built (DESIGN.md section 4).  Unset SRF_DETERMINISTIC or freeze this encoder.")
        offsets = _lin(self.sampling_offsets, query)
        logits = _lin(self.attention_weights, query)
        if self._train_node_ok(value, query, reference_points, bs, S, Q):
            # training on the GPU: the raw offsets (pixels) and raw logits go to the node, which does the softmax and the positions
            core = ops.msda_autograd(value.reshape(bs * S, -1), shapes, reference_points.reshape(bs * Q, L, 2), offsets.reshape(bs * Q, -1),
                                     logits.reshape(bs * Q, -1), heads, P).view(bs, Q, -1)
        else:
            weights = logits.view(bs, Q, heads, L * P).softmax(-1).view(bs, Q, heads, L, P)
            normalizer = _shape_const(shapes, query)
            locations = reference_points[:, :, None, :, None, :] + offsets.view(bs, Q, heads, L, P, 2) / normalizer[None, None, None, :, None, :]
            core = multi_scale_deformable_attn_pytorch(value.view(bs, S, heads, -1), shapes, locations, weights)
        output = _lin(self.output_proj, core)
        if not self.batch_first:
            output = output.permute(1, 0, 2)
        return self.dropout(output) + identity


_SHAPE_CONSTS = {}


def _shape_const(shapes, like):
    """(L, 2) = (W_l, H_l) on `like`'s device, uploaded once: a host -> device copy per call would be illegal inside a graph capture."""
    key = (tuple(shapes), like.device, like.dtype)
    t = _SHAPE_CONSTS.get(key)
    if t is None:
        t = _SHAPE_CONSTS[key] = torch.tensor([[w, h] for h, w in shapes], dtype=like.dtype, device=like.device)
    return t


@FEEDFORWARD_NETWORK.register_module()
class FFN(BaseModule):
    """mmcv's FFN: layers = Sequential(Sequential(Linear, act, Dropout) x (num_fcs - 1), Linear, Dropout); out = identity + layers(x)."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.0,
                 dropout_layer=None, add_identity=True, init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        if num_fcs < 2:
            raise ValueError(f"num_fcs should be no less than 2. got {num_fcs}.")
        if dropout_layer is not None:
            raise NotImplementedError("FFN: dropout_layer is not built")
        self.embed_dims, self.feedforward_channels, self.num_fcs = embed_dims, feedforward_channels, num_fcs
        self.act_cfg = act_cfg
        layers, in_channels = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(in_channels, feedforward_channels), build_activation_layer(act_cfg), nn.Dropout(ffn_drop)))
            in_channels = feedforward_channels
        layers.append(nn.Linear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        self.dropout_layer = nn.Identity()
        self.add_identity = add_identity

    def forward(self, x, identity=None):
        if not self.training and self.num_fcs == 2 and isinstance(self.layers[0][1], nn.ReLU):
            out = _lin(self.layers[1], _lin(self.layers[0][0], x, relu=True))    # the dropouts are identities in eval
        else:
            out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        return (x if identity is None else identity) + self.dropout_layer(out)


@TRANSFORMER_LAYER.register_module()
class BaseTransformerLayer(BaseModule):
    def __init__(self, attn_cfgs=None, ffn_cfgs=dict(type="FFN", embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.0,
                                                      act_cfg=dict(type="ReLU", inplace=True)),
                 operation_order=None, norm_cfg=dict(type="LN"), init_cfg=None, batch_first=False, **kwargs):
        super().__init__(init_cfg)
        ffn_cfgs = copy.deepcopy(dict(ffn_cfgs)) if isinstance(ffn_cfgs, dict) else copy.deepcopy(ffn_cfgs)
        # the deprecated top-level keys the configs still carry are folded into ffn_cfgs, as mmcv does (with a warning there)
        for old, new in (("feedforward_channels", "feedforward_channels"), ("ffn_dropout", "ffn_drop"), ("ffn_num_fcs", "num_fcs")):
            if old in kwargs:
                ffn_cfgs[new] = kwargs.pop(old)
        if kwargs:
            raise NotImplementedError(f"BaseTransformerLayer: arguments {sorted(kwargs)} are not built")
        operation_order = tuple(operation_order)
        if not set(operation_order) <= {"self_attn", "norm", "ffn", "cross_attn"}:
            raise ValueError(f"BaseTransformerLayer: unknown operations in {operation_order}")
        if "cross_attn" in operation_order:
            raise NotImplementedError("BaseTransformerLayer: cross_attn is not built (DESIGN.md section 7)")
        if operation_order[0] == "norm":
            raise NotImplementedError("BaseTransformerLayer: the pre-norm operation order is not built (DESIGN.md section 7)")
        num_attn = operation_order.count("self_attn")
        if isinstance(attn_cfgs, dict):
            attn_cfgs = [copy.deepcopy(attn_cfgs) for _ in range(num_attn)]
        if len(attn_cfgs) != num_attn:
            raise ValueError(f"{len(attn_cfgs)} attn_cfgs for {num_attn} attentions in {operation_order}")
        self.batch_first = batch_first
        self.operation_order = operation_order
        self.norm_cfg = norm_cfg
        self.pre_norm = False
        self.attentions = ModuleList()
        for cfg in attn_cfgs:
            cfg = dict(cfg)
            cfg["batch_first"] = batch_first
            self.attentions.append(build_attention(cfg))
        self.embed_dims = self.attentions[0].embed_dims
        num_ffns = operation_order.count("ffn")
        if isinstance(ffn_cfgs, dict):
            ffn_cfgs = [copy.deepcopy(ffn_cfgs) for _ in range(num_ffns)]
        self.ffns = ModuleList()
        for cfg in ffn_cfgs:
            cfg = dict(cfg)
            cfg.setdefault("embed_dims", self.embed_dims)
            cfg.setdefault("type", "FFN")
            self.ffns.append(build_feedforward_network(cfg))
        self.norms = ModuleList([build_norm_layer(norm_cfg, self.embed_dims)[1] for _ in range(operation_order.count("norm"))])

    def forward(self, query, key=None, value=None, query_pos=None, key_pos=None, attn_masks=None, query_key_padding_mask=None,
                key_padding_mask=None, **kwargs):
        norm_index = attn_index = ffn_index = 0
        for op in self.operation_order:
            if op == "self_attn":   # key = value = query, key_pos = query_pos; identity None: the attention adds its own input
                query = self.attentions[attn_index](query, query, query, None, query_pos=query_pos, key_pos=query_pos,
                                                    key_padding_mask=query_key_padding_mask, **kwargs)
                attn_index += 1
            elif op == "norm":
                query = self.norms[norm_index](query)
                norm_index += 1
            else:
                query = self.ffns[ffn_index](query, None)
                ffn_index += 1
        return query

    # ---- the layer on channels-last rows (GPU inference) --------------------------------------------------------------------------------
    def rows_ok(self):
        """The structure `forward_rows` executes: (self_attn, norm, ffn, norm) around a MultiScaleDeformableAttention, a two-layer ReLU
        FFN with the identity add, LayerNorms, everything in eval mode."""
        if self.operation_order != ("self_attn", "norm", "ffn", "norm") or self.training:
            return False
        ffn = self.ffns[0]
        return (isinstance(self.attentions[0], MultiScaleDeformableAttention) and isinstance(ffn, FFN) and ffn.num_fcs == 2
                and ffn.add_identity and isinstance(ffn.layers[0][1], nn.ReLU) and all(isinstance(n, nn.LayerNorm) for n in self.norms)
                and self.embed_dims % 4 == 0 and ffn.feedforward_channels % 4 == 0 and max(self.embed_dims, ffn.feedforward_channels) <= 1024)

    def forward_rows(self, x, pos, ref, shapes):
        """x (B S, C) rows of the flattened channels-last pyramid (batch-major, levels one after the other), pos (S, C) the position
        embedding, ref (B S, L, 2) -> (B S, C).  Launches: value_proj, the add of pos, offsets + logits as one GEMM, srf_msda_fwd,
        output_proj + residual + LayerNorm, fc1 + ReLU, fc2 + residual + LayerNorm."""
        att, ffn = self.attentions[0], self.ffns[0]
        ns = att.num_heads * att.num_levels * att.num_points
        value = ops.linear(x, att.value_proj.weight, att.value_proj.bias)
        wq, bq = att.qproj()
        B = x.shape[0] // pos.shape[0]
        q = (x.view(B, *pos.shape) + pos).view_as(x)
        qp = ops.linear(q, wq, bq)
        core = ops.msda(value, shapes, ref, qp[:, :2 * ns], qp[:, 2 * ns:], att.num_heads, att.num_points)
        x = ops.linear(core, att.output_proj.weight, att.output_proj.bias, residual=x, ln2=self.norms[0])
        fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
        hidden = ops.linear(x, fc1.weight, fc1.bias, relu1=True)
        return ops.linear(hidden, fc2.weight, fc2.bias, residual=x, ln2=self.norms[1])


class TransformerLayerSequence(BaseModule):
    def __init__(self, transformerlayers=None, num_layers=None, init_cfg=None):
        super().__init__(init_cfg)
        if isinstance(transformerlayers, dict):
            transformerlayers = [copy.deepcopy(transformerlayers) for _ in range(num_layers)]
        if len(transformerlayers) != num_layers:
            raise ValueError(f"{len(transformerlayers)} transformerlayers for num_layers = {num_layers}")
        self.num_layers = num_layers
        self.layers = ModuleList([build_transformer_layer(cfg) for cfg in transformerlayers])
        self.embed_dims = self.layers[0].embed_dims
        self.pre_norm = self.layers[0].pre_norm

    def forward(self, query, key, value, query_pos=None, key_pos=None, attn_masks=None, query_key_padding_mask=None, key_padding_mask=None,
                **kwargs):
        for layer in self.layers:
            query = layer(query, key, value, query_pos=query_pos, key_pos=key_pos, attn_masks=attn_masks,
                          query_key_padding_mask=query_key_padding_mask, key_padding_mask=key_padding_mask, **kwargs)
        return query


@TRANSFORMER_LAYER_SEQUENCE.register_module()
class DetrTransformerEncoder(TransformerLayerSequence):
    """mmdet's: a final LayerNorm only in the pre-norm order; in the post-norm order the configs use there is none."""

    def __init__(self, *args, post_norm_cfg=dict(type="LN"), **kwargs):
        super().__init__(*args, **kwargs)
        self.post_norm = None

    def forward(self, *args, **kwargs):
        return super().forward(*args, **kwargs)

    def rows_supported(self, B, shapes):
        """Whether `forward_rows` takes a batch of B pyramids of `shapes`: every layer has the structure and `srf_msda_fwd` the shape."""
        S = sum(h * w for h, w in shapes)
        for layer in self.layers:
            if not layer.rows_ok():
                return False
            att = layer.attentions[0]
            if att.num_levels != len(shapes) or not ops.msda_supported(B, S, S, att.num_heads, att.embed_dims // att.num_heads,
                                                                      att.num_levels, att.num_points,
                                                                      offs_ld=3 * att.num_heads * att.num_levels * att.num_points,
                                                                      logits_ld=3 * att.num_heads * att.num_levels * att.num_points):
                return False
            ns = att.num_heads * att.num_levels * att.num_points
            if (2 * ns) % 4:   # the logits' base inside the shared row buffer stays 16-byte aligned
                return False
        return True

    def forward_rows(self, x, pos, ref, shapes):
        for layer in self.layers:
            x = layer.forward_rows(x, pos, ref, shapes)
        return x
