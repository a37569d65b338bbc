"""The one cache of tensors derived from a module's parameters and buffers.

Everything held for a module lives in `mod.__dict__["_srf_derived"]`, a plain dict name -> (key, value); key is the tuple of
(t._version, t.data_ptr()) over the tensors the value was made from.  Optimiser steps, `copy_` and `load_state_dict` bump a version,
`p.data = other` changes a pointer; an in-place update THROUGH `.data` (`p.data.mul_()`, old-style EMA) changes neither and needs
`invalidate` (the detector: `weights_changed()`).  The names in use:

  wino, wino43                          Winograd F(2x2, 3x3) / F(4x4, 3x3) operands               (nhwc.packed)
  gemm, gemm_direct, gemm_split, gemm_bf16    the operand orders of a channels-last 1x1 layer     (nhwc.packed)
  cgemm, cgemm_split, cgemm_bf16        the same for the implicit-im2col GEMM                     (nhwc.packed)
  conv1x1_nchw                          the `srf_conv1x1` operand                                 (dense.conv1x1_cat_bn_act)
  spconv                                the packed sparse-conv weight                             (sparse._SparseConv)
  spconv_bf16                           its bf16 operand images, inside `sparse.mfma_dtype`       (sparse._SparseConv)
  dcn, dcn_offset                       the two GEMM operands of a DCNv2 pack                     (compat/dcn.py)
  bn_fold                               (scale, shift) of an eval BatchNorm                       (fold_bn)
  linear_padded                         an nn.Linear weight zero-padded to K % 4 == 0             (dense.linear_graph_safe)
  msda_qproj                            `sampling_offsets` and `attention_weights` as one GEMM operand and its bias
                                                                                                  (compat/transformer.py)
  lidar_pos                             position + level embedding of every pixel of the BEV pyramid, an eval-mode function of the
                                        weights alone                                             (plugin/heads.py `_lidar_pos`)
"""
import torch

_SLOT = "_srf_derived"


def get(mod, name, tensors, make):
    """The value `make()` gave for `name` on `mod`, rebuilt (under no_grad) when one of `tensors` has another version or pointer.
    A None result is a value like any other: it is cached, not retried."""
    key = tuple((t._version, t.data_ptr()) for t in tensors)
    held = mod.__dict__.setdefault(_SLOT, {})
    entry = held.get(name)
    if entry is None or entry[0] != key:
        with torch.no_grad():
            entry = held[name] = (key, make())
    return entry[1]


def names(mod):
    """The set of names currently held for `mod`."""
    return set(mod.__dict__.get(_SLOT, ()))


def invalidate(model):
    """Drops everything held for every module of `model`."""
    for m in model.modules():
        m.__dict__.pop(_SLOT, None)


def foldable_bn(bn, cls):
    """A `cls` (nn.BatchNorm1d / nn.BatchNorm2d) that is the affine map `fold_bn` folds: eval mode, running statistics, gamma and beta."""
    return isinstance(bn, cls) and not bn.training and bn.track_running_stats and bn.affine


def fold_bn(bn):
    """(scale, shift) of an eval-mode BatchNorm1d / BatchNorm2d: scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    def make():
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        return scale.contiguous(), shift.contiguous()
    return get(bn, "bn_fold", (bn.weight, bn.bias, bn.running_mean, bn.running_var), make)
