#!/usr/bin/env python3
"""Generate tests/golden/train_conv_calls.json: the sequence of `ops` calls each autograd node of srfdet3d_amd/train_conv.py makes,
forward and backward, at one tiny shape (N = 1, H = 4, W = 32, 32 channels) on CPU tensors -- each convolution node a second time as
`<case>/bf16`: forward inside `train_conv.mfma_dtype(torch.bfloat16, routes=[...])`, backward after the context has closed, the route
list as a last `-- routes --` record.  The `ops` functions the nodes use are
replaced by stand-ins that record their arguments and return tensors of the right shape: per call the op's name and, for every
parameter of the real function's signature (defaults filled in, so positional and keyword spellings are one), a tensor's shape and
strides, a scalar's value, "callable" for a lazily packed weight, null for None.  `ops.nhwc_ld` tests `is_cuda`; it is stood in for,
unrecorded, by `make_nhwc_calls._ld`.  tests/test_train_conv_calls.py runs the same
recorder on the tree under test and compares: same kernels, same order, same arguments -- with unchanged kernels, unchanged bits.

The committed file was written from the commit BEFORE the nodes were rewritten over one layer primitive, its `/bf16` cases from the
commit BEFORE the three bf16-product modes were put on one context class, each from a checkout of it made by
hand (this script runs no git command):

usage:  python tests/golden/make_train_conv_calls.py [--tree CHECKOUT]      (default: the tree this file lies in)
"""
import argparse
import contextlib
import inspect
import json
import os
import sys

import torch

from make_nhwc_calls import _conv_gemm_nhwc, _ld

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "train_conv_calls.json")
N, H, W, C = 1, 4, 32, 32


def _describe(v):
    if isinstance(v, torch.Tensor):
        return dict(shape=list(v.shape), stride=list(v.stride()))
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list)):
        return [_describe(e) for e in v]
    if callable(v):
        return "callable"
    raise TypeError(f"cannot describe {type(v)}")


def _zeros(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def _conv_out(x, Cout, out):
    return out if out is not None else _zeros(x.shape[0], x.shape[1], x.shape[2], Cout)


def _conv1x1_nhwc(x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None, pool=False, top=None, packed_direct=None,
                  packed_split=None, packed_bf16=None):
    for p in (packed_weight, packed_direct, packed_split, packed_bf16):     # every lazily packed operand is packed: its pack call is recorded
        if callable(p):
            p()
    return _conv_out(x, Cout, out)


# name -> what the stand-in returns (the arguments are bound to the REAL function's signature first)
STANDINS = {
    "wino43": lambda x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None: _conv_out(x, Cout, out),
    "conv1x1_nhwc": _conv1x1_nhwc,
    "conv_gemm_nhwc": _conv_gemm_nhwc,
    "pack_conv_gemm_bf16_weights": lambda weight: _zeros(1),
    "pack_conv1x1_nhwc_bf16_weights": lambda weight: _zeros(1),
    "conv_wgrad_nhwc_bf16": lambda g, x, ksize: _zeros(g.shape[3], x.shape[3], ksize, ksize),
    "conv_wgrad_bf16_supported": lambda g, x, ksize: True,
    "pack_wino43_weights": lambda weight: _zeros(1),
    "pack_conv1x1_nhwc_weights": lambda weight: _zeros(1),
    "pack_conv1x1_nhwc_split_weights": lambda weight: _zeros(1),
    "bn_eval_fold": lambda gamma, beta, mean, var, eps: torch.ones(3, gamma.numel()),
    "nhwc_affine_relu_bwd": lambda gy, y, scale, relu, gy2=None: (_zeros(*gy.shape), _zeros(2, gy.shape[3])),
    "bn_eval_grads": lambda sums, fold, mean: _zeros(2, mean.numel()),
    "conv_wgrad_nhwc": lambda g, x, ksize: _zeros(g.shape[3], x.shape[3], ksize, ksize),
    "conv_wgrad_supported": lambda g, x, ksize: True,
    "nhwc_colmean": lambda x: _zeros(x.shape[0], x.shape[3]),
    "ese_gate": lambda mean, weight, bias: _zeros(*mean.shape),
    "nhwc_affine": lambda x, scale=None, shift=None, relu=False, residual=None, out=None: _zeros(*x.shape),
    "nhwc_colsum_prod": lambda a, b: _zeros(a.shape[0], a.shape[3]),
}


@contextlib.contextmanager
def recording(ops, calls):
    real = {name: getattr(ops, name) for name in (*STANDINS, "nhwc_ld")}

    def standin(name):
        sig = inspect.signature(real[name])

        def fn(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append(dict(op=name, args={p: _describe(v) for p, v in bound.arguments.items()}))
            return STANDINS[name](*a, **k)
        return fn
    try:
        for name in STANDINS:
            setattr(ops, name, standin(name))
        ops.nhwc_ld = _ld            # silent: not an `ops` call of the record
        yield
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)


def _t(*shape, grad=True):
    return torch.randn(*shape).requires_grad_(grad)


def _map(channels=C, grad=True, channels_last=True):
    x = torch.randn(N, channels, H, W)
    return (x.contiguous(memory_format=torch.channels_last) if channels_last else x).requires_grad_(grad)


def _bn(channels=C, grad=True):
    return [_t(channels, grad=grad), _t(channels, grad=grad), torch.randn(channels), torch.rand(channels) + 0.5]   # gamma, beta, mean, var


def _cases(tc):
    """name -> a function that runs one node forward and returns its output."""
    osa = lambda grad_x: lambda: tc._OSAChain.apply(_map(grad=grad_x), (1e-5, 1e-5, 1e-3), _t(C, C, 3, 3), *_bn(), _t(C, C, 3, 3), *_bn(),  # noqa: E731
                                                    _t(C, 3 * C, 1, 1), *_bn())
    return {
        "_Wino43Conv": lambda: tc._Wino43Conv.apply(_map(), _t(C, C, 3, 3), _t(C)),
        "_Wino43Conv/nchw_no_bias": lambda: tc._Wino43Conv.apply(_map(channels_last=False), _t(C, C, 3, 3), None),
        "_ConvAffineRelu/3x3": lambda: tc._ConvAffineRelu.apply(_map(), _t(C, C, 3, 3), None, *_bn(), 1e-5, True),
        "_ConvAffineRelu/1x1_bias_frozen": lambda: tc._ConvAffineRelu.apply(_map(grad=False), _t(C, C, 1, 1), _t(C), *_bn(grad=False), 1e-3, False),
        "_OSAChain": osa(True),
        "_OSAChain/frozen_x": osa(False),
        "_Conv1x1": lambda: tc._Conv1x1.apply(_map(), _t(C, C, 1, 1), _t(C)),
        "_ESEApply": lambda: tc._ESEApply.apply(_map(), _map(), _t(C, C, 1, 1), _t(C)),
    }


BF16 = "/bf16"   # the suffix of a case run inside the bf16-product mode: every case but `_ESEApply`, which has no convolution


def record(tc, ops):
    """{case: [call records]} of srfdet3d_amd.train_conv module `tc` over the `ops` module it uses."""
    out = {}
    cases = _cases(tc)
    for name, run in [*cases.items(), *((n + BF16, r) for n, r in cases.items() if n != "_ESEApply")]:
        torch.manual_seed(0)
        calls, routes = [], ([] if name.endswith(BF16) else None)
        with recording(ops, calls):
            with tc.mfma_dtype(None if routes is None else torch.bfloat16, routes=routes):
                y = run()
            calls.append(dict(op="-- backward --", args={}))
            y.backward(torch.randn_like(y))
        if routes is not None:
            calls.append(dict(op="-- routes --", args=routes))
        out[name] = calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="root of the checkout whose srfdet3d_amd/train_conv.py is recorded")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from srfdet3d_amd import ops, train_conv
    assert os.path.abspath(train_conv.__file__).startswith(os.path.abspath(a.tree) + os.sep), train_conv.__file__
    with open(OUT, "w") as f:
        json.dump(record(train_conv, ops), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "from", train_conv.__file__)


if __name__ == "__main__":
    main()
