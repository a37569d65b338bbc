#!/usr/bin/env python3
"""Generate tests/golden/nhwc_calls.json: the sequence of `ops` calls the channels-last executor (srfdet3d_amd/nhwc.py) makes for
VoVNet, the FPNs and SECONDCustom, on CPU tensors.  The `ops` functions the executor calls are replaced by stand-ins that record their
arguments and return tensors of the right shape: per call the op's name and, for every parameter of the real function's signature
(defaults filled in), a tensor's shape, strides, storage offset and the serial number of its storage in order of first appearance
within the case (which block buffer a slice belongs to), a scalar's value, "callable" for a lazily packed weight, null for None.
The file holds one line per kernel call: the op, the number of pack calls it caused and a digest of their records (the 1140 calls in
full are 320 KB); `--full FILE` writes the records themselves, for comparing two trees call by call.
`ops.nhwc_ld` and `ops.wino43_supported` test `is_cuda`; they are stood in for by their integer parts.  tests/test_nhwc_calls.py
runs the same recorder on the tree under test and compares: same kernels, same order, same arguments -- with unchanged kernels,
unchanged bits.

The committed file was written from the commit BEFORE the executor was rewritten over one plan per network, from a checkout of it
made by hand (this script runs no git command):

usage:  python tests/golden/make_nhwc_calls.py [--tree CHECKOUT]      (default: the tree this file lies in)
"""
import argparse
import contextlib
import hashlib
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "nhwc_calls.json")
STAGES = ["stage2", "stage3", "stage4", "stage5"]
IMG_NECK = dict(in_channels=[256, 512, 768, 1024], out_channels=256, num_outs=4, add_extra_convs="on_output", relu_before_extra_convs=True)
MAPS = [(8, 12), (4, 6), (2, 3), (1, 2)]
# SECONDCustom as the reference configs build it (voxel / dynamic-voxel configs; pillar configs) and the form with a stride-1 head
SECONDS = {
    "second/voxel": dict(in_channels=256, out_channels=[128, 256], layer_nums=[5, 5], layer_strides=[1, 2]),
    "second/pillar": dict(in_channels=64, out_channels=[64, 128, 256], layer_nums=[3, 5, 5], layer_strides=[2, 2, 2]),
    "second/128": dict(in_channels=128, out_channels=[128, 128, 256], layer_nums=[3, 5, 5], layer_strides=[1, 2, 2]),
}


class _Serials:
    """Storage -> its number in order of first appearance; the storages are held so that no address comes back within a case."""

    def __init__(self):
        self.seen, self.held = {}, []

    def __call__(self, t):
        s = t.untyped_storage()
        if s.data_ptr() not in self.seen:
            self.seen[s.data_ptr()] = len(self.seen)
            self.held.append(s)
        return self.seen[s.data_ptr()]


def _describe(v, serial):
    if isinstance(v, torch.Tensor):
        return dict(shape=list(v.shape), stride=list(v.stride()), offset=v.storage_offset(), storage=serial(v))
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list)):
        return [_describe(e, serial) for e in v]
    if callable(v):
        return "callable"
    raise TypeError(f"cannot describe {type(v)}")


def _zeros(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def _ld(x):
    """ops.nhwc_ld without its device test."""
    N, H, W, C = x.shape
    ld = x.stride(2) if W > 1 else (x.stride(1) if H > 1 else max(C, 1))
    ok = (C == 1 or x.stride(3) == 1) and ld >= C and (W == 1 or x.stride(2) == ld) and (H == 1 or x.stride(1) == W * ld) \
        and (N == 1 or x.stride(0) == H * W * ld)
    if x.dim() != 4 or x.dtype != torch.float32 or not ok:
        raise RuntimeError("not a channel slice of an NHWC buffer")
    return ld


def _out(shape, out):
    return out if out is not None else _zeros(*shape)


def _packs(*operands):
    for p in operands:     # every lazily packed operand is packed: its pack call is recorded
        if callable(p):
            p()


def _conv1x1_nhwc(x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None, pool=False, top=None, packed_direct=None,
                  packed_split=None, packed_bf16=None):
    _packs(packed_weight, packed_direct, packed_split, packed_bf16)
    y = _out((*x.shape[:3], Cout), out)
    return (y, _zeros(x.shape[0], Cout)) if pool else y


def _conv_gemm_nhwc(x, packed_weight, Cout, ksize, stride, pad, scale=None, shift=None, relu=False, out=None, packed_split=None,
                    packed_bf16=None):
    _packs(packed_weight, packed_split, packed_bf16)
    N, H, W, _ = x.shape
    return _out((N, (H + 2 * pad - ksize[0]) // stride + 1, (W + 2 * pad - ksize[1]) // stride + 1, Cout), out)


def _wino43_supported(ops):
    def fn(x, Cout, out=None):
        if not (x.dim() == 4 and x.dtype == torch.float32 and ops.wino43_channels_ok(x.shape[3], Cout) and x.data_ptr() % 16 == 0):
            return False
        try:
            ld, old = _ld(x), (_ld(out) if out is not None else Cout)
        except RuntimeError:
            return False
        if ld % 4 or old % 4 or (out is not None and out.data_ptr() % 16):
            return False
        N, H, W, _ = x.shape
        return ops.wino43_range_ok(N * H * W, max(ld, old)) and ops.wino43_tiles_ok(N, H, W)
    return fn


_PACKS = ["pack_wino3x3_weights", "pack_wino43_weights", "pack_conv1x1_nhwc_weights", "pack_conv1x1_nhwc_direct_weights",
          "pack_conv1x1_nhwc_split_weights", "pack_conv1x1_nhwc_bf16_weights", "pack_conv_gemm_weights", "pack_conv_gemm_split_weights",
          "pack_conv_gemm_bf16_weights"]
# name -> what the stand-in returns (the arguments are bound to the REAL function's signature first)
STANDINS = {
    "stem_conv_nchw": lambda x, weight, scale=None, shift=None, relu=False, out=None:
        _out((x.shape[0], (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1, weight.shape[0]), out),
    "wino43": lambda x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None: _out((*x.shape[:3], Cout), out),
    "wino3x3": lambda x, packed_weight, Cout, scale=None, shift=None, relu=False, out=None: _out((*x.shape[:3], Cout), out),
    "conv1x1_nhwc": _conv1x1_nhwc,
    "conv_gemm_nhwc": _conv_gemm_nhwc,
    "nhwc_affine": lambda x, scale=None, shift=None, relu=False, residual=None, out=None: _out(x.shape, out),
    "ese_gate": lambda mean, weight, bias: _zeros(*mean.shape),
    "to_channels_last": lambda x: x.contiguous(memory_format=torch.channels_last),
    **{name: (lambda weight: _zeros(1)) for name in _PACKS},
}


def _maxpool(ops):
    return lambda x, out=None: _out((x.shape[0], ops.pool3s2_out(x.shape[1]), ops.pool3s2_out(x.shape[2]), x.shape[3]), out)


@contextlib.contextmanager
def recording(nhwc, ops, calls):
    """Within the context the executor's `ops` calls are appended to `calls` instead of launched."""
    standins = dict(STANDINS, nhwc_maxpool3s2_ceil=_maxpool(ops))
    silent = dict(nhwc_ld=_ld, wino43_supported=_wino43_supported(ops))
    real = {name: getattr(ops, name) for name in (*standins, *silent)}
    serial = _Serials()

    def standin(name):
        sig = inspect.signature(real[name])

        def fn(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append(dict(op=name, args={p: _describe(v, serial) for p, v in bound.arguments.items()}))
            return standins[name](*a, **k)
        fn.__name__ = name
        return fn
    # an executor that binds the pack functions at import (as it did before it held their names) is handed the stand-ins directly
    bound_packs = {k: v for k, v in nhwc._PACK.items() if not isinstance(v, str)}
    try:
        for name in standins:
            setattr(ops, name, standin(name))
        for name, fn in silent.items():
            setattr(ops, name, fn)
        for k, v in bound_packs.items():
            nhwc._PACK[k] = getattr(ops, v.__name__)
        yield
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)
        nhwc._PACK.update(bound_packs)


def _eval(m):
    return m.eval().requires_grad_(False)


def vovnet(spec="V-99-eSE", out_features=STAGES, **kw):
    from srfdet3d_amd.plugin.vovnet import VoVNet
    return _eval(VoVNet(spec, out_features=list(out_features), **kw))


def fpn(**kw):
    from srfdet3d_amd.compat.necks import FPN
    return _eval(FPN(**kw))


def second(**kw):
    from srfdet3d_amd.plugin.backbones import SECONDCustom
    return _eval(SECONDCustom(**kw))


def levels(channels, maps=MAPS, n=1, device="cpu"):
    """Channels-last pyramid levels (logical NCHW)."""
    return [torch.zeros(n, c, h, w, device=device).contiguous(memory_format=torch.channels_last) for c, (h, w) in zip(channels, maps)]


def _image():
    return torch.zeros(1, 3, 32, 48)


def _env(name, value):
    @contextlib.contextmanager
    def cm():
        old = os.environ.get(name)
        os.environ[name] = value
        try:
            yield
        finally:
            os.environ.pop(name) if old is None else os.environ.__setitem__(name, old)
    return cm()


def _cases(nhwc):
    """name -> a function that runs the executor; what it returns besides is appended to the record (the bf16 routes)."""
    def v99_upto():
        outs, cur = nhwc.vovnet_forward(vovnet(), _image(), upto="stage3")
        assert list(outs) == ["stage2", "stage3"] and tuple(cur.shape) == (1, 4, 6, 512)

    def v99_wino43_off():
        with _env("SRF_WINO43", "0"):
            nhwc.vovnet_forward(vovnet(), _image())

    def v99_fpn_bf16():
        routes = []
        with nhwc.mfma_dtype(torch.bfloat16, routes=routes):
            nhwc.fpn_forward(fpn(**IMG_NECK), list(nhwc.vovnet_forward(vovnet(), _image()).values()))
        return routes

    def fpn_consumer():
        neck = fpn(**IMG_NECK)
        convs = [_eval(torch.nn.Conv2d(256, 128, 3, padding=1)) for _ in range(4)]
        with nhwc.level_consumer(neck, lambda i, x: nhwc.conv3x3(x, convs[i])):
            assert isinstance(nhwc.fpn_forward(neck, levels(IMG_NECK["in_channels"])), nhwc.ConsumedLevels)

    bev_neck = dict(in_channels=[128, 256], out_channels=128, num_outs=4, add_extra_convs="on_output", act_cfg=dict(type="ReLU"),
                    norm_cfg=dict(type="BN2d", eps=1e-3, momentum=0.01))
    cases = {
        "vovnet99": lambda: nhwc.vovnet_forward(vovnet(), _image()) and None,
        "vovnet99/upto_stage3": v99_upto,
        "vovnet19/stem_out": lambda: nhwc.vovnet_forward(vovnet("V-19-eSE", ["stem", *STAGES]), _image()) and None,
        "vovnet99/wino43_off": v99_wino43_off,
        "vovnet99+fpn/bf16": v99_fpn_bf16,
        "fpn/img": lambda: nhwc.fpn_forward(fpn(**IMG_NECK), levels(IMG_NECK["in_channels"])) and None,
        "fpn/img_consumer": fpn_consumer,
        "fpn/bev_bn_extra": lambda: nhwc.fpn_forward(fpn(**bev_neck), levels([128, 256], [(16, 16), (8, 8)])) and None,
    }
    for name, kw in SECONDS.items():
        cases[name] = lambda kw=kw: nhwc.second_forward(second(**kw), torch.zeros(1, kw["in_channels"], 16, 16)) and None
    return cases


def record(nhwc, ops):
    """{case: [call records]} of the executor module `nhwc` over the `ops` module it uses."""
    out = {}
    for name, run in _cases(nhwc).items():
        torch.manual_seed(0)
        calls = []
        with recording(nhwc, ops, calls), torch.no_grad():
            routes = run()
        if routes is not None:
            calls.append(dict(op="-- routes --", args=routes))
        out[name] = calls
    return out


def layers(calls):
    """The calls of a case, each kernel call (first) with the pack calls it causes."""
    out, ahead = [], []
    for c in calls:
        if c["op"].startswith("pack_wino"):
            ahead.append(c)            # packed eagerly, just before its Winograd call
        elif c["op"].startswith("pack_"):
            out[-1].append(c)          # packed from inside the GEMM call before it
        else:
            out.append([c] + ahead)
            ahead = []
    assert not ahead
    return out


def brief(layer):
    """A kernel call as the fixture holds it: the op, how many pack calls go with it, and a digest of their full records."""
    return f"{layer[0]['op']} +{len(layer) - 1} " + hashlib.sha256(json.dumps(layer, sort_keys=True).encode()).hexdigest()[:10]


def dump(rec, f, line=brief):
    """One kernel call per line."""
    f.write("{\n")
    for i, (name, calls) in enumerate(sorted(rec.items())):
        f.write(f" {json.dumps(name)}: [\n")
        f.write(",\n".join("  " + json.dumps(line(c), sort_keys=True) for c in layers(calls)))
        f.write("\n ]" + ("," if i + 1 < len(rec) else "") + "\n")
    f.write("}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="root of the checkout whose srfdet3d_amd/nhwc.py is recorded")
    ap.add_argument("--full", metavar="FILE", help="also write the records in full, one call per line, to compare two trees call by call")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from srfdet3d_amd import nhwc, ops
    assert os.path.abspath(nhwc.__file__).startswith(os.path.abspath(a.tree) + os.sep), nhwc.__file__
    rec = record(nhwc, ops)
    with open(OUT, "w") as f:
        dump(rec, f)
    if a.full:
        with open(a.full, "w") as f:
            dump(rec, f, line=lambda layer: layer)
    print("wrote", OUT, "from", nhwc.__file__, {k: len(v) for k, v in rec.items()})


if __name__ == "__main__":
    main()
