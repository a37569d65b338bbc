"""Definitions of the layers the channels-last executor adds for the bottleneck ResNets (csrc/conv.hip: srf_stem_conv7_nchw; csrc/nhwc.hip:
srf_nhwc_maxpool3s2_pad1; the residual form of the 1x1 GEMM), in numpy float64 on the CPU.  tests/test_resnet_ref.py holds them to
torch's own float64 operators; the GPU tests compare the kernels with them.

Error bound of a k-ordered f32 dot product of n terms followed by an f32 scale / shift, whatever the order of summation:
|error| <= gamma(n + 2) * (|scale| * sum |x w| + |shift|), gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1): n - 1 additions and n products are at most n roundings per term, the affine adds two."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def conv_out(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def conv2d_nchw(x, w, stride, pad):
    """x (N, Cin, H, W), w (Cout, Cin, kh, kw) -> (N, Cout, Ho, Wo) in float64, zero padding; one tap at a time."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    xp = np.zeros((N, Cin, H + 2 * pad + stride, W + 2 * pad + stride))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    y = np.zeros((N, Cout, Ho, Wo))
    for ky in range(kh):
        for kx in range(kw):
            tap = xp[:, :, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride]
            y += np.einsum("nchw,oc->nohw", tap, w[:, :, ky, kx])
    return y


def affine_act(y, scale, shift, relu, axis):
    """y * scale + shift along `axis` (either may be None), optional ReLU."""
    shape = [1] * y.ndim
    shape[axis] = -1
    if scale is not None:
        y = y * np.asarray(scale, np.float64).reshape(shape)
    if shift is not None:
        y = y + np.asarray(shift, np.float64).reshape(shape)
    return np.maximum(y, 0.0) if relu else y


def stem7(x, w, scale=None, shift=None, relu=False):
    """Conv2d(Cin, 64, 7, stride 2, padding 3) + scale / shift + ReLU: NCHW images -> (value, error bound), both (N, Ho, Wo, 64)."""
    y = conv2d_nchw(x, w, 2, 3)
    mag = conv2d_nchw(np.abs(x), np.abs(w), 2, 3)
    K = w.shape[1] * 49
    bound = gamma(K + 2) * affine_act(mag, None if scale is None else np.abs(scale), None if shift is None else np.abs(shift), False, 1)
    return affine_act(y, scale, shift, relu, 1).transpose(0, 2, 3, 1), bound.transpose(0, 2, 3, 1)


def conv_nhwc(x, w, stride, pad, scale=None, shift=None, relu=False):
    """A Conv2d on an (N, H, W, Cin) map, w (Cout, Cin, kh, kw) -> (value, error bound) (N, Ho, Wo, Cout)."""
    xc = np.asarray(x, np.float64).transpose(0, 3, 1, 2)
    y = conv2d_nchw(xc, w, stride, pad)
    mag = conv2d_nchw(np.abs(xc), np.abs(w), stride, pad)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    bound = gamma(K + 2) * affine_act(mag, None if scale is None else np.abs(scale), None if shift is None else np.abs(shift), False, 1)
    return affine_act(y, scale, shift, relu, 1).transpose(0, 2, 3, 1), bound.transpose(0, 2, 3, 1)


def pool3s2p1_out(h):
    return (h - 1) // 2 + 1


def maxpool3s2_pad1(x):
    """MaxPool2d(3, stride 2, padding 1), floor mode, on (N, H, W, C): the padding is -inf."""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = pool3s2p1_out(H), pool3s2p1_out(W)
    xp = np.full((N, H + 3, W + 3, C), -np.inf, x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    y = np.full((N, Ho, Wo, C), -np.inf, x.dtype)
    for ky in range(3):
        for kx in range(3):
            y = np.maximum(y, xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
    return y


def residual_act(z, res, relu):
    """The residual epilogue on f32 values: act(fl(z + res)), the add BEFORE the ReLU."""
    v = np.asarray(z, np.float32) + np.asarray(res, np.float32)
    return np.maximum(v, np.float32(0)) if relu else v


def fpn_order(z, res, relu):
    """What the top-down form would give: act(z) + res -- the add AFTER the ReLU."""
    z = np.asarray(z, np.float32)
    return (np.maximum(z, np.float32(0)) if relu else z) + np.asarray(res, np.float32)
