"""The bf16-product mode of the training convolutions (train_conv.mfma_dtype) restated in float64 on the CPU: a convolution that rounds
its operands to bf16 in all three directions,

    forward        y  = conv(bf16(x), bf16(W))
    data gradient  dx = conv^T(bf16(gy), bf16(W))
    weight grad    dW = sum_p bf16(gy[p]) bf16(x[p + tap])

with bf16() = round to nearest even of the value as an f32 (Tensor.bfloat16()), everything else -- sums, bias, BatchNorm, ReLU -- exact
in float64 under torch's own autograd.  The nodes of train_conv.py in the mode are held to it by tests/test_gpu_train_bf16.py."""
import torch
import torch.nn.functional as F


def bf16(t):
    return t.float().bfloat16().double()


class RoundedConv(torch.autograd.Function):
    """k x k / stride 1 / padding k // 2 convolution without bias, float64 tensors."""

    @staticmethod
    def forward(ctx, x, w, g_operand=None):
        ctx.save_for_backward(x, w)
        ctx.g_operand = g_operand
        return F.conv2d(bf16(x), bf16(w), None, padding=w.shape[2] // 2)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        pad = w.shape[2] // 2
        if ctx.g_operand is not None:
            # The operand of the two gradient products is the f32 tensor the (unchanged, f32) BatchNorm / ReLU backward pass hands the
            # convolution, rounded ONCE.  float64 -> f32 -> bf16 of this reference's own gy rounds twice, and a value an f32 ulp beside a
            # bf16 rounding boundary lands on the other bf16 neighbour: 2^-9 of one element, 1e-4 of a 1450-pixel gradient.  So the f32
            # tensor is handed in -- and may differ from gy by f32 rounding only.
            assert float((ctx.g_operand - gy).abs().max()) <= 1e-6 * float(gy.abs().max())
            gy = ctx.g_operand
        g = bf16(gy)
        gx = torch.nn.grad.conv2d_input(x.shape, bf16(w), g, padding=pad) if ctx.needs_input_grad[0] else None
        gw = torch.nn.grad.conv2d_weight(bf16(x), w.shape, g, padding=pad) if ctx.needs_input_grad[1] else None
        return gx, gw, None


def conv(x, w, bias=None, g_operand=None):
    y = RoundedConv.apply(x, w, g_operand)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def conv_bn_relu(x, w, bias, gamma, beta, mean, var, eps, relu, got=None, tol=0.0, g_operand=None):
    """got, tol: the ReLU has no derivative at 0, and an output the reference puts within rounding of 0 may lie on the other side in f32:
    its value differs by nothing, its gradient by everything.  Where the reference's own |u| <= tol * max |y| -- the tolerance the
    OUTPUT is held to -- the reference takes the side `got` (the node's output) took; everywhere else its own.
    g_operand: the f32 gradient the convolution receives, see `RoundedConv.backward`."""
    u = F.batch_norm(conv(x, w, bias, g_operand), mean, var, gamma, beta, False, 0.0, eps)
    if not relu:
        return u
    if got is None:
        return torch.relu(u)
    ud = u.detach()
    near = ud.abs() <= tol * float(torch.relu(ud).max())
    return u * torch.where(near, got > 0, ud > 0)
