"""float64 references of the sparse convolution for the gradient tests: conv3d autograd on a densified small grid, and the
same operation straight on a rulebook (index_select / mm / index_add_), which scales to encoder-sized levels.  Plain torch
ops only, no project kernel."""
import torch
import torch.nn.functional as F


def dense_grads(idx, shape, feats, W, gout_rows, out_idx, out_shape, stride, pad, ksize):
    """conv3d on the densified grid; the loss is sum(out[active outputs] * gout_rows).  numpy in, numpy (out, d_feats, d_W) out."""
    B = int(idx[:, 0].max()) + 1
    cin, cout = W.shape[1], W.shape[2]
    f = torch.from_numpy(feats).double().requires_grad_(True)
    w = torch.from_numpy(W).double().requires_grad_(True)
    i = torch.from_numpy(idx).long()
    # channels-last dense grid so that an active site is one row: (B, D, H, W, C) -> (B, C, D, H, W)
    dense = torch.zeros(B, *shape, cin, dtype=torch.float64).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), f).permute(0, 4, 1, 2, 3)
    w5 = w.view(*ksize, cin, cout).permute(4, 3, 0, 1, 2)
    full = F.conv3d(dense, w5, stride=stride, padding=pad)
    o = torch.from_numpy(out_idx).long()
    out = full[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]]
    (out * torch.from_numpy(gout_rows).double()).sum().backward()
    return out.detach().numpy(), f.grad.numpy(), w.grad.numpy()


def conv_ref(nbr, x, W, g):
    """Rulebook convolution in float64: out[o] = sum_k W[k]^T x[nbr[k][o]] (nbr[k][o] = -1: no pair), and for the output
    gradient g the input and weight gradients.  Returns ((out, d_x, d_W), (|out|, |d_x|, |d_W|)): the second triple is the
    same computation on |x|, |W|, |g|, the sum of the magnitudes of the terms behind every element."""
    def run(x, W, g):
        out = x.new_zeros(nbr.shape[1], W.shape[2])
        dx = torch.zeros_like(x)
        dW = torch.zeros_like(W)
        for k in range(nbr.shape[0]):
            o = torch.nonzero(nbr[k] >= 0).squeeze(1)
            i = nbr[k].index_select(0, o).long()
            xi, go = x.index_select(0, i), g.index_select(0, o)
            out.index_add_(0, o, xi @ W[k])
            dx.index_add_(0, i, go @ W[k].T)
            dW[k] = xi.T @ go
        return out, dx, dW

    x, W, g = x.double(), W.double(), g.double()
    return run(x, W, g), run(x.abs(), W.abs(), g.abs())


def conv_ref_autograd(nbr, x, W):
    """The forward of conv_ref as out-of-place torch ops, for torch autograd to differentiate (float64 inputs)."""
    out = x.new_zeros(nbr.shape[1], W.shape[2])
    for k in range(nbr.shape[0]):
        o = torch.nonzero(nbr[k] >= 0).squeeze(1)
        out = out.index_add(0, o, x.index_select(0, nbr[k].index_select(0, o).long()) @ W[k])
    return out
