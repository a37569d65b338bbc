"""`GridMask` (mmdet3d_plugin/models/utils/grid_mask.py:72-128), the image augmentation SRFDet applies to every training image
batch when a config sets use_grid_mask=True (srfdet.py:47-48, :189-190).

The numpy draws stay on the host in the reference's order -- np.random.rand() against prob, then randint(2, h), randint(d)
for st_h, randint(d) for st_w, randint(rotate) -- and `l` is the reference's min(max(int(d * ratio + 0.5), 1), d - 1).  The
device work is `ops.grid_mask`: the stripe mask is evaluated per pixel inside the kernel instead of being built as an
(hh, ww) numpy array, rotated by 0 degrees with PIL, cropped and uploaded, and `out = x * mask` is written to a new tensor
(the caller's image is not changed, as with the reference's `x * mask`).  The product is linear in x, so the gradient is
the same masked product of the incoming gradient.

What is different: rotate > 1 (a PIL rotation of the mask) and offset=True are not implemented -- no config uses them.  The
detector calls GridMask only in training, whereas the reference's forward draws np.random.rand() in eval too before it
returns the input; here an eval forward leaves numpy's global RNG untouched.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops


class _GridMaskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params):
        ctx.params = params
        return ops.grid_mask(x, **params)

    @staticmethod
    def backward(ctx, g):
        return ops.grid_mask(g.contiguous(), **ctx.params), None


class GridMask(nn.Module):
    def __init__(self, use_h, use_w, rotate=1, offset=False, ratio=0.5, mode=0, prob=1.):
        super().__init__()
        if rotate > 1 or offset:
            raise NotImplementedError("srfdet3d_amd: GridMask(rotate > 1) / GridMask(offset=True) (no reference config uses them)")
        self.use_h = use_h
        self.use_w = use_w
        self.rotate = rotate
        self.offset = offset
        self.ratio = ratio
        self.mode = mode
        self.st_prob = prob
        self.prob = prob

    def set_prob(self, epoch, max_epoch):
        self.prob = self.st_prob * epoch / max_epoch

    def draw(self, h):
        """The host half: the reference's numpy draws for an image of height h -> the `ops.grid_mask` parameters, or None
        when this call leaves the image as it is."""
        if np.random.rand() > self.prob:
            return None
        d = np.random.randint(2, h)
        self.l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        st_h = np.random.randint(d)
        st_w = np.random.randint(d)
        np.random.randint(self.rotate)  # the rotation angle: 0 for rotate == 1, drawn to keep numpy's stream in step
        return dict(d=int(d), l=int(self.l), st_h=int(st_h), st_w=int(st_w), use_h=bool(self.use_h), use_w=bool(self.use_w),
                    mode=int(self.mode))

    def forward(self, x):
        """(n, c, h, w) float32 on the GPU -> x * mask (a new tensor) or x itself when the draw says no."""
        if not self.training:
            return x
        params = self.draw(x.shape[-2])
        if params is None:
            return x
        return _GridMaskFn.apply(x.contiguous(), params)
