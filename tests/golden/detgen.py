"""Deterministic tensors keyed by name, shared by make_fixtures.py (which feeds them to the reference's
own Python) and by the tests (which feed them to this repo's implementation).

Storing only a name -> seed rule keeps the committed fixtures down to the expected OUTPUTS: every input and
every weight is regenerated on both sides from `det(name, shape)`.
"""
import zlib

import numpy as np


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode("utf-8")))


def det(name, shape, scale=1.0, shift=0.0):
    """float32 array ~ N(shift, scale^2), a pure function of (name, shape)."""
    return (_rng(name).standard_normal(tuple(shape)).astype(np.float32) * np.float32(scale) + np.float32(shift))


def det_uniform(name, shape, lo=0.0, hi=1.0):
    return _rng(name).uniform(lo, hi, size=tuple(shape)).astype(np.float32)


def det_param(name, shape):
    """Weight rule used for every module parameter / buffer in the fixtures.

    matrices / conv kernels: N(0, 2/(fan_in+fan_out)); LayerNorm/BatchNorm weight: 1 + 0.1 N(0,1);
    biases and running_mean: 0.1 N(0,1); running_var: U(0.5, 1.5).
    """
    shape = tuple(shape)
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "running_var":
        return det_uniform(name, shape, 0.5, 1.5)
    if leaf == "num_batches_tracked":
        return np.zeros(shape, np.int64)
    if len(shape) >= 2:
        recept = int(np.prod(shape[2:])) if len(shape) > 2 else 1
        fan_out, fan_in = shape[0] * recept, shape[1] * recept
        return det(name, shape, scale=float(np.sqrt(2.0 / (fan_in + fan_out))))
    if leaf == "weight":
        return det(name, shape, scale=0.1, shift=1.0)
    return det(name, shape, scale=0.1)


def load_det_params(module, prefix=""):
    """Overwrite every parameter and buffer of a torch module with det_param(prefix + its name)."""
    import torch
    with torch.no_grad():
        for n, p in list(module.named_parameters()) + list(module.named_buffers()):
            v = det_param(prefix + n, p.shape)
            p.copy_(torch.from_numpy(v).to(p.dtype))
    return module


# ------------------------------------------------------------------------------------------------------------
# The damped, trained-like rule of the free-running decoder fixture (make_free_fixture.py -> decoder_free.npz,
# tests/test_gpu_decoder_free.py).  White-noise feature maps make the five-stage loop chaotic (every stage
# multiplies a rounding difference by ~10); a trained decoder reads smooth maps, refines by small steps and
# starts from proposals spread over the scene.  Everything is computed in float64 and rounded to float32 once,
# so the arrays do not depend on the summation order or the libm of the machine that regenerates them.
# ------------------------------------------------------------------------------------------------------------
FREE_EXPERTS = 4            # num_dpg_exp of every config
FREE_DAMPINGS = (0.1, 0.05, 0.02, 0.01)


def free_damping(stored):
    """the member of FREE_DAMPINGS a fixture's float32 `meta.damping` stands for (the rule multiplies by the exact value)"""
    (d,) = [d for d in FREE_DAMPINGS if np.float32(d) == np.float32(stored)]
    return d


def lowpass_map(name, shape, block=8, gain=4.0):
    """det(name, shape) low-passed over its last two axes: mean over block x block cells (the last cell of an axis
    may be narrower), bilinear interpolation of the cell means back to the full size (cell centres as the nodes,
    clamped at the border), times `gain`.  White noise of unit variance comes out with a standard deviation of
    about gain / block * 0.8, i.e. ~0.4: the order of the `scale=0.5` maps of the other fixtures."""
    x = det(name, shape).astype(np.float64)
    for axis in (x.ndim - 2, x.ndim - 1):
        n = x.shape[axis]
        starts = np.arange(0, n, block)
        counts = np.minimum(starts + block, n) - starts
        cell = np.add.reduceat(x, starts, axis=axis) / counts.reshape([-1 if a == axis else 1 for a in range(x.ndim)])
        src = np.clip((np.arange(n) + 0.5) / block - 0.5, 0.0, len(starts) - 1.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), max(len(starts) - 2, 0))
        i1 = np.minimum(i0 + 1, len(starts) - 1)
        w = (src - i0).reshape([-1 if a == axis else 1 for a in range(x.ndim)])
        x = np.take(cell, i0, axis=axis) * (1.0 - w) + np.take(cell, i1, axis=axis) * w
    return (x * gain).astype(np.float32)


def spread_proposal_boxes(name, P, experts=FREE_EXPERTS, size_lo=0.5, size_hi=45.0, jitter=0.02):
    """`init_proposal_boxes.weight` (experts * P, 10) of the free-running fixture: one base box per proposal, repeated
    over the experts with N(0, jitter^2) added, so the softmax mix over the experts keeps the spread.

    base box: centre logits of U(0.03, 0.97) of the range (the head applies the sigmoid), every 16th proposal moved
    next to a face of the range so that the [0, 1] clamp of the centres is met even by small steps; a footprint scale that is
    log-uniform in [size_lo, size_hi] m with width and length within a factor e^+-0.3 of it (BEV RoIs of 0.075 m cells
    change pyramid level at 8.4, 16.8 and 33.6 m, so all four levels are populated), height log-uniform in
    [0.5, 4] m, all stored as logs; a uniform yaw as (sin, cos); velocities N(0, 0.5^2)."""
    r = _rng(name)
    c = r.uniform(0.03, 0.97, size=(P, 3))
    edge = np.arange(0, P, 16)                      # every 16th proposal starts 1e-4 .. 1e-3 of the range (1 .. 11 cm) inside
    near = r.uniform(1e-4, 1e-3, size=len(edge))    # a face of the range, x and y faces in turn: half of them step out
    c[edge, np.arange(len(edge)) % 2] = np.where(np.arange(len(edge)) % 4 < 2, near, 1.0 - near)
    s = np.exp(r.uniform(np.log(size_lo), np.log(size_hi), size=(P, 1)))
    wl = np.clip(s * np.exp(r.uniform(-0.3, 0.3, size=(P, 2))), size_lo, size_hi)
    h = np.exp(r.uniform(np.log(0.5), np.log(4.0), size=(P, 1)))
    yaw = r.uniform(-np.pi, np.pi, size=(P, 1))
    vel = r.standard_normal((P, 2)) * 0.5
    base = np.concatenate([np.log(c / (1.0 - c)), np.log(wl), np.log(h), np.sin(yaw), np.cos(yaw), vel], 1)
    out = base[None] + r.standard_normal((experts, P, 10)) * jitter
    return out.reshape(experts * P, 10).astype(np.float32)


def free_param(name, shape, damping, local=None):
    """det_param, with the weight and bias of every `bboxes_delta*` layer times `damping` and
    `init_proposal_boxes.weight` from spread_proposal_boxes.  `local` is the parameter's name inside the module."""
    local = name if local is None else local
    if local == "init_proposal_boxes.weight":
        return spread_proposal_boxes(name, shape[0] // FREE_EXPERTS)
    v = det_param(name, shape)
    if "bboxes_delta" in local:
        v = (v.astype(np.float64) * damping).astype(np.float32)
    return v


def load_free_params(module, prefix, damping):
    """Overwrite every parameter and buffer of a head with free_param(prefix + its name)."""
    import torch
    with torch.no_grad():
        for n, p in list(module.named_parameters()) + list(module.named_buffers()):
            p.copy_(torch.from_numpy(free_param(prefix + n, tuple(p.shape), damping, n)).to(p.dtype))
    return module


# the cases of decoder_free.npz: name -> (proposals, batch size, fusion head)
FREE_CASES = {"l200": (200, 1, False), "l900": (900, 1, False), "l200b2": (200, 2, False), "f200": (200, 1, True)}
FREE_BEV_SIZES = (184, 92, 46, 23)                       # strides 8..64 of the 1472^2 nuScenes grid
FREE_IMG_SIZES = ((32, 56), (16, 28), (8, 14), (4, 7))   # strides 4..32 of a 128 x 224 px image, six cameras
FREE_N_CAM = 6


def free_prefix(case, k):
    """tensor-name prefix of a case at seed index k (the generator records the first k that meets its conditions)"""
    return f"free.{case}.k{k}."


def free_inputs(case, k):
    """-> (BEV pyramid [(bs,128,s,s)], camera pyramid [(bs,6,256,h,w)] or None), numpy float32."""
    P, bs, fusion = FREE_CASES[case]
    pre = free_prefix(case, k)
    bev = [lowpass_map(f"{pre}feat{i}", (bs, 128, s, s)) for i, s in enumerate(FREE_BEV_SIZES)]
    img = [lowpass_map(f"{pre}img{i}", (bs, FREE_N_CAM, 256, h, w)) for i, (h, w) in enumerate(FREE_IMG_SIZES)] if fusion else None
    return bev, img



def free_metas(bs):
    """the scaled six-camera rig of fusion_nusc.npz (128 x 224 px images), one meta per sample"""
    from srfdet3d_amd import synthetic
    l2i = synthetic.camera_rig(f=177.0, cx=112.0, cy=64.0)
    return [dict(lidar2img=[m for m in l2i]) for _ in range(bs)]


def repo_head(case, k, damping):
    """this repository's head for a case, with the parameters of the rule above"""
    from srfdet3d_amd import workloads
    from srfdet3d_amd.compat.registry import build_head
    P, bs, fusion = FREE_CASES[case]
    m = workloads.model_cfg("srfdet_voxel_nusc_LC" if fusion else "srfdet_voxel_nusc_L")
    hc = dict(m.bbox_head)
    hc.update(num_proposals=P, train_cfg=None, test_cfg=m.test_cfg, use_img=fusion)
    return load_free_params(build_head(hc).eval(), free_prefix(case, k), damping)


def level_stats(rois, num_levels=4, finest_scale=56.0):
    """(R,5) RoIs -> (count per level, smallest distance of log2(scale / finest_scale + 1e-6) to a level boundary)."""
    r = rois.astype(np.float64)
    scale = np.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    if not np.isfinite(scale).all():
        return None, 0.0
    lg = np.log2(scale / finest_scale + 1e-6)
    lvl = np.clip(np.floor(lg), 0, num_levels - 1).astype(np.int64)
    margin = np.abs(lg[:, None] - np.arange(1, num_levels)[None]).min()
    return np.bincount(lvl, minlength=num_levels), float(margin)
