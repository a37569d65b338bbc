"""How many parameter gradients of a LiDAR + camera training step repeat bit for bit over two passes, with SRF_DETERMINISTIC=1 and
without, and which kernels of the backward pass are left that add with atomics.

The model and inputs are those of tests/test_gpu_fixtures_r2.py::test_lc_training_step: `srfdet_voxel_nusc_LC` with 64 proposals, the
LiDAR branch frozen, one frame of six 128 x 224 images.  Each pass starts from the same seeds (torch for dropout, numpy for GridMask) and the
same weights; nothing is stepped.  A report, not a test: what repeats outside this library's kernels depends on the torch and MIOpen builds.

  python tools/grad_repeat_report.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from srfdet3d_amd import synthetic as S, workloads  # noqa: E402
from srfdet3d_amd.compat.boxes import LiDARInstance3DBoxes  # noqa: E402
from srfdet3d_amd.plugin import training  # noqa: E402


def inputs(dev):
    g = torch.Generator().manual_seed(2)
    n = 8
    b = torch.cat([torch.rand(n, 2, generator=g) * 60 - 30, torch.rand(n, 1, generator=g) * 2 - 3, torch.rand(n, 3, generator=g) * 3 + 1,
                   torch.rand(n, 1, generator=g) * 6 - 3, torch.randn(n, 2, generator=g)], 1)
    return dict(img=torch.from_numpy(S.camera_images(3000, h=128, w=224)).to(dev), points=[torch.from_numpy(S.nuscenes_sweep(2000, 8000)).to(dev)],
                img_metas=[dict(box_type_3d=LiDARInstance3DBoxes, lidar2img=[m for m in S.camera_rig(f=177.0, cx=112.0, cy=64.0)])],
                gt_bboxes_3d=[LiDARInstance3DBoxes(b.to(dev), box_dim=9)], gt_labels_3d=[torch.randint(0, 10, (n,), generator=g).to(dev)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = workloads.build("srfdet_voxel_nusc_LC", 64, train=True)
    training.freeze_lidar_components(model)
    model = model.to(dev).train()
    inp = inputs(dev)

    def grads():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        np.random.seed(0)
        sum(model(return_loss=True, **inp).values()).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}

    report = {}
    for name, value in (("unset", None), ("SRF_DETERMINISTIC=1", "1")):
        if value is None:
            os.environ.pop("SRF_DETERMINISTIC", None)
        else:
            os.environ["SRF_DETERMINISTIC"] = value
        grads()                                                              # warm-up: MIOpen's solver search
        a, b = grads(), grads()
        differ = sorted(n for n in a if not torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)))
        report[name] = dict(parameters=len(a), repeat=len(a) - len(differ), differ=differ)
        print(f"{name}: {len(a) - len(differ)} of {len(a)} parameter gradients repeat bit for bit")
        for n in differ:
            print("   differs:", n, tuple(a[n].shape))
    # the kernels of one forward + backward under the switch whose names say atomic, or that are MIOpen / rocBLAS weight gradients
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        grads()
    names = {}
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA"):
            names[ev.name] = names.get(ev.name, 0) + 1
    # (this library's own kernels are listed separately below: its radix-sort scatter and split GEMMs carry such words without an atomic)
    suspects = {k: v for k, v in names.items() if "srf_" not in k and any(s in k.lower() for s in (
        "atomic", "wrw", "bwdwrw", "backwardweights", "splitk", "split_k", "index_put", "scatter", "embedding", "grid_sampler"))}
    report["kernels_under_the_switch"] = len(names)
    report["suspect_kernels"] = suspects
    print(f"{len(names)} distinct kernels in a step under the switch; by name possibly atomic:")
    for k, v in sorted(suspects.items()):
        print(f"   {v:4d} x {k[:160]}")
    ours = sorted(k for k in names if "srf_roi_extract_bwd_k" in k or "srf_spconv_bwd_weight_k" in k or "srf_msda_bwd" in k)
    print("float-atomic kernels of this library under the switch:", ours or "none")
    report["own_atomic_kernels_under_the_switch"] = ours
    os.environ.pop("SRF_DETERMINISTIC", None)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
