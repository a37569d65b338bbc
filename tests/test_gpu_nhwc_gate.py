"""The tensor-level half of the channels-last executor's gates on the GPU, at the smallest shapes at which the predicates differ: which
tensors a caller's condition (`nhwc.enabled() and nhwc.<net>_supported(net, x)`) lets through.  EXPECTED is what the gates answered
before they were rewritten over one plan per network (measured with `verdicts` on that tree); no kernel is launched."""
import pytest
import torch

import make_nhwc_calls as calls

pytestmark = pytest.mark.gpu
MAPS = [(8, 12), (4, 6), (2, 3), (1, 2)]
CHANNELS = [64, 96, 128, 160]


def verdicts(dev, monkeypatch):
    """name -> verdict, from the tree `srfdet3d_amd` is imported from."""
    from srfdet3d_amd import nhwc, ops
    vov = calls.vovnet("V-19-eSE").to(dev)
    neck = calls.fpn(in_channels=CHANNELS, out_channels=64, num_outs=4).to(dev)
    sec = calls.second(in_channels=64, out_channels=[64, 128], layer_nums=[1, 1], layer_strides=[1, 2]).to(dev)
    img = torch.zeros(1, 3, 32, 48, device=dev)
    lv = calls.levels(CHANNELS, MAPS, device=dev)
    bev = torch.zeros(1, 64, 16, 16, device=dev)

    def ask(x_img=img, x_lv=lv, x_bev=bev):
        return [nhwc.enabled() and nhwc.vovnet_supported(vov, x_img), nhwc.enabled() and nhwc.fpn_supported(neck, x_lv),
                nhwc.enabled() and nhwc.second_supported(sec, x_bev)]
    out = {}
    with torch.enable_grad():
        out["grad enabled"] = ask()
    with torch.no_grad():
        out["f32 CUDA tensor"] = ask()
        out["f16 tensor"] = ask(img.half(), [x.half() for x in lv], bev.half())
        out["CPU tensor"] = ask(img.cpu(), [x.cpu() for x in lv], bev.cpu())
        with torch.autocast("cuda", dtype=torch.float16):
            out["under autocast"] = ask()
        monkeypatch.setenv("SRF_IMG_NHWC", "0")
        out["SRF_IMG_NHWC=0"] = ask()
        monkeypatch.setenv("SRF_IMG_NHWC", "1")
        # FPN inputs that are views: channels 4 .. 68 and 2 .. 66 of a 68-wide pixel-major buffer (the second 8 bytes off a 16-byte boundary), every
        # second row of a map (channels-last strides, but no channel slice of a pixel-major buffer), the NCHW-contiguous map
        wide = torch.zeros(1, 68, 8, 12, device=dev).contiguous(memory_format=torch.channels_last)
        rows = torch.zeros(1, 64, 16, 12, device=dev).contiguous(memory_format=torch.channels_last)[:, :, ::2]
        out["FPN: aligned channel slice"] = nhwc.enabled() and nhwc.fpn_supported(neck, [wide[:, 4:68], *lv[1:]])
        out["FPN: channel slice 8 bytes off"] = nhwc.enabled() and nhwc.fpn_supported(neck, [wide[:, 2:66], *lv[1:]])
        out["FPN: every second row"] = nhwc.enabled() and nhwc.fpn_supported(neck, [rows, *lv[1:]])
        out["FPN: NCHW-contiguous level"] = nhwc.enabled() and nhwc.fpn_supported(neck, [lv[0].contiguous(), *lv[1:]])
        out["SECOND: channels-last input"] = nhwc.enabled() and nhwc.second_supported(sec, bev.contiguous(memory_format=torch.channels_last))
        # the kernels' own predicates, composed from the limit functions of ops.py
        x = wide.permute(0, 2, 3, 1)
        out["ops.wino3x3_supported"] = [ops.wino3x3_supported(x[..., 4:68]), ops.wino3x3_supported(x[..., 4:16]), ops.wino3x3_supported(x[..., 2:66]),
                                        ops.wino3x3_supported(x[..., 4:68].cpu())]
        out["ops.conv_gemm_nhwc_supported"] = [ops.conv_gemm_nhwc_supported(x[..., 4:68]), ops.conv_gemm_nhwc_supported(x[..., 4:52]),
                                               ops.conv_gemm_nhwc_supported(x[..., 2:66]), ops.conv_gemm_nhwc_supported(x[:, ::2, :, 4:68])]
        out["ops.wino43_supported"] = [ops.wino43_supported(x[..., 4:68], 64), ops.wino43_supported(x[..., 4:68], 66),
                                       ops.wino43_supported(x[..., 4:68], 64, out=x[..., 2:66]), ops.wino43_supported(x[..., 2:66], 64)]
    return {k: [bool(e) for e in v] if isinstance(v, list) else bool(v) for k, v in out.items()}


EXPECTED = {
    "grad enabled": [False, False, False],
    "f32 CUDA tensor": [True, True, True],
    "f16 tensor": [False, False, False],
    "CPU tensor": [False, False, False],
    "under autocast": [False, False, False],
    "SRF_IMG_NHWC=0": [False, False, False],
    "FPN: aligned channel slice": True,
    "FPN: channel slice 8 bytes off": False,
    "FPN: every second row": False,
    "FPN: NCHW-contiguous level": False,
    "SECOND: channels-last input": True,
    "ops.wino3x3_supported": [True, False, False, False],
    "ops.conv_gemm_nhwc_supported": [True, False, False, False],
    "ops.wino43_supported": [True, False, False, False],
}


def test_tensor_level_verdicts(dev, monkeypatch):
    got = verdicts(dev, monkeypatch)
    for name, want in EXPECTED.items():
        assert got[name] == want, name
    assert sorted(got) == sorted(EXPECTED)


def test_the_entries_refuse_what_the_gates_refuse(dev, monkeypatch):
    """`nhwc.vovnet`, `nhwc.fpn`, `nhwc.second` answer None -- the module path -- for a tensor the gate refuses, before any launch."""
    from srfdet3d_amd import nhwc
    vov = calls.vovnet("V-19-eSE").to(dev)
    neck = calls.fpn(in_channels=CHANNELS, out_channels=64, num_outs=4).to(dev)
    sec = calls.second(in_channels=64, out_channels=[64, 128], layer_nums=[1, 1], layer_strides=[1, 2]).to(dev)
    img, lv, bev = torch.zeros(1, 3, 32, 48, device=dev), calls.levels(CHANNELS, MAPS, device=dev), torch.zeros(1, 64, 16, 16, device=dev)
    with torch.enable_grad():
        assert nhwc.vovnet(vov, img) is None and nhwc.fpn(neck, lv) is None and nhwc.second(sec, bev) is None
    with torch.no_grad():
        assert nhwc.vovnet(vov, img.half()) is None and nhwc.fpn(neck, [lv[0].contiguous(), *lv[1:]]) is None
        monkeypatch.setenv("SRF_IMG_NHWC", "0")
        assert nhwc.vovnet(vov, img) is None and nhwc.fpn(neck, lv) is None and nhwc.second(sec, bev) is None
