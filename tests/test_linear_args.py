"""Return codes of `srf_linear`, `srf_self_attention_batched`, `srf_dynconv_mid`, `srf_ese_gate`, `srf_stage_tail`, `srf_apply_deltas` and
`srf_dpg_mix`, in the order the entry points check them: sizes and pitches SRF_EINVAL, a half-given LayerNorm SRF_EINVAL, nothing to do
SRF_OK, null pointers SRF_EINVAL, a shape outside the limits SRF_EUNSUPPORTED (`srf_stage_tail` answers its limits first, then nothing to
do, then the null pointers), a workspace too small SRF_EWORKSPACE -- all before any HIP call: the library loads and answers on a machine
without a GPU.  Every pointer handed in here is a made-up address that no kernel may ever see, so every call in this file ends in a
refusal or in a nothing-to-do SRF_OK (M == 0, P == 0, B == 0, R == 0, N == 0); none passes every check.  (The one test marked `gpu`
below brings real buffers: a workspace one byte short is refused after the device has been asked for.)"""
import ctypes

import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
PTR = ctypes.c_void_p(0x1000)        # never dereferenced: not a device address
LN = dict(ln1_g=PTR, ln1_b=PTR)


def linear(X=PTR, M=9, K=2048, ldx=None, W=PTR, N=128, ldw=None, bias=None, ln1_g=None, ln1_b=None, relu1=0, residual=None, ldr=0, ln2_g=None,
           ln2_b=None, relu2=0, Y=PTR, ldy=None, ws=PTR, ws_bytes=0):
    """The defaults are a split-K shape with ws_bytes = 0: a call that passes every other check still ends at SRF_EWORKSPACE, never in a
    launch.  No call here asks for M <= 8 without a row step: that route (the GEMV) has no workspace to stop it."""
    return _lib.lib().srf_linear(X, M, K, K if ldx is None else ldx, W, N, K if ldw is None else ldw, bias, ln1_g, ln1_b, 1e-5, relu1, residual,
                                 ldr, ln2_g, ln2_b, 1e-5, relu2, Y, N if ldy is None else ldy, ws, ws_bytes, None)


def need(M, N, K):
    return _lib.lib().srf_linear_workspace_bytes(M, N, K)


def test_linear_sizes_and_pitches():
    assert linear() == EWORKSPACE                                            # the base call: only the workspace stops it
    for kw in (dict(K=2046), dict(K=2049), dict(K=0), dict(K=-4), dict(N=0), dict(N=-1), dict(M=-1),
               dict(ldx=2050), dict(ldw=2054), dict(ldx=2044), dict(ldw=2044), dict(ldy=127), dict(ldy=0)):
        assert linear(**kw) == EINVAL, kw
        assert linear(**{**kw, "M": min(0, kw.get("M", 0))}) == EINVAL, kw   # the sizes come before the nothing-to-do answer
    assert linear(ldx=2052, ldw=2056, ldy=133) == EWORKSPACE                 # legal pitches


@pytest.mark.parametrize("kw", [dict(ln1_g=PTR), dict(ln1_b=PTR), dict(ln2_g=PTR), dict(ln2_b=PTR), dict(ln1_g=PTR, ln1_b=PTR, ln2_b=PTR)])
def test_linear_half_a_layernorm(kw):
    assert linear(**kw) == EINVAL
    assert linear(**kw, M=0) == EINVAL                                       # before the nothing-to-do answer


def test_linear_nothing_to_do_comes_before_the_null_pointers():
    assert linear(M=0) == OK
    assert linear(M=0, X=None, W=None, Y=None, ws=None) == OK
    assert linear(M=0, N=4096, **LN) == OK                                   # and before the limits
    for name in ("X", "W", "Y"):
        assert linear(**{name: None}) == EINVAL
        assert linear(**{name: None}, N=2048, **LN) == EINVAL                # null pointers before the limits


@pytest.mark.parametrize("kw", [LN, dict(ln2_g=PTR, ln2_b=PTR), dict(residual=PTR, ldr=1025), dict(relu2=1)])
@pytest.mark.parametrize("K,M", [(2048, 9), (128, 9), (128, 1), (2048, 1)])
def test_linear_row_steps_need_n_up_to_1024(kw, K, M):
    assert linear(N=1025, K=K, M=M, **kw) == EUNSUPPORTED
    assert linear(N=1025, K=K, M=M, **kw, ws_bytes=need(M, 1025, K)) == EUNSUPPORTED        # the limit before the workspace
    assert linear(N=1024, K=K, M=M, **kw, ws_bytes=need(M, 1024, K) - 1) == EWORKSPACE      # N = 1024 is inside: two passes


# every two-pass route (tests/test_gpu_linear_routes.py), one byte short: (M, K, N, row steps)
TWO_PASS = [(9, 132, 129, LN), (5, 36, 200, dict(relu2=1)), (9, 132, 1024, dict(residual=PTR, ldr=1024)),        # one slab, <16>
            (9, 2048, 10, {}), (9, 2052, 128, LN), (5, 2340, 10, LN), (1, 2048, 128, dict(relu2=1)),             # split-K, <2>
            (9, 2048, 129, {}), (9, 2340, 1024, LN), (5, 2048, 200, LN),                                         # split-K, <16>
            (9, 2048, 1028, {}), (9, 2048, 1100, dict(relu1=1, bias=PTR)), (33, 2340, 4096, {})]                 # split-K, columns


@pytest.mark.parametrize("M,K,N,kw", TWO_PASS)
def test_linear_workspace_one_byte_short(M, K, N, kw):
    nsplit = (K + 255) // 256 if K >= 2048 else 1
    assert need(M, N, K) == nsplit * M * N * 4
    assert linear(M=M, K=K, N=N, **kw, ws_bytes=need(M, N, K) - 1) == EWORKSPACE
    assert linear(M=M, K=K, N=N, **kw, ws=None, ws_bytes=need(M, N, K)) == EWORKSPACE       # a null workspace of the right size
    assert linear(M=M, K=K, N=N, **kw, ws_bytes=0) == EWORKSPACE


def test_linear_workspace_size():
    assert need(9, 128, 2044) == 9 * 128 * 4 and need(9, 128, 2048) == 8 * 9 * 128 * 4 and need(9, 128, 2052) == 9 * 9 * 128 * 4
    assert need(0, 128, 128) == 128 * 4


# ------------------------------------------------------------------------------------------------------------------- attention
def attention(qkv=PTR, B=1, P=17, E=128, H=8, out=PTR):
    return _lib.lib().srf_self_attention_batched(qkv, B, P, E, H, out, None)


def test_attention_codes():
    for kw in (dict(E=100, H=8), dict(E=128, H=3), dict(E=128, H=0), dict(E=0), dict(E=128, H=2), dict(E=264, H=8), dict(B=65536), dict(B=-1),
               dict(P=-1), dict(E=130, H=5)):
        assert attention(**kw) == EINVAL, kw                                  # E % H, head dim > 32, B beyond the grid, E % 4
        assert attention(**{**kw, "P": min(0, kw.get("P", 0))}) == EINVAL, kw   # before the nothing-to-do answer
    assert attention(P=0) == OK and attention(B=0) == OK and attention(P=0, qkv=None, out=None) == OK
    assert attention(P=0, E=64, H=8) == OK                                    # nothing to do comes before the head-dim table
    assert attention(qkv=None) == EINVAL and attention(out=None) == EINVAL
    for E, H in ((64, 8), (96, 8), (96, 4), (160, 8), (224, 8), (4, 1)):      # head dim 8, 12, 24, 20, 28, 4: a multiple of 4 up to 32, not 16 or 32
        assert attention(E=E, H=H) == EUNSUPPORTED, (E, H)
        assert attention(E=E, H=H, qkv=None) == EINVAL                        # null pointers before the table
    assert _lib.lib().srf_self_attention(PTR, 17, 64, 8, PTR, None) == EUNSUPPORTED
    assert _lib.lib().srf_self_attention(PTR, 0, 128, 8, PTR, None) == OK


# ------------------------------------------------------------------------------------------------------------------ DynamicConv
DYN_POINTERS = ["feats", "params", "g1", "b1", "g2", "b2", "out"]


def dynconv(feats=PTR, params=PTR, R=3, S=49, C=100, D=32, g1=PTR, b1=PTR, g2=PTR, b2=PTR, out=PTR):
    """C = 100 by default: a call that passes every other check ends at SRF_EUNSUPPORTED, never in a launch."""
    return _lib.lib().srf_dynconv_mid(feats, params, R, S, C, D, g1, b1, 1e-5, g2, b2, 1e-5, out, None)


def test_dynconv_codes():
    for kw in (dict(S=0), dict(S=65), dict(S=-1), dict(R=-1)):
        assert dynconv(**kw) == EINVAL, kw
        assert dynconv(**kw, C=128) == EINVAL and dynconv(**kw, C=256, D=64) == EINVAL
        assert dynconv(**{**kw, "R": min(0, kw.get("R", 0))}) == EINVAL, kw   # before the nothing-to-do answer
    assert dynconv(R=0) == OK and dynconv(R=0, C=128) == OK and dynconv(R=0, C=128, feats=None, out=None) == OK
    for name in DYN_POINTERS:
        assert dynconv(**{name: None}) == EINVAL
        assert dynconv(**{name: None}, C=128) == EINVAL and dynconv(**{name: None}, C=256, D=64) == EINVAL
    for C, D in ((128, 64), (256, 32), (64, 16), (128, 0), (0, 32), (132, 32), (512, 128), (100, 32)):
        for S in (1, 49, 64):
            assert dynconv(C=C, D=D, S=S) == EUNSUPPORTED, (C, D, S)


# --------------------------------------------------------------------------------------------------------------------- eSE gate
def ese(mean=PTR, N=9, C=256, W=PTR, bias=PTR, gate=PTR):
    """N = 9 by default: a call that passes every other check ends at SRF_EUNSUPPORTED (at most 8 rows per launch)."""
    return _lib.lib().srf_ese_gate(mean, N, C, W, bias, gate, None)


def test_ese_gate_codes():
    assert ese() == EUNSUPPORTED and ese(N=1000) == EUNSUPPORTED
    for kw in (dict(N=-1), dict(N=1, C=0), dict(N=1, C=-4), dict(N=1, C=6), dict(N=8, C=255), dict(N=0, C=2)):
        assert ese(**kw) == EINVAL, kw
    assert ese(N=0) == OK and ese(N=0, mean=None, W=None, gate=None) == OK
    for name in ("mean", "W", "gate"):
        assert ese(N=1, **{name: None}) == EINVAL and ese(N=8, **{name: None}) == EINVAL


# ------------------------------------------------------------------------------------------------------------------- stage tail
TAIL_POINTERS = ["obj_in", "w1", "b1", "w2", "b2", "n3_g", "n3_b", "wl", "bl", "wd", "bd", "boxes_m", "weights6", "pc_range", "obj_out", "logits",
                 "pred"]
HOST6 = _lib.hf([1.0] * 6)


def tail(R=10, C=128, F=512, n_cls=2, n_reg=3, ncls=10, Dd=10, ws=None, ws_bytes=0, **ptr):
    """obj_in is NULL by default: a call that passes the shape checks with R > 0 ends at SRF_EINVAL, never in a launch.  The tower arrays
    are host arrays the entry point reads only after every check here; NULL."""
    a = {name: PTR for name in TAIL_POINTERS}
    a.update(weights6=HOST6, pc_range=HOST6, obj_in=None)
    a.update(ptr)
    towers = (None, None, None, None)
    return _lib.lib().srf_stage_tail(a["obj_in"], R, C, F, a["w1"], a["b1"], a["w2"], a["b2"], a["n3_g"], a["n3_b"], 1e-5, n_cls, *towers,
                                     n_reg, *towers, a["wl"], a["bl"], ncls, a["wd"], a["bd"], Dd, a["boxes_m"], a["weights6"], a["pc_range"],
                                     5.0, a["obj_out"], a["logits"], a["pred"], ws, ws_bytes, None)


TAIL_OUTSIDE = [dict(C=64), dict(C=256), dict(F=100), dict(F=640), dict(F=0), dict(F=-128), dict(n_cls=5), dict(n_cls=-1), dict(n_reg=5),
                dict(n_reg=-1), dict(ncls=0), dict(ncls=33), dict(Dd=7), dict(Dd=33)]
TAIL_INSIDE = [dict(F=128), dict(F=256), dict(F=384), dict(F=512), dict(n_cls=0, n_reg=0), dict(n_cls=4, n_reg=4), dict(ncls=1), dict(ncls=32),
               dict(Dd=8), dict(Dd=32)]


def test_stage_tail_codes():
    for kw in TAIL_OUTSIDE:
        assert tail(**kw) == EUNSUPPORTED, kw
        assert tail(**kw, R=0) == EUNSUPPORTED, kw                                # the shapes come before the nothing-to-do answer
        assert tail(**kw, obj_in=PTR, w1=None) == EUNSUPPORTED, kw               # and before the null pointers
    assert tail(R=-1) == EUNSUPPORTED
    for kw in TAIL_INSIDE:
        assert tail(**kw, R=0) == OK, kw
        assert tail(**kw) == EINVAL, kw                                          # obj_in is NULL
    assert tail(R=0, **{name: None for name in TAIL_POINTERS}) == OK             # nothing to do comes before the null pointers
    for name in TAIL_POINTERS[1:]:
        assert tail(obj_in=PTR, **{name: None}) == EINVAL, name
        assert tail(obj_in=PTR, **{name: None}, ws=PTR, ws_bytes=0) == EINVAL, name      # null pointers before the workspace
    need = _lib.lib().srf_stage_tail_workspace_bytes
    assert need(200, 128, 512) == 4 * 200 * 128 * 4 and need(37, 128, 384) == 3 * 37 * 128 * 4 and need(0, 128, 512) == 0


def _stub_head(C, F, n_cls, n_reg, ncls, Dd, fuse=True):
    from types import SimpleNamespace as NS
    lin = lambda n: NS(weight=NS(shape=(n, C)))
    return NS(fuse_stage_tail=fuse, feat_channels_lidar=C, linear1_lidar=lin(F), cls_module_lidar=[None] * (3 * n_cls),
              reg_module_lidar=[None] * (3 * n_reg), class_logits_lidar=lin(ncls), bboxes_delta_lidar=lin(Dd))


def test_the_head_fuses_exactly_what_stage_tail_supports():
    """plugin/heads.py::_tail_fusable restates the limits of srf_stage_tail; the entry point answers R == 0 after its shape checks and before
    it touches a pointer.  (C, F, cls layers, reg layers, ncls, Dd) on both sides of every limit."""
    from srfdet3d_amd.plugin import heads
    base = dict(C=128, F=512, n_cls=2, n_reg=3, ncls=10, Dd=10)
    seen = set()
    for kw in TAIL_OUTSIDE + TAIL_INSIDE + [{}]:
        if any(v < 0 for v in kw.values()):
            continue                                                             # a module cannot have fewer than no layers or rows
        c = {**base, **kw}
        fusable = bool(heads._StageBase._tail_fusable(_stub_head(**c)))
        assert fusable == (tail(**c, R=0) == OK), c
        seen.add(fusable)
    assert seen == {True, False}
    assert not heads._StageBase._tail_fusable(_stub_head(**base, fuse=False))


@pytest.mark.gpu
@pytest.mark.parametrize("short", [1, 4])
def test_stage_tail_workspace_short_writes_nothing(dev, short):
    """With real buffers: a workspace `short` bytes short is SRF_EWORKSPACE and all three outputs keep the sentinel."""
    import decoder_ref as R
    params, boxes = R.stage_tail_inputs(37, 384, 1, 1, 3, 8, seed=3)
    d = R.stage_tail_device(params, boxes, dev)
    need = _lib.lib().srf_stage_tail_workspace_bytes(37, 128, 384)
    rc, *outs = R.call_stage_tail(d, R.GEOM, True, ws_bytes=need - short, sentinel=777.0)
    assert rc == EWORKSPACE and all((o == 777.0).all() for o in outs)


# ----------------------------------------------------------------------------------------------------- apply_deltas, dpg_mix
def deltas(d=None, boxes=PTR, R=9, Dd=10, weights6=HOST6, pc_range=HOST6, out=PTR):
    """deltas is NULL by default: a call that passes the other checks with R > 0 ends at SRF_EINVAL."""
    return _lib.lib().srf_apply_deltas(d, boxes, R, Dd, weights6, pc_range, 5.0, out, None)


def test_apply_deltas_codes():
    for kw in (dict(Dd=7), dict(Dd=0), dict(weights6=None), dict(pc_range=None), dict(R=-1)):
        assert deltas(**kw) == EINVAL, kw
        assert deltas(**{**kw, "R": min(0, kw.get("R", 0))}) == EINVAL, kw       # before the nothing-to-do answer
    assert deltas(R=0) == OK and deltas(R=0, boxes=None, out=None) == OK and deltas(R=0, Dd=8) == OK and deltas(R=0, Dd=64) == OK
    assert deltas() == EINVAL and deltas(d=PTR, boxes=None) == EINVAL and deltas(d=PTR, out=None) == EINVAL


def mix(wl=None, wi=None, B=2, E=4, P=200, boxes_w=PTR, D=10, feats_w=PTR, C=128, boxes=PTR, feats=PTR):
    """wl is NULL by default: a call that passes the size checks with B > 0 ends at SRF_EINVAL."""
    return _lib.lib().srf_dpg_mix(wl, wi, B, E, P, boxes_w, D, feats_w, C, boxes, feats, None)


def test_dpg_mix_codes():
    for kw in (dict(E=0), dict(E=17), dict(E=-1), dict(D=2), dict(P=0), dict(P=-1), dict(C=0), dict(B=-1)):
        assert mix(**kw) == EINVAL, kw
        assert mix(**kw, wl=PTR) == EINVAL, kw
        assert mix(**{**kw, "B": min(0, kw.get("B", 0))}) == EINVAL, kw          # before the nothing-to-do answer
    assert mix(B=0) == OK and mix(B=0, E=1, D=3, C=1) == OK and mix(B=0, E=16) == OK
    assert mix() == EINVAL                                                       # wl is NULL; wi may be
    for name in ("boxes_w", "feats_w", "boxes", "feats"):
        assert mix(wl=PTR, **{name: None}) == EINVAL, name


def test_all_are_declared_and_bound():
    assert {"srf_linear", "srf_linear_workspace_bytes", "srf_self_attention", "srf_self_attention_batched", "srf_dynconv_mid",
            "srf_ese_gate", "srf_stage_tail", "srf_stage_tail_workspace_bytes", "srf_apply_deltas", "srf_dpg_mix"} <= set(_lib.SIGNATURES)
