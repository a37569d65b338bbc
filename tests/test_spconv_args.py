"""Return codes of the three forward entry points of the sparse convolution (`srf_spconv_fwd`, `srf_spconv_fwd_packed`,
`srf_spconv_fwd_bf16`) and of the two weight packers, in the order the common check of csrc/spconv_frame.hpp decides them: sizes
SRF_EINVAL, half an alpha / beta pair SRF_EINVAL, a shape without the form SRF_EUNSUPPORTED, no output row SRF_OK, null pointers
SRF_EINVAL, an input the kernels cannot address SRF_EUNSUPPORTED -- all before any HIP call, so the library answers on a machine without
a GPU.  The codes are the ones the entry points returned while each of them spelled the checks out itself.

Every pointer handed in is a made-up address that no kernel may ever see: every call in this file ends in a refusal or in the
nothing-to-do SRF_OK of A_out == 0; none passes every check.  The base call of each entry point is stopped by its LAST check (an input
without rows), so a row of the table that leaves the base's code unchanged has passed everything in front of it."""
import ctypes

import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
PTR = ctypes.c_void_p(0x10000)       # never dereferenced: not a device address
FWD, PACKED, BF16 = "srf_spconv_fwd", "srf_spconv_fwd_packed", "srf_spconv_fwd_bf16"
ENTRIES = (FWD, PACKED, BF16)
GIB2_ROWS = (1 << 31) // (64 * 4)    # rows of a 64-channel input of exactly 2 GiB


def call(entry, inp=PTR, A_in=0, Cin=64, W=PTR, K=27, nbr=PTR, nbr_stride=50, A_out=50, Cout=64, alpha=None, beta=None, out=PTR):
    """The defaults are a (27, 64, 64) layer -- a shape of all three entry points -- whose input has no rows: what stops it is the last
    check of each (the float4 rule of srf_spconv_fwd, the descriptor rule of the other two)."""
    L = _lib.lib()
    a = (inp, A_in, Cin, W, K, nbr, nbr_stride, A_out, Cout, alpha, beta, None, 0, out, None)
    return L.srf_spconv_fwd(*a, None) if entry == FWD else getattr(L, entry)(*a, None, None)


ALL = lambda code: {e: code for e in ENTRIES}
EMPTY = dict(A_out=0, nbr_stride=0)
NULLS = dict(inp=None, W=None, nbr=None, out=None)
# (what the row shows, arguments, code per entry point)
TABLE = [
    ("base: only the last check stops it", {}, ALL(EUNSUPPORTED)),
    # 1. sizes -- in front of everything, the nothing-to-do answer and an unknown shape included
    *[(f"sizes {kw}", kw, ALL(EINVAL)) for kw in (dict(A_in=-1), dict(A_out=-1), dict(Cin=0), dict(Cin=-4), dict(Cin=513), dict(K=0), dict(K=-1),
                                                  dict(K=28), dict(nbr_stride=49), dict(nbr_stride=0))],
    ("sizes before the empty output", dict(K=28, **EMPTY), ALL(EINVAL)),
    ("sizes before the empty output", dict(Cin=513, **EMPTY), ALL(EINVAL)),
    ("sizes before the shape", dict(K=0, Cout=48), ALL(EINVAL)),
    ("Cin = 512 is a legal size", dict(Cin=512), {FWD: EUNSUPPORTED, PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    # 2. the alpha / beta pair
    ("alpha without beta", dict(alpha=PTR), ALL(EINVAL)),
    ("beta without alpha", dict(beta=PTR), ALL(EINVAL)),
    ("the pair before the empty output", dict(alpha=PTR, **EMPTY), ALL(EINVAL)),
    ("the pair before the shape", dict(beta=PTR, Cout=48), ALL(EINVAL)),
    ("a whole pair passes", dict(alpha=PTR, beta=PTR), ALL(EUNSUPPORTED)),
    # 3. the shape: the packed and the bf16 entry refuse it before the empty output, srf_spconv_fwd has no shape table in front of it
    ("no form, before the empty output", dict(Cout=48, **EMPTY), {FWD: OK, PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    ("no form, before the null pointers", dict(Cout=48, A_in=100, **NULLS), {FWD: EINVAL, PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    ("a packed shape without a bf16 form", dict(Cin=32, Cout=32, **EMPTY), {FWD: OK, PACKED: OK, BF16: EUNSUPPORTED}),
    ("a packed shape without a bf16 form", dict(K=3, **EMPTY), {FWD: OK, PACKED: OK, BF16: EUNSUPPORTED}),
    ("the 32-channel layout exists at K = 27 only", dict(K=9, Cin=32, Cout=32, **EMPTY), {FWD: OK, PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    # 4. no output row: nothing is touched
    ("empty output", EMPTY, ALL(OK)),
    ("empty output, before the null pointers", dict(**EMPTY, **NULLS), ALL(OK)),
    ("empty output, before the 2 GiB input", dict(A_in=GIB2_ROWS, **EMPTY), ALL(OK)),
    ("empty output under a wider table", dict(A_out=0, nbr_stride=50), ALL(OK)),
    # 5. null pointers -- in front of the addressing rules
    *[(f"null {name}", {name: None, "A_in": 100}, ALL(EINVAL)) for name in ("inp", "W", "nbr", "out")],
    ("null before the 2 GiB input", dict(inp=None, A_in=GIB2_ROWS), ALL(EINVAL)),
    ("null before the float4 rule", dict(out=None, Cin=5, Cout=32, A_in=100), {FWD: EINVAL, PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    # 6. what the kernels cannot address: 32-bit buffer offsets (packed, bf16); whole float4s of an input with rows (srf_spconv_fwd, Cout != 16)
    ("an input of 2 GiB", dict(A_in=GIB2_ROWS), {PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    ("an input of 2 GiB, 128 channels", dict(A_in=GIB2_ROWS // 2, Cin=128, Cout=128), {PACKED: EUNSUPPORTED, BF16: EUNSUPPORTED}),
    ("Cin no multiple of 4", dict(Cin=6, Cout=32, A_in=100), {FWD: EUNSUPPORTED}),
    ("an output width without a kernel", dict(Cout=256, A_in=100), ALL(EUNSUPPORTED)),
    ("an output width without a kernel", dict(Cout=48, A_in=100), ALL(EUNSUPPORTED)),
]


@pytest.mark.parametrize("entry", ENTRIES)
def test_forward_codes_in_the_order_of_the_common_check(entry):
    for what, kw, want in TABLE:
        if entry in want:
            assert call(entry, **kw) == want[entry], (entry, what, kw)


# (what, (W, K, Cin, Cout, packed), code of srf_spconv_pack_weights, of srf_spconv_bf16_pack_weights); a shape WITH the form and both
# pointers would be packed, so no such row
PACK_TABLE = [
    ("null W", (None, 27, 64, 64, PTR), EINVAL, EINVAL),
    ("null packed", (PTR, 27, 64, 64, None), EINVAL, EINVAL),
    ("K = 0", (PTR, 0, 64, 64, PTR), EINVAL, EINVAL),
    ("K = 28", (PTR, 28, 64, 64, PTR), EINVAL, EINVAL),
    ("Cin = 0", (PTR, 27, 0, 64, PTR), EINVAL, EINVAL),
    ("Cout = 0", (PTR, 27, 64, 0, PTR), EINVAL, EINVAL),
    ("the null pointer before the shape", (None, 27, 48, 64, PTR), EINVAL, EINVAL),
    ("no form", (PTR, 27, 48, 64, PTR), EUNSUPPORTED, EUNSUPPORTED),
    ("no form", (PTR, 27, 32, 128, PTR), EUNSUPPORTED, EUNSUPPORTED),
    ("no form", (PTR, 27, 16, 16, PTR), EUNSUPPORTED, EUNSUPPORTED),
    ("the 32-channel layout exists at K = 27 only", (PTR, 3, 32, 32, PTR), EUNSUPPORTED, EUNSUPPORTED),
    ("Cin = 513 is no size error of a packer", (PTR, 27, 513, 64, PTR), EUNSUPPORTED, EUNSUPPORTED),
]


def test_pack_codes():
    L = _lib.lib()
    for what, a, want32, want16 in PACK_TABLE:
        assert L.srf_spconv_pack_weights(*a, None) == want32, (what, a)
        assert L.srf_spconv_bf16_pack_weights(*a, None) == want16, (what, a)


def test_no_row_of_the_tables_can_reach_a_launch():
    """a call launches only with four pointers, A_out > 0 and a passing last check; the tables hold none"""
    L = _lib.lib()
    for what, kw, want in TABLE:
        assert all(code != OK or kw.get("A_out", 50) == 0 for code in want.values()), what
    for what, (W, K, cin, cout, packed), _, _ in PACK_TABLE:
        assert W is None or packed is None or not 0 < K <= 27 or cin <= 0 or cout <= 0 or (
            L.srf_spconv_packed_weight_bytes(K, cin, cout) == 0 and L.srf_spconv_bf16_packed_weight_bytes(K, cin, cout) == 0), what
