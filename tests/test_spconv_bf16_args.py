"""Argument checks of the bf16-product sparse convolution (csrc/spconv_bf16.hip; no GPU): the shapes with that form, and the codes of a
defective call, which follow srf_spconv_fwd_packed and are all decided before any HIP call.

Every pointer is a fake address, so no row expects a launch: each call is either rejected or has no output row, and the module skips
itself where a GPU is present (there a call that passes the checks would hand the fake address to a kernel)."""
import pytest

from srfdet3d_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
P = 0x10000            # 16-byte aligned, never dereferenced
SRF_KMAX = 27
SHAPES = [(27, 32, 64), (27, 64, 64), (27, 64, 128), (27, 128, 128), (3, 128, 128)]
OTHER = [(27, 48, 64), (27, 32, 128), (27, 16, 32), (27, 32, 32), (3, 32, 32)]


@pytest.fixture(scope="module", autouse=True)
def L():
    lib = _lib.lib()
    if lib.srf_device_count() > 0:
        pytest.skip("a GPU is present: a fake address must never reach a kernel")
    return lib


def fwd(L, K=27, Cin=64, Cout=64, A_in=100, A_out=50, nbr_stride=50, inp=P, Wp=P, nbr=P, out=P, alpha=None, beta=None):
    return L.srf_spconv_fwd_bf16(inp, A_in, Cin, Wp, K, nbr, nbr_stride, A_out, Cout, alpha, beta, None, 0, out, None, None, None)


def test_the_byte_count_is_positive_for_exactly_the_five_shapes(L):
    for K, cin, cout in SHAPES:
        assert L.srf_spconv_bf16_packed_weight_bytes(K, cin, cout) == K * cin * cout * 2
        assert L.srf_spconv_packed_weight_bytes(K, cin, cout) > 0      # all of them shapes of the f32 packed kernel
    for K, cin, cout in OTHER + [(3, 64, 64), (9, 128, 128), (0, 64, 64), (27, 0, 64), (27, 64, 0), (-1, 64, 64), (28, 64, 64)]:
        assert L.srf_spconv_bf16_packed_weight_bytes(K, cin, cout) == 0, (K, cin, cout)


def test_pack_refuses_other_shapes_and_bad_arguments(L):
    pack = L.srf_spconv_bf16_pack_weights
    for K, cin, cout in OTHER:
        assert pack(P, K, cin, cout, P, None) == EUNSUPPORTED, (K, cin, cout)
    assert pack(None, 27, 64, 64, P, None) == EINVAL
    assert pack(P, 27, 64, 64, None, None) == EINVAL
    assert pack(P, SRF_KMAX + 1, 64, 64, P, None) == EINVAL
    assert pack(P, 0, 64, 64, P, None) == EINVAL
    assert pack(None, 27, 48, 64, P, None) == EINVAL                 # the null pointer before the shape


def test_forward_refuses_other_shapes(L):
    for K, cin, cout in OTHER:
        assert fwd(L, K=K, Cin=cin, Cout=cout) == EUNSUPPORTED, (K, cin, cout)
        assert fwd(L, K=K, Cin=cin, Cout=cout, A_out=0, nbr_stride=0) == EUNSUPPORTED    # the shape before the empty output


def test_forward_bad_arguments(L):
    for K, cin, cout in SHAPES:
        kw = dict(K=K, Cin=cin, Cout=cout)
        assert fwd(L, inp=None, **kw) == EINVAL
        assert fwd(L, Wp=None, **kw) == EINVAL
        assert fwd(L, nbr=None, **kw) == EINVAL
        assert fwd(L, out=None, **kw) == EINVAL
        assert fwd(L, nbr_stride=49, **kw) == EINVAL
        assert fwd(L, alpha=P, **kw) == EINVAL and fwd(L, beta=P, **kw) == EINVAL    # alpha without beta and the reverse
        assert fwd(L, A_in=-1, **kw) == EINVAL and fwd(L, A_out=-1, **kw) == EINVAL
    assert fwd(L, K=SRF_KMAX + 1) == EINVAL and fwd(L, K=0) == EINVAL
    assert fwd(L, K=SRF_KMAX + 1, inp=None) == EINVAL


def test_no_output_row_is_ok_and_an_empty_or_huge_input_is_unsupported(L):
    for K, cin, cout in SHAPES:
        kw = dict(K=K, Cin=cin, Cout=cout)
        assert fwd(L, A_out=0, nbr_stride=0, **kw) == OK
        assert fwd(L, A_out=0, nbr_stride=0, inp=None, Wp=None, nbr=None, out=None, **kw) == OK   # nothing is touched
        assert fwd(L, A_in=0, **kw) == EUNSUPPORTED
        rows_2gib = (1 << 31) // (cin * 4)
        assert fwd(L, A_in=rows_2gib, **kw) == EUNSUPPORTED
        assert fwd(L, A_in=rows_2gib, inp=None, **kw) == EINVAL       # the null pointer before the range
