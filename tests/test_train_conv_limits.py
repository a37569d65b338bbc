"""The shape limits of the training convolutions as functions of integers: the kernels' own (srfdet3d_amd/ops.py, beside their
wrappers) and what a layer of srfdet3d_amd/train_conv.py adds.  Every row carries its verdict and where that verdict comes from: a
line of csrc/, or the expression the predicates of train_conv.py held before the limits were written once.  CPU only."""
import pytest

from srfdet3d_amd import ops, train_conv

P30, P31 = 1 << 30, 1 << 31

# (function, arguments, verdict, reason)
WINO43 = [
    (ops.wino43_channels_ok, (24, 32), True, "24 % 8 == 0: the kernel packs Cin / 8 chunks (csrc/wino43.hip:461)"),
    (ops.wino43_channels_ok, (36, 32), False, "36 & 7: srf_wino43_packed_weight_bytes answers 0 (csrc/wino43.hip:461)"),
    (ops.wino43_channels_ok, (32, 32), True, "csrc/wino43.hip:461, :402"),
    (ops.wino43_channels_ok, (32, 1028), True, "1028 % 4 == 0: whole output quads (csrc/wino43.hip:402)"),
    (ops.wino43_channels_ok, (32, 1030), False, "a quad of output channels would straddle Cout (csrc/wino43.hip:402)"),
    (ops.wino43_range_ok, (P30 - 5, 1), True, "4 * (2^30 - 5) = 2^32 - 20 < 0xFFFFFFF0 (csrc/wino43.hip:561)"),
    (ops.wino43_range_ok, (P30 - 4, 1), False, "4 * (2^30 - 4) = 2^32 - 16 = 0xFFFFFFF0: refused (csrc/wino43.hip:561)"),
    (ops.wino43_range_ok, (1 << 20, 1 << 10), False, "4 GB"),
    (ops.wino43_tiles_ok, (1, 4, 4 * (P31 - 65)), True, "2^31 - 65 tiles < (1 << 31) - 64, the wrapper's bound"),
    (ops.wino43_tiles_ok, (1, 4, 4 * (P31 - 64)), False, "2^31 - 64 tiles: the wrapper's bound (the kernel's own is 2^31 - 32, csrc/wino43.hip:546)"),
    (ops.wino43_tiles_ok, (1, 5, 4 * ((P31 - 64) // 2)), False, "H = 5 is two rows of tiles: ceil, not floor (csrc/wino43.hip:537-539)"),
    # a layer of `_Wino43Conv`: `eligible` held Cin % 8, Cout % 8, Cin >= 32 and N H W max(Cin, Cout) 4 < (1 << 32) - 16
    (train_conv.wino_layer_ok, (2, 8, 8, 24, 32), False, "Cin >= 32 (`eligible`)"),
    (train_conv.wino_layer_ok, (2, 8, 8, 36, 32), False, "Cin % 8 (`eligible`; csrc/wino43.hip:461)"),
    (train_conv.wino_layer_ok, (2, 8, 8, 32, 32), True, "`eligible`"),
    (train_conv.wino_layer_ok, (2, 8, 8, 32, 1024), True, "`eligible` has no upper bound on Cout"),
    (train_conv.wino_layer_ok, (2, 8, 8, 32, 1028), False, "Cout % 8 (`eligible`): Cout is the data gradient's Cin"),
    (train_conv.wino_layer_ok, (2, 8, 8, 32, 1032), True, "`eligible` has no upper bound on Cout"),
    (train_conv.wino_layer_ok, (1, 1, (1 << 25) - 1, 32, 32), True, "128 (2^25 - 1) = 2^32 - 128 < (1 << 32) - 16"),
    (train_conv.wino_layer_ok, (1, 1, 1 << 25, 32, 32), False, "128 * 2^25 = 2^32"),
    (train_conv.wino_layer_ok, (1, 1, 1 << 25, 32, 24), False, "the wider of Cin and Cout counts"),
    # a layer of `_ConvAffineRelu` / `_OSAChain`: Cout <= 1024 (csrc/nhwc.hip:592) and the tile count on top
    (train_conv.fused_layer_ok, (3, 2, 8, 8, 32, 1024), True, "`fused_eligible`: Cout <= 1024"),
    (train_conv.fused_layer_ok, (3, 2, 8, 8, 32, 1032), False, "`fused_eligible`: Cout <= 1024, srf_nhwc_affine_relu_bwd's C (csrc/nhwc.hip:592)"),
    (train_conv.fused_layer_ok, (3, 2, 8, 8, 24, 32), False, "Cin >= 32"),
    (train_conv.fused_layer_ok, (5, 2, 8, 8, 32, 32), False, "3x3 and 1x1 only"),
]

GEMM = [
    (ops.gemm_k_ok, (48,), False, "srf_gemm_check_1x1: K & 31 (csrc/gemm_host.hpp)"),
    (ops.gemm_k_ok, (32,), True, "srf_gemm_check_1x1: K & 31 (csrc/gemm_host.hpp)"),
    (ops.gemm_k_ok, (1056,), True, "33 * 32"),
    (ops.gemm_rows_ok, ((1 << 22) - 1,), True, "128 rows x (2^22 - 1) floats x 4 B < 2^31 (srf_gemm_check_1x1: x_ld * f.tile_rows * 4 >= 2^31, csrc/gemm_host.hpp)"),
    (ops.gemm_rows_ok, (1 << 22,), False, "128 rows x 2^22 floats x 4 B = 2^31 (srf_gemm_check_1x1: x_ld * f.tile_rows * 4 >= 2^31, csrc/gemm_host.hpp)"),
    (ops.below_2gb, ((1 << 29) - 1, 1), True, "4 (2^29 - 1) < 2^31 (csrc/wgrad.hip:337; srf_gemm_check_conv: *x_bytes >= 2^31, csrc/gemm_host.hpp)"),
    (ops.below_2gb, (1 << 29, 1), False, "4 * 2^29 = 2^31 (csrc/wgrad.hip:337; srf_gemm_check_conv: *x_bytes >= 2^31, csrc/gemm_host.hpp)"),
    # a 1x1 layer on the GEMMs in three directions: the predicates held Cin % 32, Cout % 32, Cout <= 1024, H W > 1 and
    # N H W max(Cin, Cout) 512 < (1 << 31) 128
    (train_conv.gemm_layer_ok, (2, 8, 8, 32, 32), True, "`fused_eligible`, `conv2d`"),
    (train_conv.gemm_layer_ok, (2, 8, 8, 48, 32), False, "K = 48 forward (srf_gemm_check_1x1: K & 31, csrc/gemm_host.hpp)"),
    (train_conv.gemm_layer_ok, (2, 8, 8, 32, 48), False, "K = 48 in the data gradient (srf_gemm_check_1x1: K & 31, csrc/gemm_host.hpp)"),
    (train_conv.gemm_layer_ok, (2, 8, 8, 32, 1024), True, "Cout <= 1024"),
    (train_conv.gemm_layer_ok, (2, 8, 8, 32, 1056), False, "Cout <= 1024 (`fused_eligible`, `conv2d`)"),
    (train_conv.gemm_layer_ok, (1, 1 << 12, (1 << 12) - 1, 32, 32), True, "(2^24 - 2^12) 32 512 < 2^31 128"),
    (train_conv.gemm_layer_ok, (1, 1 << 12, 1 << 12, 32, 32), False, "2^24 * 32 * 512 = 2^31 * 128: 2 GB (csrc/wgrad.hip:337)"),
    (train_conv.gemm_layer_ok, (1, 1 << 12, 1 << 11, 32, 64), False, "the wider of Cin and Cout counts"),
    (train_conv.gemm_layer_ok, (2, 1, 1, 32, 32), False, "H W > 1 (`eligible_1x1`, `osa_eligible`)"),
    (train_conv.gemm_layer_ok, (2, 1, 2, 32, 32), True, "H W = 2"),
    (train_conv.fused_layer_ok, (1, 2, 8, 8, 32, 32), True, "the 1x1 form of a fused layer is `gemm_layer_ok`"),
    (train_conv.fused_layer_ok, (1, 2, 1, 1, 32, 32), False, "H W > 1"),
]


@pytest.mark.parametrize("fn,args,want,why", WINO43 + GEMM, ids=[f"{r[0].__name__}{r[1]}" for r in WINO43 + GEMM])
def test_limit(fn, args, want, why):
    assert fn(*args) is want, why


def test_the_two_spellings_of_2_gb_are_one():
    """`N H W C 512 < (1 << 31) 128`, as the predicates wrote it, is `4 N H W C < 1 << 31` for integers."""
    for p in ((1 << 24) - 1, 1 << 24, (1 << 24) + 1):
        assert (p * 32 * 512 < (1 << 31) * 128) is ops.below_2gb(p, 32)
