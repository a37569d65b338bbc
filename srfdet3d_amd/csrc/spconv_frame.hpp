// spconv_frame.hpp -- what the kernel forms of the sparse convolution share (spconv.hip: srf_spconv_fwd / srf_spconv_fwd_packed and
// their row plans; spconv_bf16.hip: srf_spconv_fwd_bf16): the offset limit, the XCD deal of the tiles, the live-row clamp of a
// static-shape level, the epilogue, the table from a layer shape to its kernels, and the common argument check of the three forward
// entry points.  Every form keeps its own K loop, staging, gather, LDS layout, weight packing and grid: this is a frame for what the
// forms share, not a merge of the forms.
#pragma once
#include "common.hpp"

#define SRF_KMAX 27   // kernel offsets of a layer (3 x 3 x 3): the size of every per-offset table in LDS and registers

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an L2).  Give every XCD one contiguous
// range of output tiles, so that the input rows its tiles gather (rows that are close in index are close in space)
// stay in that XCD's 4 MB L2 instead of being re-fetched through the fabric.  Bijective for any grid size.
__device__ __forceinline__ int srf_xcd_tile(int b, int n)
{
    const int q = n >> 3, r = n & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// Static-shape levels: the launch is sized by the capacity A_out, rows >= *rows_dev are padding; their tiles do nothing.
// rows_dev == NULL: every row is live.
__device__ __forceinline__ int srf_live_rows(int A_out, const int *__restrict__ rows_dev)
{
    if (rows_dev) {
        const int live = *rows_dev;
        A_out = A_out < live ? A_out : live;
    }
    return A_out;
}

// THE epilogue, on one f32 accumulator: y = fma(acc, alpha, beta) under `affine` (eval-BatchNorm), y += residual under `has_res`,
// y = max(y, 0) under `relu` -- in this order, each step one correctly rounded f32 operation (__fmaf_rn / __fadd_rn spelled out: the
// library is built without contraction, and oracle/srf_oracle.c:orc_spconv_fwd forms the same three steps).  This order and this
// spelling are the bit-exactness contract of the whole encoder; every kernel form calls this function per output element and states
// nothing of its own.  `res` is a callable that yields the element's residual -- a load from memory in the forms that fetch it here, a
// register in the forms that fetched theirs ahead -- and is called only under `has_res`, behind the fma, as the kernels always did.
template <class Res>
__device__ __forceinline__ float srf_spconv_epilogue(float acc, bool affine, float al, float be, bool has_res, Res &&res, int relu)
{
    if (affine) acc = __fmaf_rn(acc, al, be);
    if (has_res) acc = __fadd_rn(acc, res());
    if (relu) acc = acc > 0.0f ? acc : 0.0f;
    return acc;
}

// ---- the shape table: which (K, Cin, Cout) has which kernel and which row plan -------------------------------------------------------
//   Cin -> Cout        K      packed layout (srf_spconv_fwd_packed)   bf16 form (srf_spconv_fwd_bf16)     row plan (`tiles`)
//   16 / 32 -> 32      27     w32: srf_spconv_w32_k                    no                                 row order (srf_spconv_order_build)
//   32 / 64 -> 64      any    gs:  srf_spconv_gsp_k                    K = 27                             row ranges (srf_spconv_tiles_build)
//   64 / 128 -> 128    any    gs:  srf_spconv_gsp_k                    K = 27; 128 -> 128 also at K = 3   row ranges
// Every other shape has no packed form, no bf16 form and no plan (the *_packed_weight_bytes queries return 0, the pack and forward
// entry points SRF_EUNSUPPORTED) and runs on srf_spconv_fwd, which takes Cout = 16 (any Cin <= 512) and 32, 64, 128 (Cin a multiple of 4)
// and gives the same bits as the packed form.  The bf16 shapes are the ones the encoders run on the 64- / 128-channel kernel.
enum SrfPackedLayout { SRF_PACKED_NONE, SRF_PACKED_W32, SRF_PACKED_GS };
enum SrfPlanKind { SRF_PLAN_NONE, SRF_PLAN_ROWS, SRF_PLAN_ORDER };   // (the values srf_spconv_plan_kind returns)
struct SrfSpconvShape {
    SrfPackedLayout packed;
    bool bf16;
    SrfPlanKind plan;
};
static inline SrfSpconvShape srf_spconv_shape(int K, int Cin, int Cout)
{
    if (K <= 0 || K > SRF_KMAX) return {SRF_PACKED_NONE, false, SRF_PLAN_NONE};
    if (K == SRF_KMAX && Cout == 32 && (Cin == 16 || Cin == 32)) return {SRF_PACKED_W32, false, SRF_PLAN_ORDER};
    if ((Cout == 64 && (Cin == 32 || Cin == 64)) || (Cout == 128 && (Cin == 64 || Cin == 128)))
        return {SRF_PACKED_GS, K == SRF_KMAX || (K == 3 && Cin == 128 && Cout == 128), SRF_PLAN_ROWS};
    return {SRF_PACKED_NONE, false, SRF_PLAN_NONE};
}

// ---- the common argument check of srf_spconv_fwd, srf_spconv_fwd_packed and srf_spconv_fwd_bf16 -------------------------------------
// what differs between the three
struct SrfSpconvRules {
    bool shape_ok;   // the entry point has a kernel for (K, Cin, Cout); srf_spconv_fwd decides by Cout behind the checks and passes true
    bool quads;      // the kernels of Cout != 16 gather whole float4s: Cin a multiple of 4, an input with rows
    bool range32;    // the kernels gather through a buffer descriptor, 32-bit byte offsets: an input with rows, below 2 GiB
};

// Order: sizes (SRF_EINVAL), half an alpha / beta pair (SRF_EINVAL), a shape without the form (SRF_EUNSUPPORTED), no output row (SRF_OK:
// the caller returns without a launch), null pointers (SRF_EINVAL), what the kernels cannot address (SRF_EUNSUPPORTED) -- all before any
// HIP call.
static inline int srf_spconv_check(const SrfSpconvRules &f, const void *in, int A_in, int Cin, const void *W, int K, const void *nbr,
                                   int nbr_stride, int A_out, int Cout, const void *alpha, const void *beta, const void *out)
{
    if (A_in < 0 || A_out < 0 || Cin <= 0 || Cin > 512 || K <= 0 || K > SRF_KMAX || nbr_stride < A_out) return SRF_EINVAL;
    if ((alpha == nullptr) != (beta == nullptr)) return SRF_EINVAL;
    if (!f.shape_ok) return SRF_EUNSUPPORTED;
    if (A_out == 0) return SRF_OK;
    if (!in || !W || !nbr || !out) return SRF_EINVAL;
    if (f.quads && Cout != 16 && ((Cin & 3) || A_in == 0)) return SRF_EUNSUPPORTED;
    if (f.range32 && (A_in == 0 || (long long)A_in * Cin * 4 >= (1ll << 31))) return SRF_EUNSUPPORTED;
    return SRF_OK;
}
