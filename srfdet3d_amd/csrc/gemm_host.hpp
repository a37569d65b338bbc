// gemm_host.hpp -- the host front of the four dense GEMM families: srf_conv1x1_nhwc / srf_conv_gemm_nhwc (conv.hip, operands staged
// through LDS), srf_conv1x1_nhwc_direct (gemm_direct.hip, LDS-free), srf_conv1x1_nhwc_split / srf_conv_gemm_nhwc_split (gemm_split.hip,
// bf16 split) and srf_conv1x1_nhwc_bf16 / srf_conv_gemm_nhwc_bf16 (gemm_bf16.hip, bf16 products).  What every family's entry points
// share lives here: the argument checks, the top-down / residual / pooled descriptors, the fill of the fields the four argument structs
// (GemmArgs, GdArgs, GsArgs, GbArgs) have in common, and the launch of the one pool-finish kernel.  gemm_tile128.hpp builds on it for
// the direct, split and bf16 families, which share one tile shape: their common argument fields, work-item decode, epilogue, launch
// function and entry-point bodies.  conv.hip keeps its own tile forms, grids and the mixed launch; every family keeps its K loop and
// its weight packing.
#pragma once
#include "common.hpp"

// what the checks need to know about a family
struct SrfGemmFamily {
    int tile_rows;   // rows of the tile behind the 32-bit range limit: ld * tile_rows * 4 bytes < 2^31
    bool y_range;    // the limit holds for y_ld as well as for x_ld (y is written through a buffer descriptor)
    int pool_rows;   // the pooled form wants a workspace of one column sum per block of this many rows
};

// the coarser level an FPN lateral convolution adds in its epilogue: rows are the pixels of an (N, mapH, mapW) map
struct SrfGemmTop {
    const float *top;
    long long top_ld;
    int mapH, mapW, topH, topW;
};

// the residual form's extra operand: an (M, res_ld) row-major matrix on the rows of y, added to the affine result BEFORE the ReLU
// (the identity of a ResNet bottleneck; the top-down form adds after it).  Read through a buffer descriptor over the rows of one tile.
struct SrfGemmRes {
    const float *res;
    long long res_ld;
};

// the pooled form's extra arguments
struct SrfGemmPool {
    long long HW;
    const float *mean;
    const void *workspace;
    size_t workspace_bytes;
};

static inline size_t srf_gemm_pool_bytes(int N, long long HW, int Cout, int pool_rows)
{
    return (size_t)N * (size_t)srf_ceil_div(HW, pool_rows) * Cout * 4;
}

// The plain (batch = M rows), top-down, pooled (batch = N images) and residual (batch = M rows) forms of every family.  Order: sizes (SRF_EINVAL), an empty batch
// (SRF_OK: the caller returns without a launch), null pointers (SRF_EINVAL), shape and alignment, then 32-bit ranges (SRF_EUNSUPPORTED),
// the workspace (SRF_EWORKSPACE).
static inline int srf_gemm_check_1x1(const SrfGemmFamily &f, long long batch, int K, long long x_ld, const void *x, const void *W_packed,
                                     int Cout, const void *y, long long y_ld, const SrfGemmTop *td = nullptr,
                                     const SrfGemmPool *pool = nullptr, const SrfGemmRes *rd = nullptr)
{
    if (batch < 0 || K <= 0 || Cout <= 0 || x_ld < K || y_ld < Cout) return SRF_EINVAL;
    if (td && (td->mapH <= 0 || td->mapW <= 0 || td->topH <= 0 || td->topW <= 0 || td->top_ld < Cout)) return SRF_EINVAL;
    if (pool && pool->HW <= 0) return SRF_EINVAL;
    if (rd && rd->res_ld < Cout) return SRF_EINVAL;
    if (batch == 0) return SRF_OK;
    if (!x || !W_packed || !y || (td && !td->top) || (pool && (!pool->mean || !pool->workspace)) || (rd && !rd->res)) return SRF_EINVAL;
    if ((K & 31) || (x_ld & 3) || ((uintptr_t)x & 15) || ((uintptr_t)W_packed & 15) || (pool && batch > 65535)) return SRF_EUNSUPPORTED;
    if (rd && ((rd->res_ld & 3) || ((uintptr_t)rd->res & 15))) return SRF_EUNSUPPORTED;
    if (x_ld * f.tile_rows * 4 >= (1ll << 31) || (f.y_range && y_ld * f.tile_rows * 4 >= (1ll << 31))) return SRF_EUNSUPPORTED;
    if (td && batch * td->topH * td->topW * td->top_ld >= (1ll << 31)) return SRF_EUNSUPPORTED;
    if (rd && rd->res_ld * f.tile_rows * 4 >= (1ll << 31)) return SRF_EUNSUPPORTED;   // the rows of one tile inside res's descriptor
    if (pool && pool->workspace_bytes < srf_gemm_pool_bytes((int)batch, pool->HW, Cout, f.pool_rows)) return SRF_EWORKSPACE;
    return SRF_OK;
}

// The implicit-im2col forms.  Same order; the output size and the extent of the input come back through Ho, Wo and x_bytes.
static inline int srf_gemm_check_conv(const SrfGemmFamily &f, int N, int H, int W, int Cin, long long x_ld, const void *x, const void *W_packed,
                                      int Cout, int kh, int kw, int stride, int pad, const void *y, long long y_ld, int *Ho, int *Wo,
                                      long long *x_bytes)
{
    if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || x_ld < Cin || y_ld < Cout)
        return SRF_EINVAL;
    if (N == 0) return SRF_OK;
    if (!x || !W_packed || !y) return SRF_EINVAL;
    if ((Cin & 31) || (x_ld & 3) || ((uintptr_t)x & 15) || ((uintptr_t)W_packed & 15)) return SRF_EUNSUPPORTED;
    // a kernel larger than the padded map has no output pixel.  Asked of the sizes, not of Ho: C's division rounds towards zero, so
    // (H + 2 pad - kh) / stride + 1 is 1 for a numerator of -1 and a stride >= 2, where the floor division of Conv2d gives 0
    if ((long long)H + 2ll * pad < kh || (long long)W + 2ll * pad < kw) return SRF_EINVAL;
    const long long ho = ((long long)H + 2ll * pad - kh) / stride + 1, wo = ((long long)W + 2ll * pad - kw) / stride + 1;
    if (ho >= (1ll << 31) || wo >= (1ll << 31)) return SRF_EUNSUPPORTED;   // a padding of 2^30 and more
    *Ho = (int)ho;
    *Wo = (int)wo;
    *x_bytes = (long long)N * H * W * x_ld * 4;
    if (*x_bytes >= (1ll << 31) || (f.y_range && y_ld * f.tile_rows * 4 >= (1ll << 31))) return SRF_EUNSUPPORTED;
    return SRF_OK;
}

// the fields GemmArgs, GdArgs, GsArgs and GbArgs share; the struct is value-initialised by the caller, which then adds its weight pointer and
// column-tile count
template <class Args>
static inline void srf_gemm_set_base(Args &a, const float *x, long long M, int K, long long x_ld, int Cout, const float *scale,
                                     const float *shift, int relu, float *y, long long y_ld)
{
    a.x = x;
    a.y = y;
    a.scale = scale;
    a.shift = shift;
    a.x_ld = x_ld;
    a.y_ld = y_ld;
    a.M = M;
    a.K = K;
    a.Cout = Cout;
    a.nchunk = K / 32;
    a.relu = relu;
}

// top-down fields (nearest upsampling by size, as F.interpolate: source = floor(destination * topH / mapH)); td == nullptr leaves the zeros
template <class Args>
static inline void srf_gemm_set_top(Args &a, const SrfGemmTop *td)
{
    if (!td) return;
    a.top = td->top;
    a.top_ld = td->top_ld;
    a.mapH = td->mapH;
    a.mapW = td->mapW;
    a.topH = td->topH;
    a.topW = td->topW;
    a.sy = (float)td->topH / (float)td->mapH;
    a.sx = (float)td->topW / (float)td->mapW;
}

// residual fields; rd == nullptr leaves the zeros
template <class Args>
static inline void srf_gemm_set_res(Args &a, const SrfGemmRes *rd)
{
    if (!rd) return;
    a.res = rd->res;
    a.res_ld = rd->res_ld;
}

// strided-convolution fields of the implicit im2col (GemmArgs, GsArgs, GbArgs)
template <class Args>
static inline void srf_gemm_set_conv(Args &a, int H, int W, int Ho, int Wo, int kw, int stride, int pad, int Cin, long long x_bytes)
{
    a.H = H;
    a.W = W;
    a.Ho = Ho;
    a.Wo = Wo;
    a.kw = kw;
    a.stride = stride;
    a.pad = pad;
    a.cin_chunks = Cin / 32;
    a.x_bytes = x_bytes;
}

// mean[n][c] = (sum over the bpi blocks of image n of partial[(n bpi + b) C + c]) / HW, in a fixed order.  The kernel is defined once,
// in conv.hip (the library is built one object per file, without relocatable device code).
__attribute__((visibility("hidden"))) int srf_gemm_pool_finish(const float *partial, int bpi, int N, int Cout, long long HW, float *mean,
                                                               hipStream_t stream);
