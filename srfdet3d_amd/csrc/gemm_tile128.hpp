// gemm_tile128.hpp -- the frame the direct (gemm_direct.hip), split (gemm_split.hip) and bf16 (gemm_bf16.hip) GEMM kernels share around
// their K loops.  All three use one workgroup shape: a tile of 128 rows x 128 channels, four waves as 2 x 2 wave tiles of 64 x 64, and
// acc[2][2] of 16 floats per lane (the 32 x 32 MFMA layout: lane = channel li of block j, register r = row (r & 3) + 8 (r >> 2) + 4 lh of
// block i).  Stated once here:
//   * SrfTile128Args: the argument fields the frame reads.  GdArgs and GsArgs derive from it and add their own (the conv fields); GbArgs
//     has the same fields under the same names in a struct of its own (gemm_bf16.hip says why);
//   * srf_tile128_row_block, srf_tile128_item: blockIdx.x -> (column tile, row block), the per-image row tiling of the pooled form;
//   * srf_tile128_epilogue (its fields: SrfTile128Epi): scale / shift, the residual add, the ReLU, the top-down add, the stores through
//     y's descriptor and the column sums of the pooled form.  The direct and the split kernels call it; the bf16 kernels keep a copy
//     without the residual form, so a new epilogue form is written here and, if the bf16 family is to have it, there;
//   * srf_tile128_launch and one body for each kind of entry point (plain, residual, top-down, pooled, implicit im2col), templated on a
//     family description F: F::Args, F::limits (SrfGemmFamily), the kernel of each form (F::plain, F::pool, F::topdown, F::resid, F::conv;
//     nullptr where the family has none) and F::set_weights.  All three families use them.
// Each family's file keeps its K loop, its weight packing and its extern "C" entry points, which forward to the bodies here.  The
// library is built one object per file without relocatable device code: everything here is static inline / __device__ __forceinline__.
// The LDS family of conv.hip (other tile shapes, the mixed launch, plain stores) is not a user.
#pragma once
#include "common.hpp"
#include "gemm_host.hpp"

template <class WPtr>
struct SrfTile128Args {
    const float *x;
    float *y;
    WPtr Wp;   // the family's packed weights: third, where every family had it (another kernel-argument layout changes the scalar loads)
    const float *scale, *shift;
    long long x_ld, y_ld, M;
    int K, Cout, nchunk, nct, relu;   // nchunk: chunks of 32 channels (K / 32); nct: column tiles of 128
    long long mblocks;
    // per-image row tiling + column sums of the stored outputs (eSE pooling): bpi > 0: image n owns row blocks [n bpi, (n + 1) bpi)
    float *colsum;
    long long HW;
    int bpi;
    // FPN top-down step in the epilogue (as srf_conv1x1_nhwc_topdown): y += top[n][floor(py sy)][floor(px sx)][co]; rows are the
    // pixels (n, py, px) of an (N, mapH, mapW) map
    const float *top;
    long long top_ld;
    int mapH, mapW, topH, topW;
    float sy, sx;
    // residual form: y = act(fl(fma(acc, scale, shift)) + res[row][co]), the add BEFORE the ReLU (as srf_conv1x1_nhwc_residual)
    const float *res;
    long long res_ld;
};

// the work item of a workgroup: column tile ct, rows [p0, p0 + rows_here) of x and y (rows_blk = rows from p0 to the end of the matrix
// or, pooled, of the image), and the row block's slot in the column-sum workspace
struct SrfTile128Item {
    int ct;
    long long p0, rows_blk, rows_here, slot;
};

// The device functions below take the fields they read as values (the epilogue: SRF_TILE128_EPI(a)), never a reference to the kernel's
// argument struct.  A reference keeps the whole struct in memory until the call is inlined, which is after the first scalar-replacement
// pass, and the K loops then compile to other code: srf_gemm_bf16_k<GB_CONV> guarded its implicit-im2col loads with branches instead of
// selects and every bf16 kernel changed the address arithmetic of its weight loads.

// work item -> (column tile, row block): items b and b + 8 share an XCD, the column tiles of a row block sit on one L2.  Returns the
// row block; one that is >= mblocks is past the grid (the grid is rounded up to whole groups of 8 row blocks) and the kernel returns.
__device__ __forceinline__ long long srf_tile128_row_block(int nct, int &ct)
{
    const int xcd = blockIdx.x & 7, jq = blockIdx.x >> 3;
    ct = jq % nct;
    return (long long)(jq / nct) * 8 + xcd;
}

// the rows of row block mb of an (M, .) matrix; POOL: the row blocks are counted per image of HW rows, bpi to an image
template <bool POOL>
__device__ __forceinline__ SrfTile128Item srf_tile128_item(int ct, long long mb, long long M, long long HW, int bpi)
{
    long long p0 = mb * 128, rows_blk = M - p0;
    long long slot = mb;
    if (POOL) {
        const long long n = mb / bpi, lb = mb - n * bpi;
        p0 = n * HW + lb * 128;
        rows_blk = HW - lb * 128;
        slot = n * bpi + lb;
    }
    return {ct, p0, rows_blk, rows_blk < 128 ? rows_blk : 128, slot};
}

// what the epilogue reads of SrfTile128Args, by value
struct SrfTile128Epi {
    float *y;
    const float *scale, *shift;
    long long y_ld, M;
    int Cout, relu;
    float *colsum;
    const float *top;
    long long top_ld;
    int mapH, mapW, topH, topW;
    float sy, sx;
    const float *res;
    long long res_ld;
};
// by name, so that a field added to one struct and not the other, or in another place, cannot go unnoticed
#define SRF_TILE128_EPI(a)                                                                                                               \
    ({                                                                                                                                   \
        SrfTile128Epi e_ = {};                                                                                                           \
        e_.y = (a).y, e_.scale = (a).scale, e_.shift = (a).shift, e_.y_ld = (a).y_ld, e_.M = (a).M, e_.Cout = (a).Cout;                  \
        e_.relu = (a).relu, e_.colsum = (a).colsum, e_.top = (a).top, e_.top_ld = (a).top_ld, e_.mapH = (a).mapH, e_.mapW = (a).mapW;    \
        e_.topH = (a).topH, e_.topW = (a).topW, e_.sy = (a).sy, e_.sx = (a).sx, e_.res = (a).res, e_.res_ld = (a).res_ld;                \
        e_;                                                                                                                              \
    })
static_assert(sizeof(SrfTile128Epi) == 112, "a field added to SrfTile128Epi is also copied in SRF_TILE128_EPI");

// The epilogue of thread tid = (wave (wm, wn), lane (li, lh)).  `scratch` is LDS the workgroup may overwrite at this point: 128 ints
// (TOPDOWN) or 256 floats (POOL); unused otherwise.
template <bool POOL, bool TOPDOWN, bool RESID, class Acc>
__device__ __forceinline__ void srf_tile128_epilogue(const SrfTile128Epi a, const Acc (&acc)[2][2], const SrfTile128Item &it, void *scratch,
                                                     int tid, int li, int lh, int wm, int wn)
{
    const int ct = it.ct;
    const long long p0 = it.p0, rows_blk = it.rows_blk, rows_here = it.rows_here;
    float sc[2], sh[2];
    bool co_ok[2];
    const int co0 = ct * 128 + wn * 64 + li;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = co0 + j * 32;
        co_ok[j] = co < a.Cout;
        sc[j] = (co_ok[j] && a.scale) ? a.scale[co] : 1.f;
        sh[j] = (co_ok[j] && a.shift) ? a.shift[co] : 0.f;
    }
    __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(a.y + p0 * a.y_ld, 0, (int)(rows_here * a.y_ld * 4), 0x00020000);
    const int row_base = wm * 64 + 4 * lh;
    unsigned ybase[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) ybase[j] = co_ok[j] ? (unsigned)((row_base * a.y_ld + co0 + j * 32) * 4) : 0x80000000u;
    const unsigned yrow_b = (unsigned)(a.y_ld * 4);
    const long long rows_left = rows_blk - row_base;
    int *s_top = reinterpret_cast<int *>(scratch);   // [128]: offset (floats) of the top-level pixel each row of this block adds
    if (TOPDOWN) {
        if (tid < 128) {
            const long long row = p0 + tid;
            int off = 0;
            if (row < a.M) {
                const int hw = a.mapH * a.mapW;
                const int n = (int)(row / hw), rem = (int)(row - (long long)n * hw);
                const int yy = rem / a.mapW, xx = rem - yy * a.mapW;
                int ys = (int)floorf((float)yy * a.sy), xs = (int)floorf((float)xx * a.sx);
                if (ys > a.topH - 1) ys = a.topH - 1;
                if (xs > a.topW - 1) xs = a.topW - 1;
                off = (int)((((long long)n * a.topH + ys) * a.topW + xs) * a.top_ld);
            }
            s_top[tid] = off;
        }
        __syncthreads();
    }
    float csum[2] = {0.f, 0.f};
    // RESID: the residual of this block's rows through a descriptor of its own (a row past the block and a channel past Cout read as
    // zero and are never stored); the 32 values of a row block are requested together, ahead of the stores they feed
    __amdgpu_buffer_rsrc_t rr;
    unsigned rbase[2] = {0u, 0u}, rrow_b = 0;
    if (RESID) {
        rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.res) + p0 * a.res_ld, 0, (int)(rows_here * a.res_ld * 4), 0x00020000);
#pragma unroll
        for (int j = 0; j < 2; ++j) rbase[j] = co_ok[j] ? (unsigned)((row_base * a.res_ld + co0 + j * 32) * 4) : 0x80000000u;
        rrow_b = (unsigned)(a.res_ld * 4);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float rv[RESID ? 16 : 1][RESID ? 2 : 1];
        if (RESID) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    rv[r][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rr, (int)(rbase[j] + (unsigned)(i * 32 + (r & 3) + 8 * (r >> 2)) * rrow_b), 0, 0));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dr = i * 32 + (r & 3) + 8 * (r >> 2);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float v = __fmaf_rn(acc[i][j][r], sc[j], sh[j]);
                if (RESID) v = __fadd_rn(v, rv[r][j]);
                if (a.relu) v = fmaxf(v, 0.f);
                if (TOPDOWN && co_ok[j]) v = __fadd_rn(v, a.top[s_top[row_base + dr] + co0 + j * 32]);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yr, (int)(ybase[j] + (unsigned)dr * yrow_b), 0, 0);
                if (POOL) csum[j] += dr < rows_left ? v : 0.f;
            }
        }
    }
    if (POOL) {
        // column sums of the block: the two lane halves of a wave (shuffle), then the two waves that share the columns (LDS), in a
        // fixed order: reproducible bit for bit
        float *red = reinterpret_cast<float *>(scratch);   // [2][128]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float o = __shfl_xor(csum[j], 32);
            if (lh == 0) red[wm * 128 + wn * 64 + j * 32 + li] = csum[j] + o;
        }
        __syncthreads();
        if (tid < 128) {
            const int co = ct * 128 + tid;
            if (co < a.Cout) a.colsum[it.slot * a.Cout + co] = red[tid] + red[128 + tid];
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// Launches the form the arguments ask for: pooled (colsum: one column sum per 128-row block of every image of HW rows; a.bpi comes
// back), top-down (td), residual (rd), implicit im2col (conv: the caller has set the conv fields) or plain.  `a` carries the base
// fields (srf_gemm_set_base) and zeros.
template <class F>
static inline int srf_tile128_launch(typename F::Args &a, const void *W_packed, hipStream_t stream, float *colsum = nullptr, long long HW = 0,
                                     const SrfGemmTop *td = nullptr, const SrfGemmRes *rd = nullptr, bool conv = false)
{
    a.nct = srf_ceil_div(a.Cout, 128);
    a.colsum = colsum;
    a.HW = HW;
    srf_gemm_set_top(a, td);
    if constexpr (F::resid != nullptr) srf_gemm_set_res(a, rd);   // a family without the form has no such fields
    if (colsum) {
        a.bpi = (int)srf_ceil_div(HW, 128);
        a.mblocks = (a.M / HW) * a.bpi;
    } else {
        a.mblocks = srf_ceil_div(a.M, 128);
    }
    const int rc = F::set_weights(a, W_packed);
    if (rc != SRF_OK) return rc;
    const long long blocks = ((a.mblocks + 7) / 8) * 8 * a.nct;   // whole groups of 8 row blocks: one per XCD
    if (blocks >= (1ll << 31)) return SRF_EUNSUPPORTED;
    void (*const kernel)(typename F::Args) = colsum ? F::pool : td ? F::topdown : rd ? F::resid : conv ? F::conv : F::plain;
    if (!kernel) return SRF_EUNSUPPORTED;   // a form this family does not build
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

template <class F>
static inline int srf_tile128_plain(const float *x, long long M, int K, long long x_ld, const void *W_packed, int Cout, const float *scale,
                                    const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream)
{
    const int rc = srf_gemm_check_1x1(F::limits, M, K, x_ld, x, W_packed, Cout, y, y_ld);
    if (rc != SRF_OK || M == 0) return rc;
    typename F::Args a = {};
    srf_gemm_set_base(a, x, M, K, x_ld, Cout, scale, shift, relu, y, y_ld);
    return srf_tile128_launch<F>(a, W_packed, (hipStream_t)stream);
}

template <class F>
static inline int srf_tile128_residual(const float *x, long long M, int K, long long x_ld, const void *W_packed, int Cout, const float *scale,
                                       const float *shift, int relu, float *y, long long y_ld, const float *res, long long res_ld,
                                       srf_stream_t stream)
{
    const SrfGemmRes rd = {res, res_ld};
    const int rc = srf_gemm_check_1x1(F::limits, M, K, x_ld, x, W_packed, Cout, y, y_ld, nullptr, nullptr, &rd);
    if (rc != SRF_OK || M == 0) return rc;
    typename F::Args a = {};
    srf_gemm_set_base(a, x, M, K, x_ld, Cout, scale, shift, relu, y, y_ld);
    return srf_tile128_launch<F>(a, W_packed, (hipStream_t)stream, nullptr, 0, nullptr, &rd);
}

template <class F>
static inline int srf_tile128_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const void *W_packed, int Cout,
                                      const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt, long long top_ld,
                                      float *y, long long y_ld, srf_stream_t stream)
{
    const SrfGemmTop td = {top, top_ld, H, W, Ht, Wt};
    const int rc = srf_gemm_check_1x1(F::limits, N, K, x_ld, x, W_packed, Cout, y, y_ld, &td);
    if (rc != SRF_OK || N == 0) return rc;
    typename F::Args a = {};
    srf_gemm_set_base(a, x, (long long)N * H * W, K, x_ld, Cout, scale, shift, relu, y, y_ld);
    return srf_tile128_launch<F>(a, W_packed, (hipStream_t)stream, nullptr, 0, &td);
}

// workspace = srf_conv1x1_nhwc_pooled_workspace_bytes(N, HW, Cout)
template <class F>
static inline int srf_tile128_pooled(const float *x, int N, long long HW, int K, long long x_ld, const void *W_packed, int Cout,
                                     const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean, void *workspace,
                                     size_t workspace_bytes, srf_stream_t stream)
{
    const SrfGemmPool pool = {HW, mean, workspace, workspace_bytes};
    int rc = srf_gemm_check_1x1(F::limits, N, K, x_ld, x, W_packed, Cout, y, y_ld, nullptr, &pool);
    if (rc != SRF_OK || N == 0) return rc;
    typename F::Args a = {};
    srf_gemm_set_base(a, x, (long long)N * HW, K, x_ld, Cout, scale, shift, relu, y, y_ld);
    rc = srf_tile128_launch<F>(a, W_packed, (hipStream_t)stream, (float *)workspace, HW);
    if (rc != SRF_OK) return rc;
    return srf_gemm_pool_finish((const float *)workspace, a.bpi, N, Cout, HW, mean, (hipStream_t)stream);
}

// Conv2d(Cin, Cout, (kh, kw), stride, pad) with an implicit im2col; W_packed = the family's pack_weights of the weight reordered to
// (Cout, kh * kw * Cin), tap index slowest
template <class F>
static inline int srf_tile128_conv(const float *x, int N, int H, int W, int Cin, long long x_ld, const void *W_packed, int Cout, int kh, int kw,
                                   int stride, int pad, const float *scale, const float *shift, int relu, float *y, long long y_ld,
                                   srf_stream_t stream)
{
    int Ho = 0, Wo = 0;
    long long x_bytes = 0;
    const int rc = srf_gemm_check_conv(F::limits, N, H, W, Cin, x_ld, x, W_packed, Cout, kh, kw, stride, pad, y, y_ld, &Ho, &Wo, &x_bytes);
    if (rc != SRF_OK || N == 0) return rc;
    if ((long long)kh * kw * Cin >= (1ll << 31)) return SRF_EUNSUPPORTED;   // K is an int
    typename F::Args a = {};
    srf_gemm_set_base(a, x, (long long)N * Ho * Wo, kh * kw * Cin, x_ld, Cout, scale, shift, relu, y, y_ld);
    srf_gemm_set_conv(a, H, W, Ho, Wo, kw, stride, pad, Cin, x_bytes);
    return srf_tile128_launch<F>(a, W_packed, (hipStream_t)stream, nullptr, 0, nullptr, nullptr, true);
}
