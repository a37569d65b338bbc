// gemm_direct.hip -- srf_conv1x1_nhwc_direct: the 1x1 convolutions of the camera branch (VoVNet's OSA `concat` layers,
// mmdet3d_plugin/models/backbones/vovnet.py:222-223, with the eSE average pool of :165-177 from the same pass) as a GEMM on the
// f32 MFMA whose operands never touch LDS.
//
// srf_conv1x1_nhwc_k (conv.hip) stages both operands through LDS with two barriers per 32-channel chunk and reaches 79 % of the
// MFMA peak (122-128 TFLOP/s; rocBLAS 132-140).  srf_wino43_mm_k showed what the same MFMA does when a wave's operands come
// straight from L2 into its registers and nothing synchronises the waves: 98 % MFMA-busy in the reduction loop.  The same
// structure here:
//   * workgroup tile 128 pixels x 128 channels, 4 waves = 2 x 2 wave tiles of 64 x 64 (4 accumulator tiles = 64 registers),
//     three workgroups per CU (12 independent waves);
//   * A: lane (row, half) of a 32-row block loads the four channels 8 s + 4 half .. + 3 of its row for sub-step s of a chunk
//     (buffer_load_dwordx4 with a scalar chunk offset; rows past the block are out of range and read as zero).  The 32 lanes
//     touch 32 lines, the four sub-steps of a chunk the same lines again (L1 hits);
//   * B: packed once per layer as [chunk][128-column tile][wave column half][block][sub-step][half][column 32][4] -- the piece
//     a wave needs for one sub-step of one block is 1 KB contiguous, one buffer_load_dwordx4 per lane;
//   * one chunk of lookahead, in place: the registers of sub-step s are reloaded right behind its 16 MFMAs.
// The order of the fma chain of every output is the one of srf_conv1x1_nhwc_k (sub-step s of a chunk multiplies the channels
// 8 s + i (lanes 0-31) and 8 s + 4 + i (lanes 32-63), i = 0..3): identical bits.
#include "common.hpp"
#include "gemm_tile128.hpp"

typedef float gd_f32x16 __attribute__((ext_vector_type(16)));
typedef float gd_f32x4 __attribute__((ext_vector_type(4)));

struct GdArgs : SrfTile128Args<const float *> {};   // Wp: the packed image of srf_gemm_direct_pack_k; no fields of its own
#define GD_PLAIN 0
#define GD_POOL 1
#define GD_TOPDOWN 2
#define GD_RESID 3

// W (Cout, K) row-major -> the packed image (GdArgs::Wp); channels >= Cout are zero
__global__ __launch_bounds__(256) void srf_gemm_direct_pack_k(const float *__restrict__ Wt, int Cout, int K, int nct, float *__restrict__ P,
                                                             long long total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int kk = (int)(t & 3), co = (int)((t >> 2) & 31), lh = (int)((t >> 7) & 1), s2 = (int)((t >> 8) & 3), j = (int)((t >> 10) & 1),
              wn = (int)((t >> 11) & 1);
    const long long rest = t >> 12;
    const int ct = (int)(rest % nct), chunk = (int)(rest / nct);
    const int cog = ct * 128 + wn * 64 + j * 32 + co, k = chunk * 32 + s2 * 8 + lh * 4 + kk;
    P[t] = cog < Cout ? Wt[(size_t)cog * K + k] : 0.f;
}

template <int MODE>
__global__ __launch_bounds__(256, 3) void srf_gemm_direct_k(GdArgs a)
{
    constexpr bool POOL = MODE == GD_POOL, TOPDOWN = MODE == GD_TOPDOWN, RESID = MODE == GD_RESID;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    int ct;
    const long long mb = srf_tile128_row_block(a.nct, ct);
    if (mb >= a.mblocks) return;
    const SrfTile128Item it = srf_tile128_item<POOL>(ct, mb, a.M, a.HW, a.bpi);
    const long long p0 = it.p0, rows_here = it.rows_here;
    __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x) + p0 * a.x_ld, 0, (int)(rows_here * a.x_ld * 4), 0x00020000);
    const size_t chunk_bytes = (size_t)a.nct * 16384;
    __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.Wp) + ((size_t)ct * 16 + wn * 8) * 256, 0,
                                                                 (int)((size_t)a.nchunk * chunk_bytes - ((size_t)ct * 16 + wn * 8) * 1024), 0x00020000);
    unsigned aoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) aoff[i] = (unsigned)(((wm * 64 + i * 32 + li) * a.x_ld + lh * 4) * 4);
    const int boff = lane * 16;

    gd_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    gd_f32x4 fa[2][4], fb[2][4];
#define GD_LOAD(S2, C)                                                                                              \
    do {                                                                                                            \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                          \
            auto v_ = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)aoff[i_], (C) * 128 + (S2) * 32, 0);           \
            fa[i_][S2] = *reinterpret_cast<gd_f32x4 *>(&v_);                                                        \
        }                                                                                                           \
        _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                                          \
            auto v_ = __builtin_amdgcn_raw_buffer_load_b128(wr, boff, (int)((C) * chunk_bytes) + (j_ * 4 + (S2)) * 1024, 0); \
            fb[j_][S2] = *reinterpret_cast<gd_f32x4 *>(&v_);                                                        \
        }                                                                                                           \
    } while (0)
#define GD_MFMA(S2)                                                                                                 \
    do {                                                                                                            \
        _Pragma("unroll") for (int ks_ = 0; ks_ < 4; ++ks_)                                                         \
            _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_)                                                        \
                _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                                    \
                    acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i_][S2][ks_], fb[j_][S2][ks_], acc[i_][j_], 0, 0, 0); \
    } while (0)

    const int nchunk = a.nchunk;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) GD_LOAD(s2, 0);
    for (int c = 0; c < nchunk - 1; ++c) {
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            GD_MFMA(s2);
            GD_LOAD(s2, c + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) GD_MFMA(s2);
#undef GD_LOAD
#undef GD_MFMA

    // the frame's scratch LDS, sized by form: the top-down offsets [128] or the column-sum partials [2][128]
    __shared__ int scratch[POOL ? 256 : TOPDOWN ? 128 : 1];
    srf_tile128_epilogue<POOL, TOPDOWN, RESID>(SRF_TILE128_EPI(a), acc, it, scratch, tid, li, lh, wm, wn);
}

extern "C" size_t srf_conv1x1_nhwc_direct_packed_weight_bytes(int Cout, int K)
{
    if (Cout <= 0 || K <= 0 || (K & 31)) return 0;
    return (size_t)(K / 32) * srf_ceil_div(Cout, 128) * 16384;
}

extern "C" int srf_conv1x1_nhwc_direct_pack_weights(const float *W, int Cout, int K, float *packed, srf_stream_t stream)
{
    if (Cout <= 0 || K <= 0 || !W || !packed) return SRF_EINVAL;
    if (K & 31) return SRF_EUNSUPPORTED;
    const int nct = srf_ceil_div(Cout, 128);
    const long long total = (long long)(K / 32) * nct * 4096;
    hipLaunchKernelGGL(srf_gemm_direct_pack_k, dim3((unsigned)srf_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, W, Cout, K, nct, packed,
                       total);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

struct GdFamily {
    typedef GdArgs Args;
    static constexpr SrfGemmFamily limits = {128, true, 128};   // x and y through descriptors of one 128-row tile
    static constexpr void (*plain)(GdArgs) = srf_gemm_direct_k<GD_PLAIN>, (*pool)(GdArgs) = srf_gemm_direct_k<GD_POOL>,
                          (*topdown)(GdArgs) = srf_gemm_direct_k<GD_TOPDOWN>, (*resid)(GdArgs) = srf_gemm_direct_k<GD_RESID>,
                          (*conv)(GdArgs) = nullptr;
    static int set_weights(GdArgs &a, const void *W_packed)
    {
        a.Wp = (const float *)W_packed;
        return srf_conv1x1_nhwc_direct_packed_weight_bytes(a.Cout, a.K) >= ((size_t)1 << 31) ? SRF_EUNSUPPORTED : SRF_OK;   // descriptor range of Wp
    }
};

extern "C" int srf_conv1x1_nhwc_direct(const float *x, long long M, int K, long long x_ld, const float *W_packed, int Cout, const float *scale,
                                       const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream)
{
    return srf_tile128_plain<GdFamily>(x, M, K, x_ld, W_packed, Cout, scale, shift, relu, y, y_ld, stream);
}

// the residual form: as srf_conv1x1_nhwc_residual (conv.hip)
extern "C" int srf_conv1x1_nhwc_direct_residual(const float *x, long long M, int K, long long x_ld, const float *W_packed, int Cout, const float *scale,
                                               const float *shift, int relu, float *y, long long y_ld, const float *res, long long res_ld,
                                               srf_stream_t stream)
{
    return srf_tile128_residual<GdFamily>(x, M, K, x_ld, W_packed, Cout, scale, shift, relu, y, y_ld, res, res_ld, stream);
}

extern "C" int srf_conv1x1_nhwc_direct_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const float *W_packed, int Cout,
                                               const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt,
                                               long long top_ld, float *y, long long y_ld, srf_stream_t stream)
{
    return srf_tile128_topdown<GdFamily>(x, N, H, W, K, x_ld, W_packed, Cout, scale, shift, relu, top, Ht, Wt, top_ld, y, y_ld, stream);
}

// the pooled form: as srf_conv1x1_nhwc_pooled (conv.hip); workspace = srf_conv1x1_nhwc_pooled_workspace_bytes(N, HW, Cout)
extern "C" int srf_conv1x1_nhwc_direct_pooled(const float *x, int N, long long HW, int K, long long x_ld, const float *W_packed, int Cout,
                                              const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean,
                                              void *workspace, size_t workspace_bytes, srf_stream_t stream)
{
    return srf_tile128_pooled<GdFamily>(x, N, HW, K, x_ld, W_packed, Cout, scale, shift, relu, y, y_ld, mean, workspace, workspace_bytes, stream);
}
