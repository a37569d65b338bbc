// dcn.hip -- modulated deformable convolution (DCNv2) forward on the f32 MFMA, channels-last (NHWC).
//
// Reference call site: the 3x3 convolution of the 26 bottlenecks of stages 3 and 4 of the ResNet-101 image backbone of
// configs/others/srfdet_dvoxel_waymo_LC.py:68-69 (`dcn=dict(type='DCNv2', deform_groups=1)`), in the reference mmcv's
// `ModulatedDeformConv2dPack` (a CUDA operator outside the reference tree).  The definition this kernel follows is the
// repository's own, compat/dcn.py::modulated_deform_conv2d (Zhu et al., "Deformable ConvNets v2", eq. 1, with mmcv's tensor
// conventions): bilinear sampling at p = base + tap + offset, zero padding (a corner outside the map contributes 0),
// times a per-(pixel, tap, deformable group) mask.
//
// srf_dcnv2_nhwc is the implicit-im2col GEMM of srf_conv_gemm_nhwc (conv.hip, srf_gemm_body<RM, RN, CONV = true>): rows =
// output pixels, k = (tap, input channel) with the tap slowest, the same packed weights (srf_conv1x1_nhwc_pack_weights), the
// same LDS images, the same MFMA loop (v_mfma_f32_32x32x2_f32, one k-ordered fma chain per output) and the same affine +
// ReLU epilogue.  What changes is the A operand: where the plain convolution stages ONE 16-byte buffer load per (pixel, tap,
// 32-channel chunk), this kernel stages the blend of FOUR such loads,
//     a = w00 x[y0][x0] + w01 x[y0][x1] + w10 x[y1][x0] + w11 x[y1][x1],   w.. = bilinear weight * mask,
// four float4 loads and sixteen fmas per staged float4.
//   * per (pixel row of the thread, tap, deformable group) the four corner byte offsets (0x80000000 = out of the buffer
//     descriptor's range for a corner outside the map: the hardware returns zeros, the convolution's zero padding) and the
//     four mask-scaled weights are computed ONCE, into registers, and reused over the Cin / G / 32 channel chunks of that tap
//     (8 at 256 channels, 16 at 512): the chunk only moves the scalar offset of the loads;
//   * the raw (dy, dx, mask) of the NEXT (tap, group) are requested when the current one is set up, a whole tap ahead of
//     their use;
//   * the global loads of chunk c + 2 are in flight while chunk c multiplies; the blend runs when they are written to LDS.
// With zero offsets and a unit mask the weights are exactly (1, 0, 0, 0): the kernel then returns the bits of
// srf_conv_gemm_nhwc.  Fixed summation order, no atomics: two calls give the same bits.
#include "common.hpp"

typedef float dc_f32x16 __attribute__((ext_vector_type(16)));
typedef float dc_f32x4 __attribute__((ext_vector_type(4)));

struct DcnArgs {
    const float *x;
    float *y;
    const dc_f32x4 *Wp;
    const float *scale, *shift;
    const float *off, *mask;          // (N, Ho, Wo, off_ld) / (N, Ho, Wo, mask_ld)
    long long x_ld, y_ld, off_ld, mask_ld, M, mblocks;
    long long x_bytes;
    int Cout, coutBlocks, nchunk, relu;
    int H, W, Ho, Wo, kw, K, stride, pad, dil;
    int cin_chunks, cpg, G;           // Cin / 32, chunks per deformable group, deformable groups
    int mask_is_logit;
};

#define DC_FENCE() __builtin_amdgcn_sched_barrier(0)
#define DC_OOB 0x80000000u

// Workgroup tile: (64 RM) pixels x (64 RN) channels, 4 waves = 2 x 2 wave tiles of (32 RM) x (32 RN), as srf_gemm_body.
template <int RM, int RN>
__device__ __forceinline__ void srf_dcn_body(const DcnArgs &a, const unsigned bid)
{
    constexpr int TM = 64 * RM, TN = 64 * RN;
    constexpr int ASZ = 8 * TM;          // float4 per A stage
    constexpr int BSZ = 8 * TN;          // float4 per B stage
    constexpr int NA = ASZ / 256;        // pixel rows per thread (= 2 RM); one float4 (4 channels) of each per chunk
    constexpr int NB = BSZ / 256;
    constexpr int NCS = 256 / TN;        // channel sub-blocks per packed block
    extern __shared__ __attribute__((aligned(16))) dc_f32x4 s_d[];  // A[ASZ] | B[BSZ]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xcd = bid & 7, jq = bid >> 3;
    const int nct = (a.Cout + TN - 1) / TN;
    const int ct = jq % nct;
    const int cb = ct / NCS, cs = ct - cb * NCS;
    const long long mb = (long long)(jq / nct) * 8 + xcd;
    if (mb >= a.mblocks) return;
    const long long p0 = mb * TM, rows_blk = a.M - p0;

    __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, (int)a.x_bytes, 0x00020000);
    // the output pixel of each of this thread's rows: image, input coordinates of tap (0, 0), offset / mask rows
    int cn[NA];
    int cy[NA], cx[NA];
    const float *orow[NA], *mrow[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const long long pr = p0 + (tid >> 3) + 32 * j;
        const long long p = pr < a.M ? pr : a.M - 1;   // rows past the end read the last pixel's offsets and load nothing
        const long long hw = (long long)a.Ho * a.Wo;
        const int n = (int)(p / hw);
        const int rem = (int)(p - n * hw);
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        cn[j] = pr < a.M ? n : -1;
        cy[j] = oy * a.stride - a.pad;
        cx[j] = ox * a.stride - a.pad;
        orow[j] = a.off + p * a.off_ld;
        mrow[j] = a.mask + p * a.mask_ld;
    }
    const unsigned quad_b = (unsigned)((tid & 7) * 16);
    const unsigned px_b = (unsigned)(a.x_ld * 4), row_b = (unsigned)(a.W * a.x_ld * 4);

    // ---- the gather table of the current (tap, group) key = tap * G + g: 4 byte offsets + 4 weights per row ----
    unsigned go[NA][4];
    float gw[NA][4];
    float rdy[NA], rdx[NA], rm[NA];   // raw values of the key requested last
    const int nkeys = a.K * a.G;
#define DC_REQUEST(KEY)                                                                                               \
    do {                                                                                                              \
        const int rk_ = (KEY) < nkeys ? (KEY) : nkeys - 1;                                                            \
        const int rt_ = rk_ / a.G, rg_ = rk_ - rt_ * a.G;                                                             \
        const int roc_ = (rg_ * a.K + rt_) * 2, rmc_ = rg_ * a.K + rt_;                                               \
        _Pragma("unroll") for (int rj_ = 0; rj_ < NA; ++rj_) {                                                        \
            rdy[rj_] = orow[rj_][roc_];                                                                               \
            rdx[rj_] = orow[rj_][roc_ + 1];                                                                           \
            rm[rj_] = mrow[rj_][rmc_];                                                                                \
        }                                                                                                             \
    } while (0)
    // position = integer base (pixel, tap) + offset: floor and fraction are taken of the OFFSET, so the bilinear weights carry no
    // rounding of the sum (base + offset in f32 loses up to H 2^-24 of a pixel); the offset is clamped to +-2^30 (far outside any
    // map of a tensor below 2 GiB, NaN included) so that the integer conversion stays in range, the corner to [-2, H] (both ends: no
    // corner inside) so that the address arithmetic does
#define DC_SETUP(KEY)                                                                                                 \
    do {                                                                                                              \
        const int st_ = (KEY) / a.G;                                                                                  \
        const int ky_ = st_ / a.kw, kx_ = st_ - ky_ * a.kw;                                                           \
        const int by_ = ky_ * a.dil, bx_ = kx_ * a.dil;                                                               \
        _Pragma("unroll") for (int sj_ = 0; sj_ < NA; ++sj_) {                                                        \
            float m_ = rm[sj_];                                                                                       \
            if (a.mask_is_logit) m_ = 1.f / (1.f + expf(-m_));                                                        \
            const float dy_ = fminf(fmaxf(rdy[sj_], -1073741824.f), 1073741824.f);                                    \
            const float dx_ = fminf(fmaxf(rdx[sj_], -1073741824.f), 1073741824.f);                                    \
            const float fy_ = floorf(dy_), fx_ = floorf(dx_);                                                         \
            const float ly_ = dy_ - fy_, lx_ = dx_ - fx_, hy_ = 1.f - ly_, hx_ = 1.f - lx_;                           \
            const int y0_ = max(-2, min(a.H, cy[sj_] + by_ + (int)fy_)), x0_ = max(-2, min(a.W, cx[sj_] + bx_ + (int)fx_)); \
            const bool live_ = cn[sj_] >= 0;                                                                          \
            const bool y0ok_ = live_ && y0_ >= 0 && y0_ < a.H, y1ok_ = live_ && y0_ >= -1 && y0_ + 1 < a.H;           \
            const bool x0ok_ = x0_ >= 0 && x0_ < a.W, x1ok_ = x0_ >= -1 && x0_ + 1 < a.W;                             \
            const unsigned b_ = (unsigned)((((long long)cn[sj_] * a.H + y0_) * a.W + x0_) * a.x_ld * 4) + quad_b;     \
            go[sj_][0] = y0ok_ && x0ok_ ? b_ : DC_OOB;                                                                \
            go[sj_][1] = y0ok_ && x1ok_ ? b_ + px_b : DC_OOB;                                                         \
            go[sj_][2] = y1ok_ && x0ok_ ? b_ + row_b : DC_OOB;                                                        \
            go[sj_][3] = y1ok_ && x1ok_ ? b_ + row_b + px_b : DC_OOB;                                                 \
            gw[sj_][0] = (hy_ * hx_) * m_;                                                                            \
            gw[sj_][1] = (hy_ * lx_) * m_;                                                                            \
            gw[sj_][2] = (ly_ * hx_) * m_;                                                                            \
            gw[sj_][3] = (ly_ * lx_) * m_;                                                                            \
        }                                                                                                             \
    } while (0)

    const int a_dst = (tid >> 3) * 8 + ((tid & 7) ^ ((tid >> 4) & 7));  // + 256 j: rows advance by 32, the swizzle repeats
    const dc_f32x4 *Bg = a.Wp + (size_t)cb * 2048 + cs * BSZ + tid;
    const size_t b_chunk_stride = (size_t)a.coutBlocks * 2048;
    dc_f32x4 ar[NA][4], br[NB];
    // chunk = (tap, 32-channel chunk cc of the Cin channels), tap slowest; its deformable group is cc / cpg, its key tap * G + g.
    // The loader walks the chunks 0, 1, .., last, last, .. with counters (no division per chunk).  A chunk of another key than
    // the table's: set the table up from the raw values requested a tap ago, request the next key's.
    const int last = a.nchunk - 1;
    int cur_key = 0, ld_ch = 0, ld_cc = 0, ld_key = 0, ld_left = a.cpg;
#define DC_LOAD()                                                                                                     \
    do {                                                                                                              \
        if (ld_key != cur_key) {                                                                                      \
            DC_SETUP(ld_key);                                                                                         \
            DC_REQUEST(ld_key + 1);                                                                                   \
            cur_key = ld_key;                                                                                         \
        }                                                                                                             \
        const int soff_ = ld_cc * 128;                                                                                \
        _Pragma("unroll") for (int j_ = 0; j_ < NA; ++j_)                                                             \
            _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                                        \
                auto v_ = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (int)go[j_][q_], soff_, 0);                    \
                ar[j_][q_] = *reinterpret_cast<dc_f32x4 *>(&v_);                                                      \
            }                                                                                                         \
        const dc_f32x4 *bb_ = Bg + (size_t)ld_ch * b_chunk_stride;                                                    \
        _Pragma("unroll") for (int j_ = 0; j_ < NB; ++j_) br[j_] = bb_[j_ * 256];                                     \
        if (ld_ch < last) {                                                                                           \
            ++ld_ch;                                                                                                  \
            ld_cc = ld_cc + 1 == a.cin_chunks ? 0 : ld_cc + 1;                                                        \
            if (--ld_left == 0) {                                                                                     \
                ld_left = a.cpg;                                                                                      \
                ++ld_key;                                                                                             \
            }                                                                                                         \
        }                                                                                                             \
    } while (0)
    // the blend of the chunk in the staging registers (with the weights it was loaded under: DC_LOAD changes the table only
    // behind the DC_STORE of the chunk before it) -> LDS
#define DC_STORE()                                                                                                    \
    do {                                                                                                              \
        _Pragma("unroll") for (int j_ = 0; j_ < NA; ++j_) {                                                           \
            dc_f32x4 v_ = ar[j_][0] * gw[j_][0];                                                                      \
            _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                                        \
                v_[e_] = __fmaf_rn(ar[j_][1][e_], gw[j_][1], v_[e_]);                                                 \
                v_[e_] = __fmaf_rn(ar[j_][2][e_], gw[j_][2], v_[e_]);                                                 \
                v_[e_] = __fmaf_rn(ar[j_][3][e_], gw[j_][3], v_[e_]);                                                 \
            }                                                                                                         \
            s_d[a_dst + 256 * j_] = v_;                                                                               \
        }                                                                                                             \
        _Pragma("unroll") for (int j_ = 0; j_ < NB; ++j_) s_d[ASZ + tid + 256 * j_] = br[j_];                         \
    } while (0)

    const int wm = wave & 1, wn = wave >> 1;
    const int li = lane & 31, lh = lane >> 5;
    const int swz = (li >> 1) & 7;
    const int a_row = (wm * 32 * RM + li) * 8;        // + im * 256
    const int b_row = ASZ + (wn * 32 * RN + li) * 8;  // + jn * 256
    int qs[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) qs[s2] = (2 * s2 + lh) ^ swz;
    dc_f32x16 acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    dc_f32x4 fa[2][RM], fb[2][RN];
#define DC_READ(SET, S2)                                                                                              \
    do {                                                                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < RM; ++i_) fa[SET][i_] = s_d[a_row + i_ * 256 + qs[S2]];               \
        _Pragma("unroll") for (int j_ = 0; j_ < RN; ++j_) fb[SET][j_] = s_d[b_row + j_ * 256 + qs[S2]];               \
    } while (0)
#define DC_MFMA(SET)                                                                                                  \
    do {                                                                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < RM; ++i_) asm volatile("" : "+v"(fa[SET][i_]));                       \
        _Pragma("unroll") for (int j_ = 0; j_ < RN; ++j_) asm volatile("" : "+v"(fb[SET][j_]));                       \
        _Pragma("unroll") for (int ks_ = 0; ks_ < 4; ++ks_)                                                           \
            _Pragma("unroll") for (int i_ = 0; i_ < RM; ++i_)                                                         \
                _Pragma("unroll") for (int j_ = 0; j_ < RN; ++j_)                                                     \
                    acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET][i_][ks_], fb[SET][j_][ks_], acc[i_][j_], 0, 0, 0); \
    } while (0)

    // One LDS stage, as srf_gemm_body: chunk c is multiplied out of LDS while chunk c + 1 waits in registers (unblended);
    // at the end of the chunk a barrier retires the readers, the registers are blended into LDS, chunk c + 2 is requested,
    // a second barrier publishes.
    const int nchunk = a.nchunk;
    DC_REQUEST(0);
    DC_SETUP(0);
    DC_REQUEST(1);
    DC_LOAD();
    DC_STORE();
    DC_LOAD();
    __syncthreads();
    DC_READ(0, 0);
    for (int c = 0; c < nchunk; ++c) {
        DC_READ(1, 1);
        DC_FENCE();
        DC_MFMA(0);
        DC_FENCE();
        DC_READ(0, 2);
        DC_FENCE();
        DC_MFMA(1);
        DC_FENCE();
        DC_READ(1, 3);
        DC_FENCE();
        DC_MFMA(0);
        DC_FENCE();
        DC_MFMA(1);
        DC_FENCE();
        __syncthreads();
        DC_STORE();
        DC_LOAD();
        __syncthreads();
        DC_READ(0, 0);
        DC_FENCE();
    }

    // epilogue: lane = channel (li) within RN blocks of 32, accumulator register = pixel row
    float sc[RN], sh[RN];
    bool co_ok[RN];
    const int co0 = cb * 256 + cs * TN + wn * 32 * RN + li;
#pragma unroll
    for (int j = 0; j < RN; ++j) {
        const int co = co0 + j * 32;
        co_ok[j] = co < a.Cout;
        sc[j] = (co_ok[j] && a.scale) ? a.scale[co] : 1.f;
        sh[j] = (co_ok[j] && a.shift) ? a.shift[co] : 0.f;
    }
    // stores through a buffer descriptor over this block's rows: a row past the end and a channel past Cout are offsets
    // beyond the range, which the hardware drops
    const long long rows_here = rows_blk < TM ? rows_blk : TM;
    __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(a.y + p0 * a.y_ld, 0, (int)(rows_here * a.y_ld * 4), 0x00020000);
    const int row_base = wm * 32 * RM + 4 * lh;     // + i * 32 + (r & 3) + 8 * (r >> 2)
    unsigned ybase[RN];
#pragma unroll
    for (int j = 0; j < RN; ++j) ybase[j] = co_ok[j] ? (unsigned)((row_base * a.y_ld + co0 + j * 32) * 4) : DC_OOB;
    const unsigned yrow_b = (unsigned)(a.y_ld * 4);
#pragma unroll
    for (int i = 0; i < RM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dr = i * 32 + (r & 3) + 8 * (r >> 2);
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                float v = __fmaf_rn(acc[i][j][r], sc[j], sh[j]);
                if (a.relu) v = fmaxf(v, 0.f);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yrsrc, (int)(ybase[j] + (unsigned)dr * yrow_b), 0, 0);
            }
        }
        DC_FENCE();
    }
}

// 128 VGPRs, no scratch, 16 KB of LDS: four workgroups (16 waves) per CU
__global__ __launch_bounds__(256, 4) void srf_dcnv2_nhwc_k(DcnArgs a)
{
    srf_dcn_body<1, 1>(a, blockIdx.x);
}

extern "C" int srf_dcnv2_nhwc(const float *x, int N, int H, int W, int Cin, long long x_ld, const float *offset, long long offset_ld,
                              const float *mask, long long mask_ld, int mask_is_logit, const float *W_packed, int Cout, int kh, int kw,
                              int stride, int pad, int dilation, int groups, int deform_groups, const float *scale, const float *shift,
                              int relu, float *y, long long y_ld, srf_stream_t stream)
{
    if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dilation <= 0 || groups <= 0 ||
        deform_groups <= 0 || x_ld < Cin || y_ld < Cout)
        return SRF_EINVAL;
    const long long K = (long long)kh * kw;
    if (offset_ld < 2 * K * deform_groups || mask_ld < K * deform_groups) return SRF_EINVAL;
    if (groups != 1 || Cin % deform_groups != 0 || ((Cin / deform_groups) & 31)) return SRF_EUNSUPPORTED;
    // a map of one row or one column: compat/dcn.py's normalised grid (2 / max(H - 1, 1)) collapses every position onto it
    if (H < 2 || W < 2 || K > 1024) return SRF_EUNSUPPORTED;
    const long long x_bytes = (long long)N * H * W * x_ld * 4;
    if (x_bytes >= (1ll << 31)) return SRF_EUNSUPPORTED;
    if (N == 0) return SRF_OK;
    if (!x || !offset || !mask || !W_packed || !y) return SRF_EINVAL;
    if ((x_ld & 3) || ((uintptr_t)x & 15) || ((uintptr_t)W_packed & 15)) return SRF_EUNSUPPORTED;
    const int Ho = (H + 2 * pad - dilation * (kh - 1) - 1) / stride + 1, Wo = (W + 2 * pad - dilation * (kw - 1) - 1) / stride + 1;
    if (H + 2 * pad < dilation * (kh - 1) + 1 || W + 2 * pad < dilation * (kw - 1) + 1 || Ho <= 0 || Wo <= 0) return SRF_EINVAL;
    DcnArgs a;
    a.x = x;
    a.y = y;
    a.Wp = reinterpret_cast<const dc_f32x4 *>(W_packed);
    a.scale = scale;
    a.shift = shift;
    a.off = offset;
    a.mask = mask;
    a.x_ld = x_ld;
    a.y_ld = y_ld;
    a.off_ld = offset_ld;
    a.mask_ld = mask_ld;
    a.M = (long long)N * Ho * Wo;
    a.x_bytes = x_bytes;
    a.Cout = Cout;
    a.coutBlocks = srf_ceil_div(Cout, 256);
    a.nchunk = (int)(K * (Cin / 32));
    a.relu = relu;
    a.H = H;
    a.W = W;
    a.Ho = Ho;
    a.Wo = Wo;
    a.kw = kw;
    a.K = (int)K;
    a.stride = stride;
    a.pad = pad;
    a.dil = dilation;
    a.cin_chunks = Cin / 32;
    a.G = deform_groups;
    a.cpg = a.cin_chunks / deform_groups;
    a.mask_is_logit = mask_is_logit;
    if (64 * y_ld * 4 >= (1ll << 31)) return SRF_EUNSUPPORTED;   // buffer-descriptor range of one block of output rows
    // 64 x 64 tiles for every shape.  On the two production maps (188 / 47 row blocks) they beat 64 pixels x 128 channels, which shares
    // a pixel row's gather among twice the channels but leaves 376 / 188 workgroups for 256 CUs (layer 226 against 262 us, 324 against
    // 342 us: DESIGN.md section 4); a 128-pixel tile needs 32 more address / weight registers per thread and spills.
    a.mblocks = srf_ceil_div(a.M, 64);
    const long long blocks = ((a.mblocks + 7) / 8) * 8 * srf_ceil_div(Cout, 64);
    if (blocks >= (1ll << 31)) return SRF_EUNSUPPORTED;
    hipLaunchKernelGGL(srf_dcnv2_nhwc_k, dim3((unsigned)blocks), dim3(256), (8 * 64 + 8 * 64) * 16, (hipStream_t)stream, a);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
