// spconv_bf16.hip -- srf_spconv_fwd_bf16: the 64- and 128-output-channel layers of the sparse encoder with f32 tensors and ONE bf16
// product per f32 product -- the opt-in reduced-precision mode of the LiDAR half (`SRFDet.sparse_mfma_dtype`, sparse.mfma_dtype), the
// counterpart of gemm_bf16.hip on the camera half.  The f32 route of these layers (srf_spconv_gsp_k, spconv.hip) is bound by
// v_mfma_f32_16x16x4_f32; this file is what they cost once that time is almost gone.
//
// Definition (tests/spconv_bf16_ref.py is this paragraph in numpy; tests/test_gpu_spconv_bf16.py holds the kernel to it):
//     out[o, :] = epilogue( sum over offsets k with nbr[k][o] >= 0, over channels c of  bf16(x[nbr[k][o], c]) * bf16(W[k, c, :]) )
// bf16() = round to nearest even (v_cvt_pk_bf16_f32 = torch.Tensor.bfloat16()); the weights are rounded once, when they are packed, a
// gathered row in registers right behind its load.  Every product is exact in f32; the sum is an f32 accumulation in a fixed order
// (offsets ascending; inside an offset 16 channels per v_mfma_f32_32x32x16_bf16, ascending).  The epilogue is the f32 route's
// (srf_spconv_epilogue, spconv_frame.hpp), in f32 on the f32 accumulator.  alpha, beta and the residual are not rounded; f32 is stored.
// No float atomics: two launches give the same bits.
//
// The bits of an output row depend on that row's own pairs, the operands and the epilogue alone -- not on the capacity, the live row
// count, the row plan (the kernel takes none: `tiles` is accepted and ignored) or the rows it shares a tile with.  A row is one row of
// an MFMA's A operand, and an MFMA's rows do not interact.  What the neighbours decide is only WHICH offsets a wave multiplies: one
// that none of its 32 rows has is skipped, one that another row has is multiplied with this row's operand all zero (a rulebook entry
// of -1 is gathered as an out-of-range buffer offset, which reads zeros without a branch around the load).  Such an MFMA adds
// (+-0) products to the row's accumulators.  An accumulator starts as +0 and x + (+-0) = x for every x but -0; a sum of f32 values is
// -0 only if every term is -0, the products are exact and the MFMA flushes neither its bf16 inputs nor its f32 result (gemm_bf16.hip,
// "Domain"), so an accumulator is never -0 and the skipped and the multiplied form give the same bits.
//
// Domain: as the lines of the gemm_bf16.hip header for activations (+-inf / NaN and values that round to a bf16 infinity give what IEEE
// arithmetic gives on the ROUNDED operands of the row's OWN pairs -- a non-finite input row reaches exactly the output rows whose
// rulebook column holds it, because every other row multiplies zeros from the descriptor, not that row; bf16 subnormals are kept).
// Non-finite WEIGHTS are outside the domain: a row without a pair at an offset multiplies 0 x W[k] there, which must be 0.
// Limits: the layer shapes srf_spconv_shape (spconv_frame.hpp) gives the bf16 form, inputs below 2 GiB (32-bit buffer offsets).
//
// Structure: output-stationary.  A workgroup = 4 waves x 32 consecutive output rows; a wave keeps its 32 x COUT accumulators in
// registers (COUT / 32 tiles of v_mfma_f32_32x32x16_bf16).  Lane (row r = lane & 31, half h = lane >> 5) of that MFMA holds the
// channels 16 s + 8 h .. + 7 of row r: 32 consecutive bytes of the gathered f32 row, two buffer_load_b128 and four v_cvt_pk_bf16_f32,
// no LDS trip for A.  The rows of offset k + 1 are requested before the MFMAs of offset k.  An offset's weights (CIN x COUT bf16, at most
// 32 KB, packed as [k][step s][column tile n][lane][8 bf16]: a fragment is one conflict-free ds_read_b128) are shared by the four
// waves through two LDS images: the image of the next used offset goes global -> registers before the MFMAs and registers -> LDS
// behind them, one barrier per offset.  The tile's rulebook columns sit in LDS (27 x 128 ints); offsets no row of the workgroup has
// are not staged at all.
#include "spconv_frame.hpp"

#define SB_ROWS 128   // output rows of a workgroup: 4 waves x 32

typedef __bf16 sb_bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 sb_bf8 __attribute__((ext_vector_type(8)));
typedef float sb_f2 __attribute__((ext_vector_type(2)));
typedef float sb_f4 __attribute__((ext_vector_type(4)));
typedef float sb_f16 __attribute__((ext_vector_type(16)));
typedef unsigned sb_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned sb_pk_bf16(float a, float b)
{
    const sb_f2 v = {a, b};
    const sb_bf2 h = __builtin_convertvector(v, sb_bf2);   // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
    return *reinterpret_cast<const unsigned *>(&h);
}

// W (K, Cin, Cout) f32 -> P[k][s = Cin / 16][n = Cout / 32][lane 64][j 8] bf16 = W[k][16 s + 8 (lane >> 5) + j][32 n + (lane & 31)]
__global__ __launch_bounds__(256) void srf_spconv_bf16_pack_k(const float *__restrict__ W, int Cin, int Cout, unsigned short *__restrict__ P,
                                                             int total)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int j = t & 7, lane = (t >> 3) & 63, NT = Cout / 32, NS = Cin / 16;
    const int rest = t >> 9;
    const int n = rest % NT, s = (rest / NT) % NS, k = rest / (NT * NS);
    const int c = 16 * s + 8 * (lane >> 5) + j, col = 32 * n + (lane & 31);
    P[t] = (unsigned short)(sb_pk_bf16(W[((size_t)k * Cin + c) * Cout + col], 0.f) & 0xffffu);
}

template <int CIN, int COUT>
__global__ __launch_bounds__(256, 2) void srf_spconv_bf16_k(const float *__restrict__ in, int A_in, const unsigned char *__restrict__ Wp, int K,
                                                          const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                          const float *__restrict__ alpha, const float *__restrict__ beta,
                                                          const float *__restrict__ residual, int relu, float *__restrict__ out,
                                                          const int *__restrict__ rows_dev)
{
    constexpr int NS = CIN / 16, NT = COUT / 32, IMG = CIN * COUT * 2, NLD = IMG / 4096;
    constexpr int PH = NLD > 4 ? 2 : 1, NLP = NLD / PH;   // a 32 KB image is staged in two parts: 16 registers in flight, not 32
    static_assert(IMG % 4096 == 0, "an image is copied as 16 bytes per thread and round");
    __shared__ __attribute__((aligned(16))) unsigned char s_b[2 * IMG];
    __shared__ int s_nbr[SRF_KMAX * SB_ROWS];
    __shared__ unsigned s_mask;

    A_out = srf_live_rows(A_out, rows_dev);
    const int n_tiles = (A_out + SB_ROWS - 1) / SB_ROWS;
    if ((int)blockIdx.x >= n_tiles) return;
    const int row0 = srf_xcd_tile(blockIdx.x, n_tiles) * SB_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;

    if (tid == 0) s_mask = 0u;
    for (int e = tid; e < K * SB_ROWS; e += 256) {
        const int k = e / SB_ROWS, row = row0 + (e % SB_ROWS);
        const int v = row < A_out ? nbr[(size_t)k * nbr_stride + row] : -1;
        s_nbr[e] = (unsigned)v < (unsigned)A_in ? v : -1;   // an entry outside the input is no pair
    }
    __syncthreads();
    unsigned wmask = 0u;   // the offsets any of this wave's 32 rows has
    for (int k = 0; k < K; ++k)
        if (__ballot(s_nbr[k * SB_ROWS + wave * 32 + r] >= 0) != 0ull) wmask |= 1u << k;
    if (lane == 0 && wmask) atomicOr(&s_mask, wmask);
    __syncthreads();
    unsigned m = __builtin_amdgcn_readfirstlane(s_mask);   // the offsets any row of the workgroup has

    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)((long long)A_in * CIN * 4), 0x00020000);
    sb_f16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[n][j] = 0.0f;
    sb_f4 raw[NS][2];   // the lane's 8 channels of every step of the NEXT offset's row, f32 as loaded
    sb_u4 breg[NLP];    // this thread's share of one part of the NEXT offset's weight image

#define SB_LOAD_B(KK, PART)                                                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < NLP; ++i_)                                                                          \
        breg[i_] = *reinterpret_cast<const sb_u4 *>(Wp + (size_t)(KK) * IMG + ((PART) * NLP + i_) * 4096 + tid * 16);
#define SB_LOAD_A(KK)                                                                                                          \
    {                                                                                                                          \
        const int v_ = s_nbr[(KK) * SB_ROWS + wave * 32 + r];                                                                   \
        const unsigned vo_ = v_ >= 0 ? (unsigned)v_ * (CIN * 4) + h * 32 : 0x80000000u;   /* out of range: zeros, no memory access */ \
        _Pragma("unroll") for (int s_ = 0; s_ < NS; ++s_)                                                                       \
            _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) {                                                                  \
                auto t_ = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(vo_ + s_ * 64 + q_ * 16), 0, 0);                      \
                raw[s_][q_] = *reinterpret_cast<sb_f4 *>(&t_);                                                                  \
            }                                                                                                                  \
    }
#define SB_STORE_B(BUF, PART)                                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < NLP; ++i_)                                                                          \
        *reinterpret_cast<sb_u4 *>(s_b + (BUF) * IMG + ((PART) * NLP + i_) * 4096 + tid * 16) = breg[i_];

    int buf = 0;
    if (m) {
        const int k0 = __builtin_ctz(m);
        SB_LOAD_A(k0)
#pragma unroll
        for (int ph = 0; ph < PH; ++ph) {
            SB_LOAD_B(k0, ph)
            SB_STORE_B(0, ph)
        }
        __syncthreads();
    }
    while (m) {
        const int k = __builtin_ctz(m);
        m &= m - 1;
        const int kn = m ? __builtin_ctz(m) : k;   // (the last offset requests itself again: nothing in the loop is conditional)
        sb_bf8 a[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const sb_u4 p = {sb_pk_bf16(raw[s][0][0], raw[s][0][1]), sb_pk_bf16(raw[s][0][2], raw[s][0][3]),
                             sb_pk_bf16(raw[s][1][0], raw[s][1][1]), sb_pk_bf16(raw[s][1][2], raw[s][1][3])};
            a[s] = *reinterpret_cast<const sb_bf8 *>(&p);
        }
        const bool has = (wmask & (1u << k)) != 0u;
        const unsigned char *img = s_b + buf * IMG + lane * 16;
#pragma unroll
        for (int ph = 0; ph < PH; ++ph) {
            SB_LOAD_B(kn, ph)
            if (ph == 0) SB_LOAD_A(kn)
            if (has) {
#pragma unroll
                for (int s = ph * (NS / PH); s < (ph + 1) * (NS / PH); ++s) {
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const sb_bf8 b = *reinterpret_cast<const sb_bf8 *>(img + (s * NT + n) * 1024);
                        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b, acc[n], 0, 0, 0);
                    }
                    asm volatile("" ::: "memory");   // fragments of one step in flight, not of all of them (registers)
                }
            }
            SB_STORE_B(buf ^ 1, ph)   // last read before the barrier that ended the previous offset
        }
        __syncthreads();
        buf ^= 1;
    }
#undef SB_LOAD_B
#undef SB_LOAD_A
#undef SB_STORE_B

    // epilogue: register j of a tile is row (j & 3) + 8 (j >> 2) + 4 h, the lane's column is 32 n + r
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = 32 * n + r;
        float al = 1.f, be = 0.f;
        if (alpha) {
            al = alpha[col];
            be = beta[col];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = row0 + wave * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
            if (row >= A_out) continue;
            out[(size_t)row * COUT + col] = srf_spconv_epilogue(acc[n][j], alpha, al, be, residual, [&] { return residual[(size_t)row * COUT + col]; }, relu);
        }
    }
}

extern "C" size_t srf_spconv_bf16_packed_weight_bytes(int K, int Cin, int Cout)
{
    return srf_spconv_shape(K, Cin, Cout).bf16 ? (size_t)K * Cin * Cout * 2 : 0;
}

extern "C" int srf_spconv_bf16_pack_weights(const float *W, int K, int Cin, int Cout, void *packed, srf_stream_t stream)
{
    if (!W || !packed || K <= 0 || K > SRF_KMAX || Cin <= 0 || Cout <= 0) return SRF_EINVAL;
    if (!srf_spconv_shape(K, Cin, Cout).bf16) return SRF_EUNSUPPORTED;
    const int total = K * Cin * Cout;
    hipLaunchKernelGGL(srf_spconv_bf16_pack_k, dim3(srf_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, W, Cin, Cout,
                       (unsigned short *)packed, total);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

extern "C" int srf_spconv_fwd_bf16(const float *in, int A_in, int Cin, const void *W_packed, int K, const int *nbr, int nbr_stride,
                                   int A_out, int Cout, const float *alpha, const float *beta, const float *residual, int relu,
                                   float *out, const int *rows_dev, const int *tiles, srf_stream_t stream)
{
    (void)tiles;   // no row plan: equal-height tiles (every row's bits are its own, see the header)
    // 32-bit buffer offsets into the input (range32)
    const int rc = srf_spconv_check({srf_spconv_shape(K, Cin, Cout).bf16, false, true}, in, A_in, Cin, W_packed, K, nbr, nbr_stride, A_out, Cout,
                                    alpha, beta, out);
    if (rc != SRF_OK || A_out == 0) return rc;
    const dim3 grid((unsigned)srf_ceil_div(A_out, SB_ROWS));
#define SB_LAUNCH(CIN, COUT)                                                                                                              \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_bf16_k<CIN, COUT>), grid, dim3(256), 0, (hipStream_t)stream, in, A_in,                    \
                       (const unsigned char *)W_packed, K, nbr, nbr_stride, A_out, alpha, beta, residual, relu, out, rows_dev)
    if (Cout == 64) {
        if (Cin == 32) SB_LAUNCH(32, 64);
        else SB_LAUNCH(64, 64);
    } else {
        if (Cin == 64) SB_LAUNCH(64, 128);
        else SB_LAUNCH(128, 128);
    }
#undef SB_LAUNCH
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
