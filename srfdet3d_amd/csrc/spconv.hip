// spconv.hip -- K5 sparse convolution forward on the f32 MFMA pipe, K6 densify (gfx950).
//
// Reference call sites: every SubMConv3d / SparseConv3d (+ BN1d + ReLU, + residual in SparseBasicBlock) of
// SparseEncoderCustom.forward, mmdet3d_plugin/models/middle_encoders/sparse_encoder_custom.py:125-134, and
// SparseConvTensor.dense() at :135-138.
//
// Output-stationary implicit GEMM.  A workgroup owns TM consecutive output rows and all COUT columns; for each
// kernel offset k (skipped when no row of the tile has a neighbour at k) it gathers the TM input rows named by
// nbr[k][.] into LDS in 32-channel chunks next to the matching 32 x COUT slab of W[k], and accumulates with
// v_mfma_f32_32x32x2_f32 (v_mfma_f32_16x16x4_f32 for COUT = 16).  Missing neighbours contribute exact zeros.
// The f32 MFMA is a k-ordered fma chain, so every output element is the chain over (k ascending, c ascending)
// that oracle/srf_oracle.c:orc_spconv_fwd forms -- results compare exactly.  Each output row is written once,
// with the epilogue of spconv_frame.hpp (eval-BatchNorm, residual add, ReLU) applied in registers.
//
// LDS per workgroup (COUT = 128): nbr tile 27*64*4 = 6.9 KB, A chunk 64*33*4 = 8.4 KB, W chunk 32*128*4 = 16 KB
// -> 5 workgroups per CU; latency is hidden by occupancy rather than by an explicit pipeline.
#include "spconv_frame.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SRF_KC 32

template <int TM, int COUT>
__device__ __forceinline__ void srf_stage_tile(const float *__restrict__ in, int Cin, const float *__restrict__ Wk, int c0,
                                               const int *s_nbr_k, float (*s_a)[SRF_KC + 1], float (*s_w)[COUT])
{
    const int tid = threadIdx.x;
    const bool vec = (Cin & 3) == 0;
    // gathered input rows: 8 threads per row, one float4 each
    for (int e = tid; e < TM * (SRF_KC / 4); e += 256) {
        const int r = e / (SRF_KC / 4), q = e % (SRF_KC / 4);
        const int i = s_nbr_k[r];
        const int c = c0 + q * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= 0 && c < Cin) {
            const float *src = in + (size_t)i * Cin + c;
            if (vec) {
                v = *reinterpret_cast<const float4 *>(src);
            } else {
                v.x = src[0];
                if (c + 1 < Cin) v.y = src[1];
                if (c + 2 < Cin) v.z = src[2];
                if (c + 3 < Cin) v.w = src[3];
            }
        }
        float *dst = &s_a[r][q * 4];
        dst[0] = v.x;
        dst[1] = v.y;
        dst[2] = v.z;
        dst[3] = v.w;
    }
    // weight slab: rows c0..c0+31 of W[k] (Cin x COUT), zero beyond Cin
    for (int e = tid; e < SRF_KC * (COUT / 4); e += 256) {
        const int c = e / (COUT / 4), j = e % (COUT / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 + c < Cin) v = *reinterpret_cast<const float4 *>(Wk + (size_t)(c0 + c) * COUT + j * 4);
        *reinterpret_cast<float4 *>(&s_w[c][j * 4]) = v;
    }
}

template <int TM>
__device__ __forceinline__ void srf_load_nbr_tile(const int *__restrict__ nbr, int nbr_stride, int K, int row0, int A_out,
                                                  int *s_nbr, int *s_any)
{
    if (threadIdx.x < SRF_KMAX) s_any[threadIdx.x] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < K * TM; t += 256) {
        const int k = t / TM, r = t % TM;
        const int row = row0 + r;
        const int v = row < A_out ? nbr[(size_t)k * nbr_stride + row] : -1;
        s_nbr[t] = v;
        if (v >= 0) s_any[k] = 1;  // benign race: every writer stores 1
    }
    __syncthreads();
}

// ---- pipelined wide kernel (COUT in {32, 64, 128}) ------------------------------------------------------------------
// Branch-free loads (Cin % 4 == 0 is required by the launcher): a missing neighbour or a channel beyond Cin reads a
// valid clamped address and is zeroed by a select, so all loads of a step stay in flight together.  The staging
// registers are native vectors (f32x4), not HIP's float4 struct: arrays of the union-based struct are not split into
// registers by the compiler and end up round-tripping through LDS.
template <int COUT, int TM, int NA, int NW>
__device__ __forceinline__ void srf_step_load(const float *__restrict__ in, int Cin, const float *__restrict__ W,
                                              const int *nbr_k /* this offset's TM entries: LDS tile or nbr + k*stride + row0 */, int rows_left,
                                              int k, int c0, f32x4 (&ra)[NA], f32x4 (&rw)[NW], unsigned &okmask)
{
    const int tid = threadIdx.x;
    const float *Wk = W + (size_t)k * Cin * COUT;
    // the zeroing select is applied at store time (srf_step_store): touching the loaded value here would make the
    // compiler wait for the load before the MFMA block it is meant to overlap
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int e = tid + j * 256;
        const int r = e / (SRF_KC / 4), q = e % (SRF_KC / 4);
        const int i = r < rows_left ? nbr_k[r] : -1;  // L2-resident; 8 lanes share one entry
        const int c = c0 + q * 4;
        const bool ok = (i >= 0) & (c < Cin);
        const int ii = i >= 0 ? i : 0;
        const int cc = c < Cin ? c : Cin - 4;
        ra[j] = *reinterpret_cast<const f32x4 *>(in + (size_t)ii * Cin + cc);
        m |= (ok ? 1u : 0u) << j;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int e = tid + j * 256;
        const int c = e / (COUT / 4), q = e % (COUT / 4);
        const bool ok = c0 + c < Cin;
        const int cc = ok ? c0 + c : Cin - 1;
        rw[j] = *reinterpret_cast<const f32x4 *>(Wk + (size_t)cc * COUT + q * 4);
        m |= (ok ? 1u : 0u) << (NA + j);
    }
    okmask = m;
}

template <int COUT, int TM, int NA, int NW>
__device__ __forceinline__ void srf_step_store(float (*s_a)[SRF_KC + 1], float (*s_w)[COUT], const f32x4 (&ra)[NA],
                                               const f32x4 (&rw)[NW], unsigned okmask)
{
    const int tid = threadIdx.x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int e = tid + j * 256;
        float *dst = &s_a[e / (SRF_KC / 4)][(e % (SRF_KC / 4)) * 4];
        const f32x4 v = ((okmask >> j) & 1u) ? ra[j] : zero;
        dst[0] = v[0];
        dst[1] = v[1];
        dst[2] = v[2];
        dst[3] = v[3];
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int e = tid + j * 256;
        *reinterpret_cast<f32x4 *>(&s_w[e / (COUT / 4)][(e % (COUT / 4)) * 4]) = ((okmask >> (NA + j)) & 1u) ? rw[j] : zero;
    }
}

// Waves arranged WR x WC, each owning 32 x (CT*32) outputs.  Software pipeline: the global loads of step t+1 (gathered
// rows + W slab, held in registers) are in flight while the MFMAs of step t run from LDS buffer t&1; they are written
// to buffer (t+1)&1 afterwards; one barrier per step.  Steps enumerate (active kernel offset, 32-channel chunk)
// pairs; offsets that no row of the tile uses are not visited.  A chunk is always 32 deep (zero padded), so the MFMA
// loop is fully unrolled and its LDS reads are hoisted ahead of the MFMAs by the compiler.
template <int COUT, int TM, int WR, int WC>
__global__ __launch_bounds__(256) void srf_spconv_mfma32_k(const float *__restrict__ in, int Cin,
                                                         const float *__restrict__ W, int K,
                                                         const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                         const float *__restrict__ alpha, const float *__restrict__ beta,
                                                         const float *__restrict__ residual, int relu,
                                                         float *__restrict__ out, const int *__restrict__ rows_dev)
{
    static_assert(WR * WC == 4 && TM == WR * 32, "one 32-row tile per wave row");
    constexpr int CT = COUT / WC / 32;
    constexpr int NA = TM * (SRF_KC / 4) / 256;    // float4 gathers per thread and step
    constexpr int NW = SRF_KC * (COUT / 4) / 256;  // float4 weight loads per thread and step
    // COUT = 128 leaves the 27 x TM neighbour tile in L2 (it would cost the third resident workgroup per CU);
    // the narrower kernels have LDS to spare and keep it on chip
    constexpr bool NBR_LDS = COUT < 128;
    __shared__ int s_nbr[NBR_LDS ? SRF_KMAX * TM : 1];
    __shared__ int s_any[SRF_KMAX];
    __shared__ int s_klist[SRF_KMAX + 1];
    __shared__ float s_a[2][TM][SRF_KC + 1];
    __shared__ __attribute__((aligned(16))) float s_w[2][SRF_KC][COUT];

    A_out = srf_live_rows(A_out, rows_dev);
    // tiles of LIVE rows only, dealt XCD-contiguously over the first n_tiles workgroups (a capacity-sized launch must not
    // leave whole XCDs with nothing but padding)
    const int n_tiles = (A_out + TM - 1) / TM;
    if ((int)blockIdx.x >= n_tiles) return;
    const int row0 = srf_xcd_tile(blockIdx.x, n_tiles) * TM;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WC, wc = wave % WC;
    const int rows_left = A_out - row0;
    if (tid < SRF_KMAX) s_any[tid] = 0;
    __syncthreads();
    for (int t = tid; t < K * TM; t += 256) {
        const int k = t / TM, r = t % TM;
        const int v = r < rows_left ? nbr[(size_t)k * nbr_stride + row0 + r] : -1;
        if (NBR_LDS) s_nbr[t] = v;
        if (v >= 0) s_any[k] = 1;  // benign race: every writer stores 1
    }
    __syncthreads();
    if (tid < 64) {  // compact the used offsets with one ballot (K <= 27 < 64) instead of a serial loop on one lane
        const bool used = tid < K && s_any[tid];
        const unsigned long long m = __ballot(used);
        if (used) s_klist[__popcll(m & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) s_klist[SRF_KMAX] = __popcll(m);
    }
    __syncthreads();
    const int nchunk = (Cin + SRF_KC - 1) / SRF_KC;
    const int T = s_klist[SRF_KMAX] * nchunk;

    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[ct][j] = 0.0f;

    f32x4 ra[NA], rw[NW];
    unsigned okmask = 0;
    const int ar = wr * 32 + (lane & 31);
    const int kh = lane >> 5;
    if (T > 0) {
        const int k0 = s_klist[0];
        srf_step_load<COUT, TM, NA, NW>(in, Cin, W, NBR_LDS ? s_nbr + k0 * TM : nbr + (size_t)k0 * nbr_stride + row0,
                                        NBR_LDS ? TM : rows_left, k0, 0, ra, rw, okmask);
        srf_step_store<COUT, TM, NA, NW>(s_a[0], s_w[0], ra, rw, okmask);
    }
    __syncthreads();
    int tk = 0, tc = 0;  // (offset index, chunk index) of step t+1
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        if (++tc == nchunk) {
            tc = 0;
            ++tk;
        }
        const bool more = t + 1 < T;
        if (more) {
            const int kn = s_klist[tk];
            srf_step_load<COUT, TM, NA, NW>(in, Cin, W, NBR_LDS ? s_nbr + kn * TM : nbr + (size_t)kn * nbr_stride + row0,
                                            NBR_LDS ? TM : rows_left, kn, tc * SRF_KC, ra, rw, okmask);
        }
#pragma unroll
        for (int kk = 0; kk < SRF_KC; kk += 2) {
            const float a = s_a[buf][ar][kk + kh];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const float b = s_w[buf][kk + kh][(wc * CT + ct) * 32 + (lane & 31)];
                acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[ct], 0, 0, 0);
            }
        }
        if (more) srf_step_store<COUT, TM, NA, NW>(s_a[buf ^ 1], s_w[buf ^ 1], ra, rw, okmask);
        __syncthreads();
    }

    // epilogue: C/D layout of 32x32: col = lane & 31, row = (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int col = (wc * CT + ct) * 32 + (lane & 31);
        const float al = alpha ? alpha[col] : 1.0f;
        const float be = alpha ? beta[col] : 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = row0 + wr * 32 + (j & 3) + 8 * (j >> 2) + 4 * kh;
            if (row < A_out)
                out[(size_t)row * COUT + col] =
                    srf_spconv_epilogue(acc[ct][j], alpha, al, be, residual, [&] { return residual[(size_t)row * COUT + col]; }, relu);
        }
    }
}

// =====================================================================================================================
// Packed weights (inference: the weights are constants, so they are re-laid-out once per layer).  A layer shape has at most
// one packed layout, and srf_spconv_fwd_packed runs one kernel on it (the shapes: srf_spconv_shape, spconv_frame.hpp):
//   w32 -> srf_spconv_w32_k (srf_pack_weights_w32_k)         gs -> srf_spconv_gsp_k (srf_pack_weights_gs_k)
// =====================================================================================================================
extern "C" int srf_spconv_plan_kind(int K, int Cin, int Cout) { return srf_spconv_shape(K, Cin, Cout).plan; }

__global__ void srf_pack_weights_gs_k(const float *__restrict__ W, int K, int Cin, int Cout, int nchunk, float *__restrict__ P);

// wave-private layout of the 32-output-channel layers (srf_spconv_w32_k below): [k][group of 4 steps][channel parity][col 32][4]

__global__ __launch_bounds__(256) void srf_pack_weights_w32_k(const float *__restrict__ W, int K, int Cin, float *__restrict__ P)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int total = K * Cin * 32;
    if (t >= total) return;
    const int nb = Cin / 8;
    const int i = t & 3, col = (t >> 2) & 31, kh = (t >> 7) & 1;
    const int rest = t >> 8;
    const int sg = rest % nb, k = rest / nb;
    const int c = 2 * (4 * sg + i) + kh;   // MFMA step 4 sg + i multiplies the channels 2 s (lanes 0-31) and 2 s + 1 (lanes 32-63)
    P[t] = W[((size_t)k * Cin + c) * 32 + col];
}

extern "C" size_t srf_spconv_packed_weight_bytes(int K, int Cin, int Cout)
{
    if (srf_spconv_shape(K, Cin, Cout).packed == SRF_PACKED_NONE) return 0;
    return (size_t)K * ((Cin + 31) / 32) * Cout * 32 * sizeof(float);
}

extern "C" int srf_spconv_pack_weights(const float *W, int K, int Cin, int Cout, float *packed, srf_stream_t stream)
{
    if (!W || !packed || K <= 0 || K > SRF_KMAX || Cin <= 0 || Cout <= 0) return SRF_EINVAL;
    const SrfPackedLayout layout = srf_spconv_shape(K, Cin, Cout).packed;
    if (layout == SRF_PACKED_NONE) return SRF_EUNSUPPORTED;
    if (layout == SRF_PACKED_W32) {
        hipLaunchKernelGGL(srf_pack_weights_w32_k, dim3(srf_ceil_div((long long)K * Cin * 32, 256)), dim3(256), 0, (hipStream_t)stream, W, K,
                           Cin, packed);
    } else {
        const int nchunk = (Cin + 31) / 32;
        hipLaunchKernelGGL(srf_pack_weights_gs_k, dim3(srf_ceil_div((long long)K * nchunk * Cout * 32, 256)), dim3(256), 0, (hipStream_t)stream,
                           W, K, Cin, Cout, nchunk, packed);
    }
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// ---- compacted-offset kernel (srf_spconv_gsp_k below): tile height, co-resident workgroups -----------------------------
#define SRF_GS_TMAX 88   /* most output rows of a COUT = 128 tile: 2 workgroups per CU still fit in LDS */
#define SRF_GS_SLOTS 512 /* co-resident workgroups: 256 CUs x 2 */

// Tile height.  A tile is ~80 groups of MFMAs (~200 us): with a fixed height the last partial round of tiles would leave
// most of the chip idle for that long (547 tiles of 64 rows on 512 slots: 35 tiles run alone in a second round).  The
// height is therefore chosen from the live row count so that the tiles fill a whole number of rounds of 512: 1 round up
// to 45k rows, 2 rounds up to 90k, ...  Evaluated identically on the host (grid size from the capacity) and in the
// kernel (from the device row count of a static-shape level).
__host__ __device__ static inline int srf_gs_rounds(int A) { return A <= 0 ? 1 : (A + SRF_GS_SLOTS * SRF_GS_TMAX - 1) / (SRF_GS_SLOTS * SRF_GS_TMAX); }
__host__ __device__ static inline int srf_gs_tile_rows(int A)
{
    const int per = SRF_GS_SLOTS * srf_gs_rounds(A);
    int tm = ((A + per - 1) / per + 7) & ~7;
    return tm < 16 ? 16 : tm;
}

// gs layout: Wg[k][chunk][wc = col/32][g][lane][i], idx = 4g + i, = W[k][chunk*32 + 4*(idx&7) + (lane>>4)][wc*32 + 16*(idx>>3) + (lane&15)]
// (a lane's B operands of a chunk in MFMA issue order: each f32x4 of a wave is one coalesced 1 KB load)
__global__ __launch_bounds__(256) void srf_pack_weights_gs_k(const float *__restrict__ W, int K, int Cin, int Cout, int nchunk,
                                                           float *__restrict__ P)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)K * nchunk * Cout * 32;
    if (t >= total) return;
    const int i = (int)(t & 3), lane = (int)((t >> 2) & 63), g = (int)((t >> 8) & 3);
    const int per = Cout * 32;  // elements per (offset, chunk): Cout / 32 column blocks x 4 groups x 64 lanes x 4
    const int wc = (int)((t % per) >> 10);
    const long long rest = t / per;
    const int chunk = (int)(rest % nchunk), k = (int)(rest / nchunk);
    const int idx = 4 * g + i;
    const int col = wc * 32 + 16 * (idx >> 3) + (lane & 15);
    const int c = chunk * 32 + 4 * (idx & 7) + (lane >> 4);
    P[t] = c < Cin ? W[((size_t)k * Cin + c) * Cout + col] : 0.0f;
}

// ---- work-balanced row ranges ------------------------------------------------------------------------------------------
// One round of co-resident workgroups finishes when its heaviest tile does, and the pairs per 72 rows of a sweep vary by
// 1.5x around their mean (dense clusters vs. isolated returns).  srf_spconv_tiles_build therefore cuts the rows of a
// rulebook into T ranges of (almost) equal PAIR count -- range t = the rows whose exclusive pair prefix lies in
// [t*P/T, (t+1)*P/T) -- once per rulebook (the four SubM layers of a level share it).  A workgroup walks its range in
// sub-tiles of at most SRF_GS_TMAX rows.
#define SRF_TB_ROWS 256
#define SRF_GS_ROW_BASE 8 /* cost of a row = its pairs + 8: the constant carries the row's share of the per-sub-tile work (list
                             build, epilogue: ~20 k cycles per sub-tile against ~270 cycles per pair in the step loop of
                             srf_spconv_gsp_k) and keeps sparse ranges from growing taller than a tile, which costs a second
                             sub-tile (+35 k cycles).  Round 1's kernel, whose steps were twice as long, was fitted with 12.
                             Measured (round 5, in-kernel stamps + bench_spconv): 128 -> 128 (35k rows, 68 rows per range)
                             226 / 219 us with 12 / 4 on one box, 228 / 228 on another; 64 -> 64 (60k rows, 116 rows per range of
                             at most 128) 88 / 91.5 us: the taller the ranges of a level against its tile, the larger the constant
                             it wants */
__host__ __device__ static inline int srf_gs_ranges(int A_cap)
{
    const int t = A_cap / 32;
    return t < 1 ? 1 : (t > SRF_GS_SLOTS ? SRF_GS_SLOTS : t);
}

__device__ __forceinline__ int srf_block_scan_excl(int v, int *s_scan /* 256 + 4 */, int &total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_scan[wave] = x;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_scan[w];
    }
    total = s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
    __syncthreads();
    return base + x - v;
}

// cost per row, exclusive prefix inside blocks of SRF_TB_ROWS rows (row order), block totals
__global__ __launch_bounds__(256) void srf_gs_rowpairs_k(const int *__restrict__ nbr, int nbr_stride, int K, int A,
                                                       const int *__restrict__ rows_dev, int *__restrict__ local,
                                                       int *__restrict__ blocksum, int row_cost)
{
    __shared__ int s_scan[4];
    A = srf_live_rows(A, rows_dev);
    const int r0 = blockIdx.x * SRF_TB_ROWS;
    int carry = 0;
    for (int j = 0; j < SRF_TB_ROWS / 256; ++j) {  // block-uniform trip count: the barriers inside the scan are safe
        const int r = r0 + j * 256 + threadIdx.x;
        int c = 0;
        {
            // all K entries of the row in flight at once (as a loop of `c += nbr[..] >= 0` every entry was its own round trip: 27 in a
            // row, the whole of this 9-10 us launch); rows past the end read row A - 1 and count nothing
            const int rc = r < A ? r : (A > 0 ? A - 1 : 0);   // (A == 0, a level without live rows: row 0 of the capacity-sized table, counted as nothing)
            int v[SRF_KMAX];
#pragma unroll
            for (int k = 0; k < SRF_KMAX; ++k) v[k] = nbr[(size_t)(k < K ? k : K - 1) * nbr_stride + rc];
#pragma unroll
            for (int k = 0; k < SRF_KMAX; ++k) c += (k < K && v[k] >= 0) ? 1 : 0;
            c = r < A ? c + row_cost : 0;
        }
        int total;
        const int ex = srf_block_scan_excl(c, s_scan, total);
        if (r < A) local[r] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) blocksum[blockIdx.x] = carry;
}

// exclusive scan of the block totals (one workgroup; nb <= a few hundred), total pair count at [nb]
__global__ __launch_bounds__(256) void srf_gs_blockscan_k(const int *__restrict__ blocksum, int nb, int *__restrict__ blockoff)
{
    __shared__ int s_scan[4];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? blocksum[b] : 0;
        int total;
        const int ex = srf_block_scan_excl(v, s_scan, total);
        if (b < nb) blockoff[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) blockoff[nb] = carry;
}

// tiles[t] = first row whose exclusive pair prefix reaches t*P/T (binary search over blocks, then inside the block)
__global__ __launch_bounds__(256) void srf_gs_cut_k(const int *__restrict__ local, const int *__restrict__ blockoff, int nb, int A,
                                                  const int *__restrict__ rows_dev, int T, int *__restrict__ tiles)
{
    A = srf_live_rows(A, rows_dev);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t > T) return;
    const int nbl = (A + SRF_TB_ROWS - 1) / SRF_TB_ROWS;  // live blocks (<= nb)
    if (t == T || A == 0) {
        tiles[t] = A;
        return;
    }
    const long long P = blockoff[nbl];
    const long long target = (P * t + T - 1) / T;
    // last block whose offset is <= target
    int lo = 0, hi = nbl - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blockoff[mid] <= target) lo = mid;
        else hi = mid - 1;
    }
    const long long boff = blockoff[lo];
    const int r0 = lo * SRF_TB_ROWS;
    const int r1 = r0 + SRF_TB_ROWS < A ? r0 + SRF_TB_ROWS : A;
    // first row in [r0, r1) with boff + local[r] >= target, else r1
    int a = r0, b = r1;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (boff + local[mid] >= target) b = mid;
        else a = mid + 1;
    }
    tiles[t] = a;
}

extern "C" int srf_spconv_tiles_count(int A_out) { return A_out <= 0 ? 1 : srf_gs_ranges(A_out); }

extern "C" int srf_spconv_tiles_row_cost(void) { return SRF_GS_ROW_BASE; }

extern "C" size_t srf_spconv_tiles_workspace_bytes(int A_out)
{
    if (A_out < 0) return 0;
    const size_t nb = (size_t)(A_out + SRF_TB_ROWS - 1) / SRF_TB_ROWS;
    return ((size_t)A_out + 2 * nb + 8) * sizeof(int);
}

extern "C" int srf_spconv_tiles_build(const int *nbr, int nbr_stride, int K, int A_out, const int *rows_dev, void *workspace,
                                      int *tiles, srf_stream_t stream)
{
    if (A_out < 0 || K <= 0 || K > SRF_KMAX || nbr_stride < A_out || !tiles) return SRF_EINVAL;
    if (A_out > 0 && (!nbr || !workspace)) return SRF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int T = srf_spconv_tiles_count(A_out);
    const int nb = (A_out + SRF_TB_ROWS - 1) / SRF_TB_ROWS;
    int *local = (int *)workspace, *blocksum = local + A_out, *blockoff = blocksum + nb + 1;
    if (nb > 0) {
        hipLaunchKernelGGL(srf_gs_rowpairs_k, dim3(nb), dim3(256), 0, st, nbr, nbr_stride, K, A_out, rows_dev, local, blocksum, SRF_GS_ROW_BASE);
        hipLaunchKernelGGL(srf_gs_blockscan_k, dim3(1), dim3(256), 0, st, blocksum, nb, blockoff);
    }
    hipLaunchKernelGGL(srf_gs_cut_k, dim3(srf_ceil_div(T + 1, 256)), dim3(256), 0, st, local, blockoff, nb, A_out, rows_dev, T, tiles);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// =====================================================================================================================
// srf_spconv_gsp_k: the packed kernel of the layers with COUT = 128 (Cin = 64 / 128: the SubM layers of the last level, the
// strided 64 -> 128, `conv_out`) and COUT = 64 (Cin = 32 / 64), any K.  Compacted offsets ("gs": gather rows, scatter into an
// LDS-resident output tile):
//   * only 16-20 of the 27 neighbours of a row exist, so an output-stationary tile, which runs one MFMA pass per offset any of its
//     rows uses, spends ~40 % of its MFMAs on zeros.  Here a workgroup owns up to TMAX output rows (SRF_GS_TMAX = 88 for
//     COUT = 128, 128 for COUT = 64) whose accumulators live in LDS.  For every offset k the rows that HAVE a neighbour at k are
//     compacted (one ballot per 64 rows) and processed in groups of 16 on v_mfma_f32_16x16x4_f32: the group's accumulators are read
//     from the output tile (row = the group's output slot), run through the channel-ascending MFMA chain and written back;
//   * every output element therefore sees exactly the chain (offset ascending, channel ascending, one fma per term) of
//     oracle/srf_oracle.c:orc_spconv_fwd, minus terms that are exact zeros: results are bit-identical to srf_spconv_fwd and to the
//     oracle;
//   * a wave owns 32 (COUT = 128) or 16 (COUT = 64) output channels of the tile, so no other wave touches its accumulators.  Its B
//     operands (gs layout, srf_pack_weights_gs_k) go global(L2) -> registers once per offset and tile, one offset ahead in a second
//     register set;
//   * A image of a group of 16 rows: [chunk][row 0..15][32], channel 4q + j of a chunk at position j*8 + q (lane (row, j) of the
//     16x16x4 MFMA reads its eight steps as two b128), 16-byte units XOR-swizzled by (row >> 1) & 7;
//   * LDS: the output tile ((TMAX + 1 spare row for padding slots) x (COUT + 4) floats), two A images, the flat step list below:
//     58 KB (32 -> 64) to 76 KB (128 -> 128) -> two workgroups per CU (__launch_bounds__(256, 2), SRF_GS_SLOTS);
//   * which rows a workgroup owns: one range of srf_spconv_tiles_build (equal cost), or one equal-height tile (srf_gs_tile_rows)
//     when the caller passes no ranges; either is walked in sub-tiles of at most TMAX rows.
// The step is SOFTWARE-PIPELINED, so that every wave's MFMA block is the only thing it waits for:
//   * the rows of ALL offsets of a sub-tile form ONE flat list of steps (per offset padded to whole groups of 16; s_pin holds
//     the byte offset of the input row, s_pslot the output slot): step i's rows are entries 16 i .. 16 i + 15 whatever its
//     offset, so looking two steps ahead is plain address arithmetic;
//   * step i issues, in this order: the chunk-0 fragments of A[i]; the LDS stores of A[i + 1] (gathered during step i - 1:
//     landed long ago, no wait); the gather of step i + 2; then per 32-channel chunk the fragment reads of the NEXT chunk
//     followed by the chunk's MFMAs (fragments double-buffered per chunk: 16 registers instead of 32), the output slots of
//     step i + 1 inside the first chunk; accumulators of step i back to the tile and those of step i + 1 out of it (the
//     same wave's LDS operations execute in order, so rows shared by the two steps are read after they were written);
//     barrier.  LDS instructions issued between the MFMAs of the own wave cost ~1 cycle per MFMA; what stays exposed per
//     step is one LDS latency behind the barrier and the accumulator round trip;
//   * address arithmetic per step: rows are gathered through a buffer descriptor (32-bit offset row + quad: one add per
//     load, padding entries are out-of-range offsets that read zeros without touching memory; hence inputs below 2 GiB), the
//     store addresses of the A image are precomputed per thread: ~20 vector instructions per step (they take MFMA issue time
//     on this chip);
//   * the last step of an offset is a separate instantiation (LAST) that also fetches the next offset's B operands into the
//     other register set right behind the gather: no branch inside a step, the compiler's vmcnt bookkeeping stays exact.
// The flat lists carry two dummy steps behind the real ones (zeros into the spare row), so nothing in a step is conditional.
// =====================================================================================================================

typedef __attribute__((address_space(3))) float srf_lds_float;
typedef __attribute__((address_space(3))) f32x4 srf_lds_f32x4;
__device__ __forceinline__ unsigned srf_lds_addr(const void *p) { return (unsigned)(uintptr_t)p; }   // LDS byte address of a __shared__ object

// per-thread constants of a step (LDS byte addresses for buffer 0 of the A image; the other buffer is `abuf_bytes` further)
struct SrfGspLane {
    unsigned fo0, fo1;     // the lane's two fragment quads inside chunk 0
    unsigned sto[4];       // where the four floats of the lane's first gathered quad go (its second quad: two chunks further)
    unsigned goff;         // byte offset of that quad inside the input row
    unsigned colbase;      // LDS byte address of (slot 0, the lane's first column) of the output tile
    unsigned boff;         // byte offset of the lane's B fragment inside a (offset, chunk) image
};

// what a wave carries from step to step: every address the LDS-only parts of a step use is prepared INSIDE the MFMA block before
struct SrfGspRegs {
    unsigned f0, f1;          // fragment quads of the A image the step reads
    unsigned st[4];           // where it stores the rows of the step after it
    unsigned gaddr;           // buffer offset of the row it requests (step + 2)
    unsigned oaddr[4];        // tile addresses of its accumulators
    unsigned pin_addr;        // LDS address of the row-list entries it reads (step + 3: the request after next)
    unsigned slot_addr;       // LDS address of the slots it reads (step + 1)
    unsigned info_addr;       // LDS address of the offset flag it reads (step + 1)
};

// A step multiplies one group of 16 rows.  Steps of two groups (for COUT = 64, where a wave owns ONE 16-column MFMA tile: two
// independent MFMA chains per step and half the barriers) measured slower: the rows of an offset are padded to whole steps, and
// the padding grew by 27 %.
template <int NCH, int COUT, bool LAST>
__device__ __forceinline__ void srf_gsp_step(__amdgpu_buffer_rsrc_t rs, __amdgpu_buffer_rsrc_t wrs, int kn, int &buf, const SrfGspLane &L,
                                             SrfGspRegs &G, f32x4 (&bc)[NCH][COUT / 32], f32x4 (&bn)[NCH][COUT / 32],
                                             f32x4 (&ra)[NCH >= 2 ? NCH / 2 : 1], f32x4 (&acc)[COUT / 64], int &info_next)
{
    constexpr int NT = COUT / 64, NB = COUT / 32, NA = NCH >= 2 ? NCH / 2 : 1, RS = 16, CHS = RS * 32 + 8, OS = COUT + 4;
    constexpr int TPR = NCH >= 2 ? 16 : 8;     // threads per gathered row (a quad each; rows of 128 channels: two quads each)
    constexpr unsigned ABUF = NCH * CHS * 4;   // bytes of one A buffer
    typedef const __attribute__((address_space(3))) unsigned srf_lds_u32;
    const bool gathers = TPR == 16 || threadIdx.x < 16 * TPR;   // 32-channel rows: 128 threads (two waves) carry a group of 16 rows
    // ---- LDS / memory instructions only.  In-kernel stamps (the ping-pong experiment, tools/micro/spconv_gsq_experiment.patch): a wave
    // issues NO vector instruction while the partner wave of its SIMD -- here: the CU's other workgroup -- streams f32 MFMAs, at any
    // s_setprio; a step whose first instruction is an address add therefore stands still until the partner's MFMA block is over, and
    // the two workgroups take turns instead of overlapping.  Every address below comes out of registers prepared inside this
    // wave's own previous MFMA block ----
    f32x4 af[2][2];
    af[0][0] = *reinterpret_cast<const srf_lds_f32x4 *>(G.f0);
    af[0][1] = *reinterpret_cast<const srf_lds_f32x4 *>(G.f1);
    const unsigned ro = *reinterpret_cast<srf_lds_u32 *>(G.pin_addr);     // list entries of step i + 3
    const unsigned sl4 = *reinterpret_cast<srf_lds_u32 *>(G.slot_addr);   // slots of step i + 1
    const unsigned inf = *reinterpret_cast<const __attribute__((address_space(3))) unsigned char *>(G.info_addr);  // ... and its offset flag
    if (gathers) {
        // A[i + 1]: rows gathered during step i - 1, into the buffer the previous step read
#pragma unroll
        for (int j = 0; j < NA; ++j)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) *reinterpret_cast<srf_lds_float *>(G.st[jj] + j * (2 * CHS * 4)) = ra[j][jj];
        // rows of step i + 2 (dummy steps behind the last one: out-of-range offsets, zeros)
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)G.gaddr + j * 256, 0, 0);
            ra[j] = *reinterpret_cast<f32x4 *>(&v);
        }
    }
    if (LAST) {   // B of the next offset into the other register set, a whole step ahead (through a descriptor: not an invariant
                  // load the compiler may sink to its first use behind the barrier)
        const int so = kn * (NCH * NB * 4096);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int g = 0; g < NB; ++g) {
                auto v = __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)(L.boff + g * 1024), so + c * (NB * 4096), 0);
                bn[c][g] = *reinterpret_cast<f32x4 *>(&v);
            }
    }
    unsigned oaddr_n[4];
    __builtin_amdgcn_sched_barrier(0);
    // ---- the MFMA block: fragments of the next chunk requested a chunk ahead; the vector instructions of the step in its last chunk ----
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) {
            af[(c + 1) & 1][0] = *reinterpret_cast<const srf_lds_f32x4 *>(G.f0 + (c + 1) * (CHS * 4));
            af[(c + 1) & 1][1] = *reinterpret_cast<const srf_lds_f32x4 *>(G.f1 + (c + 1) * (CHS * 4));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float a = af[c & 1][s >> 2][s & 3];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc[c][s >> 2][s & 3], acc[0], 0, 0, 0);
            if (NT == 2) acc[NT - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bc[c][NB - 2 + (s >> 2)][s & 3], acc[NT - 1], 0, 0, 0);
            if (c == NCH - 1 && s == 3) {
                // (all fragment reads of the step are issued: the address registers are free to move on)
                __builtin_amdgcn_sched_barrier(0);
                buf ^= 1;
                const int d = buf ? (int)ABUF : -(int)ABUF;   // the A buffers swap roles
                unsigned inf_here = inf;   // (opaque copies: the arithmetic on the loaded values must not be hoisted to the loads)
                asm volatile("" : "+v"(inf_here));
                info_next = __builtin_amdgcn_readfirstlane((int)inf_here);
                G.f0 += d;
                G.f1 += d;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) G.st[jj] -= d;
                unsigned ro_here = ro, sl_here = sl4;
                asm volatile("" : "+v"(ro_here), "+v"(sl_here));
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) oaddr_n[jj] = ((sl_here >> (8 * jj)) & 255u) * (unsigned)(OS * 4) + L.colbase;
                G.gaddr = ro_here + L.goff;
                asm volatile("" : "+v"(G.gaddr), "+v"(oaddr_n[0]), "+v"(oaddr_n[1]), "+v"(oaddr_n[2]), "+v"(oaddr_n[3]));
                G.pin_addr += RS * 4;
                G.slot_addr += RS;
                G.info_addr += 1;
                asm volatile("" : "+v"(G.f0), "+v"(G.f1), "+v"(G.st[0]), "+v"(G.st[1]), "+v"(G.st[2]), "+v"(G.st[3]), "+v"(G.pin_addr),
                             "+v"(G.slot_addr), "+v"(G.info_addr));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // ---- LDS only again: accumulators of step i back into the tile, those of step i + 1 out of it (in-order LDS: shared rows are
    // read after they were written); plain ds_read_b32 in assembly (the compiler pairs its own as ds_read2 and then shuffles
    // registers behind a wait).  The compiler counts none of these reads: nothing touches t[][] until the wait statement in front
    // of the barrier, which names every one of them, has retired the reads together with the stores; acc is assigned behind it ----
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int cb = 0; cb < NT; ++cb) *reinterpret_cast<srf_lds_float *>(G.oaddr[jj] + cb * 64) = acc[cb][jj];
    __builtin_amdgcn_sched_barrier(0);
    float t[NT][4];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (cb == 0) asm volatile("ds_read_b32 %0, %1" : "=v"(t[cb][jj]) : "v"(oaddr_n[jj]) : "memory");
            else asm volatile("ds_read_b32 %0, %1 offset:64" : "=v"(t[cb][jj]) : "v"(oaddr_n[jj]) : "memory");
        }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) G.oaddr[jj] = oaddr_n[jj];   // (a renaming: the copies, if any, land in the next MFMA block)
    if constexpr (NT == 1)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0][0]), "+v"(t[0][1]), "+v"(t[0][2]), "+v"(t[0][3]) : : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(t[0][0]), "+v"(t[0][1]), "+v"(t[0][2]), "+v"(t[0][3]), "+v"(t[1][0]), "+v"(t[1][1]), "+v"(t[1][2]), "+v"(t[1][3])
                     :
                     : "memory");
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[cb][jj] = t[cb][jj];
    __syncthreads();
}

template <int NCH, int COUT>
__global__ __launch_bounds__(256, 2) void srf_spconv_gsp_k(const float *__restrict__ in, int A_in, const float *__restrict__ Wg, int K,
                                                         const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                         const float *__restrict__ alpha, const float *__restrict__ beta,
                                                         const float *__restrict__ residual, int relu,
                                                         float *__restrict__ out, const int *__restrict__ rows_dev,
                                                         const int *__restrict__ tiles)
{
    constexpr int NT = COUT / 64, NB = COUT / 32;
    constexpr int RS = 16;   // rows per step (srf_gsp_step)
    constexpr int NA = NCH >= 2 ? NCH / 2 : 1, TPR = NCH >= 2 ? 16 : 8, NKW = (SRF_KMAX + 3) / 4, CHS = RS * 32 + 8;
    constexpr int TMAX = COUT == 128 ? SRF_GS_TMAX : 128, OS = COUT + 4;   // (64 channels: 128 rows = the two ballot segments; 63 KB of LDS)
    constexpr int FL = ((TMAX * SRF_KMAX + SRF_KMAX * (RS - 1) + RS - 1) / RS) * RS + 2 * RS;   // every offset padded to whole steps, two dummy steps
    static_assert(COUT == 128 || COUT == 64, "column tiling of the waves");
    static_assert(TMAX <= 128 && TMAX < 255, "two ballot segments of 64 rows; slots are bytes");
    static_assert(NCH == 1 || (NCH & 1) == 0, "a gathered row is one quad (32 channels) or NCH / 2 quads per thread");
    __shared__ unsigned s_pin[FL];                          // flat step list: byte offset of the input row (padding: out of range)
    __shared__ __attribute__((aligned(4))) unsigned char s_pslot[FL];  // ... and the row's slot in the output tile
    __shared__ int s_cnt[SRF_KMAX];
    __shared__ int s_gstart[SRF_KMAX + 1];                  // first step of an offset; [KMAX] = steps of the sub-tile
    __shared__ int s_klist[SRF_KMAX + 2];                   // used offsets ascending; [KMAX] their count, [KMAX + 1] their bit mask
    __shared__ unsigned char s_sinfo[FL / RS + 4];          // per step: bit 0 = last step of its offset, bits 1.. = the next used offset
    __shared__ __attribute__((aligned(16))) float s_out[(TMAX + 1) * OS];
    __shared__ __attribute__((aligned(16))) float s_a[2 * NCH * CHS];

    const int A_cap = A_out;
    A_out = srf_live_rows(A_out, rows_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int range0, range1;
    if (tiles) {
        const int T = srf_gs_ranges(A_cap);
        if ((int)blockIdx.x >= T) return;
        const int t = srf_xcd_tile(blockIdx.x, T);
        range0 = tiles[t];
        range1 = tiles[t + 1];
        range1 = range1 < A_out ? range1 : A_out;
    } else {
        const int tm = srf_gs_tile_rows(A_out);
        const int n_tiles = (A_out + tm - 1) / tm;
        if ((int)blockIdx.x >= n_tiles) return;
        range0 = srf_xcd_tile(blockIdx.x, n_tiles) * tm;
        range1 = range0 + tm < A_out ? range0 + tm : A_out;
    }
    if (range1 <= range0) return;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)((long long)A_in * (32 * NCH) * 4), 0x00020000);
    const int nsub = (range1 - range0 + TMAX - 1) / TMAX;
    const int TM = (((range1 - range0 + nsub - 1) / nsub) + 7) & ~7;
    for (int row0 = range0; row0 < range1; row0 += TM) {
    const int row_end = row0 + TM < range1 ? row0 + TM : range1;
    // An opaque zero: the address arithmetic of the prologue / epilogue is invariant across sub-tiles, and hoisted above this loop
    // it would stay live through the main loop, where every register is taken, and be spilled.  Tied to this value it is recomputed
    // per sub-tile instead.
    int zero = 0;
    asm volatile("" : "+s"(zero));
    for (int e = tid; e < TM * OS / 4; e += 256) reinterpret_cast<f32x4 *>(s_out)[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    int nv[NKW][2];
#pragma unroll
    for (int i = 0; i < NKW; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = wave + 4 * i, r = h * 64 + lane;
            nv[i][h] = (k < K && row0 + r < row_end) ? nbr[(size_t)(k + zero) * nbr_stride + row0 + r] : -1;
        }
    // pass 1: pairs per offset
#pragma unroll
    for (int i = 0; i < NKW; ++i) {
        const int k = wave + 4 * i;
        if (k >= SRF_KMAX) break;
        const int c = __popcll(__ballot(nv[i][0] >= 0)) + __popcll(__ballot(nv[i][1] >= 0));
        if (lane == 0) s_cnt[k] = c;
    }
    __syncthreads();
    if (tid < 64) {   // first step of every offset (exclusive prefix of the group counts), the used offsets in ascending order
        const int c = tid < SRF_KMAX ? s_cnt[tid] : 0;
        const int ng = (c + RS - 1) / RS;
        int x = ng;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (tid < SRF_KMAX) s_gstart[tid] = x - ng;
        if (tid == SRF_KMAX - 1) s_gstart[SRF_KMAX] = x;
        const unsigned long long m = __ballot(c > 0);
        if (c > 0) s_klist[__popcll(m & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) {
            s_klist[SRF_KMAX] = __popcll(m);
            s_klist[SRF_KMAX + 1] = (int)(unsigned)m;
        }
    }
    __syncthreads();
    const int S = __builtin_amdgcn_readfirstlane(s_gstart[SRF_KMAX]);
    const unsigned used = (unsigned)s_klist[SRF_KMAX + 1];
    // pass 2: compaction into the flat list
#pragma unroll
    for (int i = 0; i < NKW; ++i) {
        const int k = wave + 4 * i;
        if (k >= SRF_KMAX) break;
        const int g0 = s_gstart[k + zero] * RS;
        int base = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int v = nv[i][h];
            const unsigned long long m = __ballot(v >= 0);
            if (v >= 0) {
                const int pos = g0 + base + __popcll(m & ((1ull << lane) - 1ull));
                s_pin[pos] = (unsigned)v * (unsigned)(32 * NCH * 4);
                s_pslot[pos] = (unsigned char)(h * 64 + lane);
            }
            base += __popcll(m);
        }
        const int ng = (base + RS - 1) / RS;
        const int pad = ng * RS - base;   // padding of the offset's last step (< RS <= 32 entries): zeros into the spare row
        if (lane < pad) {
            s_pin[g0 + base + lane] = 0x80000000u;
            s_pslot[g0 + base + lane] = (unsigned char)TMAX;
        }
        if (lane < ng) {
            const unsigned later = k + 1 < 32 ? (used >> (k + 1)) : 0u;
            const int kn = later ? k + 1 + __builtin_ctz(later) : k;   // the next used offset (the last one names itself)
            s_sinfo[g0 / RS + lane] = (unsigned char)(lane == ng - 1 ? ((kn << 1) | 1) : 0);
        }
    }
    if (tid < 2 * RS) {   // two dummy steps behind the last one
        s_pin[S * RS + tid] = 0x80000000u;
        s_pslot[S * RS + tid] = (unsigned char)TMAX;
    }
    __syncthreads();
    const int ntap = __builtin_amdgcn_readfirstlane(s_klist[SRF_KMAX]);

    // per-thread constants of a step
    SrfGspLane L;
    {
        const int ar = lane & 15, aj = lane >> 4, a_swz = (ar >> 1) & 7;
        const unsigned a0 = srf_lds_addr(s_a) + (unsigned)zero;
        L.fo0 = a0 + (unsigned)(ar * 32 + (((aj << 1) ^ a_swz) << 2)) * 4u;
        L.fo1 = a0 + (unsigned)(ar * 32 + ((((aj << 1) + 1) ^ a_swz) << 2)) * 4u;
        L.colbase = srf_lds_addr(s_out) + (unsigned)((COUT == 128 ? wave * 32 : wave * 16) + ar + zero) * 4u;
        // gather: thread = (row tid / 16, quad tid % 16 of the row, and for Cin = 128 the quad 16 further = two chunks further)
        const int r = (tid / TPR) & 15, qq = tid % TPR, ch = qq >> 3, q = qq & 7, swz = (r >> 1) & 7;
        L.goff = (unsigned)(qq * 16 + zero);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) L.sto[jj] = a0 + (unsigned)(ch * CHS + r * 32 + (q & 3) + (((jj * 2 + (q >> 2)) ^ swz) << 2)) * 4u;
        const int wc = COUT == 128 ? wave : (wave >> 1), g0 = COUT == 128 ? 0 : 2 * (wave & 1);
        L.boff = (unsigned)(lane * 16 + wc * 4096 + g0 * 1024 + zero);
    }
    __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wg), 0, K * NCH * NB * 4096, 0x00020000);
    f32x4 b0[NCH][NB], b1[NCH][NB], ra[NA], acc[NT];
    SrfGspRegs G;
    int buf = 0;
    {
        constexpr unsigned ABUF = NCH * CHS * 4;
        const int aj = lane >> 4;
        G.f0 = L.fo0;
        G.f1 = L.fo1;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) G.st[jj] = L.sto[jj] + ABUF;
        const unsigned sl0 = *reinterpret_cast<const unsigned *>(s_pslot + aj * 4);   // slots of step 0
        G.gaddr = s_pin[2 * RS + ((tid / TPR) & 15)] + L.goff;                        // step 0 requests the rows of step 2
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            G.oaddr[jj] = ((sl0 >> (8 * jj)) & 255u) * (unsigned)(OS * 4) + L.colbase;
#pragma unroll
            for (int cb = 0; cb < NT; ++cb) acc[cb][jj] = 0.0f;   // the tile was just zeroed
        }
        G.pin_addr = srf_lds_addr(s_pin) + (unsigned)(3 * RS + ((tid / TPR) & 15)) * 4u;   // ... and reads the list entries of step 3
        G.slot_addr = srf_lds_addr(s_pslot) + (unsigned)(RS + aj * 4);                  // ... and the slots of step 1
        G.info_addr = srf_lds_addr(s_sinfo) + 1u + (unsigned)zero;                      // ... and its offset flag
    }
    if (ntap > 0) {
        const int k0 = s_klist[0];
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int g = 0; g < NB; ++g) {
                auto v = __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)(L.boff + g * 1024), (k0 * NCH + c) * (NB * 4096), 0);
                b0[c][g] = *reinterpret_cast<f32x4 *>(&v);
            }
        const unsigned ro0 = s_pin[(tid / TPR) & 15];
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(ro0 + L.goff + j * 256), 0, 0);
            ra[j] = *reinterpret_cast<f32x4 *>(&v);
        }
        if (TPR == 16 || tid < 16 * TPR) {
#pragma unroll
            for (int j = 0; j < NA; ++j)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) *reinterpret_cast<srf_lds_float *>(L.sto[jj] + j * (2 * CHS * 4)) = ra[j][jj];
        }
        const unsigned ro1 = s_pin[RS + ((tid / TPR) & 15)];
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(ro1 + L.goff + j * 256), 0, 0);
            ra[j] = *reinterpret_cast<f32x4 *>(&v);
        }
    }
    __syncthreads();
    // ONE flat loop over the steps: whether a step ends its offset (and which offset follows) is a byte of the step list, read in the
    // step's LDS section and turned into a scalar inside its MFMA block -- no vector instruction outside the MFMA blocks (a lookup
    // of the offset tables between two offsets used to cost three dependent LDS reads and their readfirstlanes, stalled like every
    // vector instruction while the partner workgroup multiplies)
    int info = S > 0 ? __builtin_amdgcn_readfirstlane((int)s_sinfo[0]) : 0;
    for (int i = 0; i < S;) {   // two offsets per trip: the B register sets swap roles without moves
        int info_next = 0;
        for (; !(info & 1); ++i) {
            srf_gsp_step<NCH, COUT, false>(rs, wrs, 0, buf, L, G, b0, b1, ra, acc, info_next);
            info = info_next;
        }
        srf_gsp_step<NCH, COUT, true>(rs, wrs, info >> 1, buf, L, G, b0, b1, ra, acc, info_next);
        info = info_next;
        if (++i >= S) break;
        for (; !(info & 1); ++i) {
            srf_gsp_step<NCH, COUT, false>(rs, wrs, 0, buf, L, G, b1, b0, ra, acc, info_next);
            info = info_next;
        }
        srf_gsp_step<NCH, COUT, true>(rs, wrs, info >> 1, buf, L, G, b1, b0, ra, acc, info_next);
        info = info_next;
        ++i;
    }
    // the last step's write-back went through raw LDS addresses: make the whole tile visible to the epilogue's plain reads
    __syncthreads();

    // epilogue: every output row once, BN / residual / ReLU in registers, 512 B per row and store
    constexpr int CQ = COUT / 4;
    const int c4 = ((tid & (CQ - 1)) + zero) * 4;
    f32x4 al = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
    if (alpha) {
        al = *reinterpret_cast<const f32x4 *>(alpha + c4);
        be = *reinterpret_cast<const f32x4 *>(beta + c4);
    }
    for (int r = tid / CQ; r < TM; r += 256 / CQ) {
        const int row = row0 + r;
        if (row >= row_end) break;
        f32x4 v = *reinterpret_cast<const f32x4 *>(s_out + r * OS + c4);
        f32x4 rsd = {0.f, 0.f, 0.f, 0.f};
        if (residual) rsd = *reinterpret_cast<const f32x4 *>(residual + (size_t)row * COUT + c4);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = srf_spconv_epilogue(v[j], alpha, al[j], be[j], residual, [&] { return rsd[j]; }, relu);
        *reinterpret_cast<f32x4 *>(out + (size_t)row * COUT + c4) = v;
    }
    __syncthreads();
    }
}

// =====================================================================================================================
// srf_spconv_w32_k: the 32-output-channel layers (SubM 32 -> 32 x 4 and the strided 16 -> 32 of the nuScenes encoder,
// sparse_encoder_custom.py:109-140 through spconv's SubMConv3d / SparseConv3d).  A tile kernel that walks the 27 offsets as
// gather -> LDS -> barrier -> 16 MFMAs runs at the latency of a gather per step whatever the arithmetic.  Here nothing is
// shared but the weights:
//   * a workgroup = 8 waves x 32 output rows; all 27 x Cin x 32 weights sit in LDS (110 KB at Cin = 32), copied once;
//   * every wave gathers ITS 32 rows straight into the MFMA's A layout -- lane (row, half) loads half of the neighbour's
//     channels with Cin / 8 buffer_load_dwordx4 (a missing neighbour is an out-of-range offset and reads as zero), then
//     v_permlane32_swap hands the odd channels to lanes 32-63 and the even ones to lanes 0-31 (the f32 32x32x2 MFMA takes
//     channel 2 s from lanes 0-31 and 2 s + 1 from lanes 32-63) -- three offsets in flight, no barrier, no LDS round trip;
//   * offsets none of the wave's rows has are skipped (one ballot per offset).
// Every output is the chain (offset ascending, channel ascending, zero terms added as +0) of oracle/srf_oracle.c:orc_spconv_fwd:
// bit-identical to srf_spconv_fwd and the oracle.
// =====================================================================================================================
// ---------------------------------------------------------------------------------------------------------------------
// Row order for the 32-channel layers (srf_spconv_w32_k): a wave multiplies EVERY offset that any of its 32 rows has -- 0.77 of the
// 27 offsets on the level-2 rulebook of a nuScenes sweep, 0.54 on the strided 16 -> 32 one, where 0.28 / 0.05 exist.  Rows with the same
// set of offsets put side by side share their zeros: sorted by an 11-bit key of the offset mask (has any z - 1 neighbour, has any z + 1
// neighbour, the nine offsets of the row's own z plane) inside windows of 1024 rows a 32-row group executes 0.47 / 0.28 of the
// offsets.  One launch per rulebook (shared by the SubM layers of a level): a workgroup counting-sorts its window in LDS and writes
//   plan[0 .. A_pad)                      order[pos] = row at sorted position pos (-1: padding)
//   plan[A_pad + k A_pad + pos]           the rulebook entry nbr[k][order[pos]] (-1: none)
// Which rows share a wave changes nothing in any output (every row is its own fma chain): bit-identical.
// ---------------------------------------------------------------------------------------------------------------------
#define SRF_ORD_WIN 1024
#define SRF_ORD_BINS 2048
__host__ __device__ static inline int srf_ord_pad(int A) { return ((A + SRF_ORD_WIN - 1) / SRF_ORD_WIN) * SRF_ORD_WIN; }

__global__ __launch_bounds__(256) void srf_spconv_order_k(const int *__restrict__ nbr, int nbr_stride, int K, int A, int A_pad,
                                                         const int *__restrict__ rows_dev, int *__restrict__ plan)
{
    __shared__ int s_hist[SRF_ORD_BINS];
    __shared__ int s_part[256];
    __shared__ int s_row[SRF_ORD_WIN];
    A = srf_live_rows(A, rows_dev);
    const int tid = threadIdx.x, w0 = blockIdx.x * SRF_ORD_WIN;
    for (int b = tid; b < SRF_ORD_BINS; b += 256) s_hist[b] = 0;
    __syncthreads();
    int key[4], rank[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = w0 + i * 256 + tid;
        const int rc = row < A ? row : (A > 0 ? A - 1 : 0);
        unsigned m = 0;
        int v[SRF_KMAX];
#pragma unroll
        for (int k = 0; k < SRF_KMAX; ++k) v[k] = nbr[(size_t)(k < K ? k : K - 1) * nbr_stride + rc];
#pragma unroll
        for (int k = 0; k < SRF_KMAX; ++k) m |= (k < K && v[k] >= 0 ? 1u : 0u) << k;
        const unsigned p0 = m & 0x1ffu, p1 = (m >> 9) & 0x1ffu, p2 = (m >> 18) & 0x1ffu;
        unsigned kk = K == SRF_KMAX ? ((((p0 != 0 ? 1u : 0u) | (p2 != 0 ? 2u : 0u)) << 9) | p1) : (m & (SRF_ORD_BINS - 1));
        key[i] = row < A ? (int)kk : SRF_ORD_BINS - 1;   // rows past the end sort last (their order entry becomes -1)
        rank[i] = atomicAdd(&s_hist[key[i]], 1);
    }
    __syncthreads();
    // exclusive prefix of the 2048 bins: 8 consecutive bins per thread, then the 256 partial sums
    int loc[8], sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        loc[j] = sum;
        sum += s_hist[tid * 8 + j];
    }
    s_part[tid] = sum;
    __syncthreads();
    int base = 0;
    for (int t = 0; t < tid; ++t) base += s_part[t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) s_hist[tid * 8 + j] = base + loc[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) s_row[s_hist[key[i]] + rank[i]] = i * 256 + tid;   // (ranks inside a bin: arrival order, any order is right)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = i * 256 + tid, pos = w0 + p;
        if (pos >= A_pad) continue;
        const int row = w0 + s_row[p];
        const bool live = row < A;
        plan[pos] = live ? row : -1;
        const int rc = live ? row : (A > 0 ? A - 1 : 0);
        int v[SRF_KMAX];
#pragma unroll
        for (int k = 0; k < SRF_KMAX; ++k) v[k] = nbr[(size_t)(k < K ? k : K - 1) * nbr_stride + rc];
#pragma unroll
        for (int k = 0; k < SRF_KMAX; ++k)
            if (k < K) plan[(size_t)A_pad + (size_t)k * A_pad + pos] = live ? v[k] : -1;
    }
}

extern "C" size_t srf_spconv_order_ints(int A_out, int K)
{
    if (A_out <= 0 || K <= 0 || K > SRF_KMAX) return 0;
    return (size_t)srf_ord_pad(A_out) * (size_t)(1 + K);
}

extern "C" int srf_spconv_order_build(const int *nbr, int nbr_stride, int K, int A_out, const int *rows_dev, int *plan, srf_stream_t stream)
{
    if (A_out < 0 || K <= 0 || K > SRF_KMAX || nbr_stride < A_out) return SRF_EINVAL;
    if (A_out == 0) return SRF_OK;
    if (!nbr || !plan) return SRF_EINVAL;
    const int A_pad = srf_ord_pad(A_out);
    hipLaunchKernelGGL(srf_spconv_order_k, dim3(A_pad / SRF_ORD_WIN), dim3(256), 0, (hipStream_t)stream, nbr, nbr_stride, K, A_out, A_pad,
                       rows_dev, plan);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

#ifndef SRF_W32_DEPTH
#define SRF_W32_DEPTH 6
#endif
template <int CIN>
__global__ __launch_bounds__(512) void srf_spconv_w32_k(const float *__restrict__ in, int A_in, const float *__restrict__ Wp,
                                                       const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                       const float *__restrict__ alpha, const float *__restrict__ beta,
                                                       const float *__restrict__ residual, int relu, float *__restrict__ out,
                                                       const int *__restrict__ rows_dev, const int *__restrict__ plan)
{
    constexpr int K = SRF_KMAX, H = CIN / 2, NV = H / 4, NB = CIN / 8, TM = 256;
    extern __shared__ __attribute__((aligned(16))) f32x4 s_w32[];   // [K][NB][2][32]
    const int A_cap = A_out;
    A_out = srf_live_rows(A_out, rows_dev);
    const int n_tiles = plan ? ((A_out + SRF_ORD_WIN - 1) / SRF_ORD_WIN) * 4 : (A_out + TM - 1) / TM;
    if ((int)blockIdx.x >= n_tiles) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, kh = lane >> 5;
    // with a plan (srf_spconv_order_build) the wave's 32 rows are a group of the sorted order: `row` is a POSITION, the rulebook
    // entries come from the plan's sorted copy, the output row is order[position].  The 32 groups of a 1024-row window go to its
    // four workgroups in turn (group 4 w + b to wave w of workgroup b): every workgroup, and every pair of waves that shares a SIMD,
    // gets light and heavy groups alike.
    int row0 = 0, row;
    if (plan) {
        const int A_pad = srf_ord_pad(A_cap);
        const int win = blockIdx.x >> 2, b = blockIdx.x & 3;
        row = win * SRF_ORD_WIN + (4 * wave + b) * 32 + r;
        nbr = plan + A_pad;
        nbr_stride = A_pad;
    } else {
        row0 = srf_xcd_tile(blockIdx.x, n_tiles) * TM;
        row = row0 + wave * 32 + r;
    }
    const f32x4 *Wp4 = reinterpret_cast<const f32x4 *>(Wp);
    for (int i = tid; i < K * NB * 64; i += 512) s_w32[i] = Wp4[i];
    // all K rulebook entries of the row in flight at once (a load under `row < A_out` is a load under a branch: hipcc then waits for
    // each one before the next -- 27 round trips in a row): rows past the end read the last row's entries and drop them
    int idx[K];
    unsigned anym = 0;
    const int row_ld = (plan || row < A_out) ? row : A_out - 1;     // (every position of a plan exists: padding holds -1)
    const bool row_ok = plan || row < A_out;
    const int ord = plan ? plan[row] : row;                          // the output row behind this lane's row / position (-1: none)
#pragma unroll
    for (int k = 0; k < K; ++k) idx[k] = nbr[(size_t)k * nbr_stride + row_ld];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        idx[k] = row_ok ? idx[k] : -1;
        anym |= (__ballot(idx[k] >= 0) != 0ull ? 1u : 0u) << k;
    }
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)((long long)A_in * CIN * 4), 0x00020000);
    // D offsets in flight.  The loads are NOT under the `anym` test: a load inside a scalar branch makes hipcc's wait-count pass
    // give up counting (it emitted s_waitcnt vmcnt(0) in front of every offset's MFMAs, 109 of them: the "three offsets in flight"
    // of round 3 were drained at every step and each offset paid a full gather latency, 1.4 us against 0.43 us of MFMAs).  An
    // offset no row of the wave has is 64 out-of-range lanes: the descriptor returns zeros without touching memory.
    constexpr int D = SRF_W32_DEPTH;
    f32x4 a[D][NV];
#define W32_LOAD(SET, KK)                                                                                    \
    {                                                                                                        \
        const unsigned vo_ = idx[KK] >= 0 ? (unsigned)(idx[KK] * (CIN * 4) + kh * (H * 4)) : 0x80000000u;    \
        _Pragma("unroll") for (int j_ = 0; j_ < NV; ++j_) {                                                  \
            auto v_ = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(vo_ + j_ * 16), 0, 0);                      \
            a[SET][j_] = *reinterpret_cast<f32x4 *>(&v_);                                                    \
        }                                                                                                    \
    }
#pragma unroll
    for (int k = 0; k < D - 1; ++k) W32_LOAD(k, k)
    __syncthreads();   // the weights are in LDS
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k + D - 1 < K) W32_LOAD((k + D - 1) % D, k + D - 1)
        if (anym & (1u << k)) {
            f32x4 b[NB];
#pragma unroll
            for (int sg = 0; sg < NB; ++sg) b[sg] = s_w32[((k * NB + sg) * 2 + kh) * 32 + r];
            // lanes 0-31 hold the first half of the row's channels, lanes 32-63 the second: swap so that lanes 0-31 end up with
            // the even channels (first half in x / z, second half in y / w), lanes 32-63 with the odd ones
            float e0[NV], e1[NV], o0[NV], o1[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f32x4 v = a[k % D][j];
                auto p0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[0]), __float_as_uint(v[1]), false, false);
                auto p1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2]), __float_as_uint(v[3]), false, false);
                e0[j] = __uint_as_float(p0[0]);   // channel 4 j + kh
                o0[j] = __uint_as_float(p0[1]);   // channel H + 4 j + kh
                e1[j] = __uint_as_float(p1[0]);   // channel 4 j + 2 + kh
                o1[j] = __uint_as_float(p1[1]);   // channel H + 4 j + 2 + kh
            }
            // steps in channel order: s = 2 j (channels 4 j, 4 j + 1), 2 j + 1; then the second half from step H / 2 on
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(e0[j], b[(2 * j) >> 2][(2 * j) & 3], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(e1[j], b[(2 * j + 1) >> 2][(2 * j + 1) & 3], acc, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(o0[j], b[(H / 2 + 2 * j) >> 2][(H / 2 + 2 * j) & 3], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(o1[j], b[(H / 2 + 2 * j + 1) >> 2][(H / 2 + 2 * j + 1) & 3], acc, 0, 0, 0);
            }
        }
    }
#undef W32_LOAD
    const float al = alpha ? alpha[r] : 1.0f;
    const float be = alpha ? beta[r] : 0.0f;
    // the 16 residual values in flight together (one load per row under its own `orow < A_out` branch was 16 round trips in a row)
    int orow[16];   // accumulator register j holds row (j & 3) + 8 (j >> 2) + 4 kh of the wave's 32: its output row is lane that-index's `ord`
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int o = __shfl(ord, (j & 3) + 8 * (j >> 2) + 4 * kh);
        orow[j] = (o >= 0 && o < A_out) ? o : -1;
    }
    float res[16];
    if (residual) {
#pragma unroll
        for (int j = 0; j < 16; ++j) res[j] = residual[(size_t)(orow[j] >= 0 ? orow[j] : 0) * 32 + r];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float v = srf_spconv_epilogue(acc[j], alpha, al, be, residual, [&] { return res[j]; }, relu);
        if (orow[j] >= 0) out[(size_t)orow[j] * 32 + r] = v;
    }
}

extern "C" int srf_spconv_fwd_packed(const float *in, int A_in, int Cin, const float *W_packed, int K, const int *nbr,
                                     int nbr_stride, int A_out, int Cout, const float *alpha, const float *beta,
                                     const float *residual, int relu, float *out, const int *rows_dev, const int *tiles,
                                     srf_stream_t stream)
{
    const SrfPackedLayout layout = srf_spconv_shape(K, Cin, Cout).packed;
    // both kernels gather through a buffer descriptor (range32)
    const int rc = srf_spconv_check({layout != SRF_PACKED_NONE, false, true}, in, A_in, Cin, W_packed, K, nbr, nbr_stride, A_out, Cout, alpha,
                                    beta, out);
    if (rc != SRF_OK || A_out == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (layout == SRF_PACKED_W32) {
        static bool lds_set[64] = {false};
        SRF_LDS_OPT_IN(lds_set, {srf_spconv_w32_k<32>, SRF_KMAX * 32 * 32 * 4}, {srf_spconv_w32_k<16>, SRF_KMAX * 16 * 32 * 4});
        // `tiles` of a 32-channel layer = the plan of srf_spconv_order_build (NULL: rows in their own order)
        const unsigned grid32 = tiles ? (unsigned)(srf_ord_pad(A_out) / 256) : (unsigned)srf_ceil_div(A_out, 256);
        if (Cin == 32)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_w32_k<32>), dim3(grid32), dim3(512), SRF_KMAX * 32 * 32 * 4, st, in,
                               A_in, W_packed, nbr, nbr_stride, A_out, alpha, beta, residual, relu, out, rows_dev, tiles);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_w32_k<16>), dim3(grid32), dim3(512), SRF_KMAX * 16 * 32 * 4, st, in,
                               A_in, W_packed, nbr, nbr_stride, A_out, alpha, beta, residual, relu, out, rows_dev, tiles);
        SRF_LAUNCH_CHECK();
        return SRF_OK;
    }
    // SRF_PACKED_GS.  Grid: >= the tiles of any live row count <= A_out / the ranges srf_spconv_tiles_build cut for this capacity
    const dim3 grid(tiles ? srf_gs_ranges(A_out) : SRF_GS_SLOTS * srf_gs_rounds(A_out));
#define GSP_LAUNCH(NCH, COUT) hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_gsp_k<NCH, COUT>), grid, dim3(256), 0, st, in, A_in, W_packed, K, \
                                                 nbr, nbr_stride, A_out, alpha, beta, residual, relu, out, rows_dev, tiles)
    if (Cout == 64) {
        if (Cin == 32) GSP_LAUNCH(1, 64);
        else GSP_LAUNCH(2, 64);
    } else {
        if (Cin == 128) GSP_LAUNCH(4, 128);
        else GSP_LAUNCH(2, 128);
    }
#undef GSP_LAUNCH
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// COUT = 16: four waves, each 16 rows x 16 cols on v_mfma_f32_16x16x4_f32
template <int TM>
__global__ __launch_bounds__(256) void srf_spconv_mfma16_k(const float *__restrict__ in, int Cin,
                                                         const float *__restrict__ W, int K,
                                                         const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                         const float *__restrict__ alpha, const float *__restrict__ beta,
                                                         const float *__restrict__ residual, int relu,
                                                         float *__restrict__ out, const int *__restrict__ rows_dev)
{
    constexpr int COUT = 16;
    static_assert(TM == 64, "four 16-row wave tiles");
    __shared__ int s_nbr[SRF_KMAX * TM];
    __shared__ int s_any[SRF_KMAX];
    __shared__ float s_a[TM][SRF_KC + 1];
    __shared__ __attribute__((aligned(16))) float s_w[SRF_KC][COUT];

    A_out = srf_live_rows(A_out, rows_dev);
    const int row0 = blockIdx.x * TM;
    if (row0 >= A_out) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    srf_load_nbr_tile<TM>(nbr, nbr_stride, K, row0, A_out, s_nbr, s_any);

    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const int ar = wave * 16 + (lane & 15);
    const int kq = lane >> 4;
    for (int k = 0; k < K; ++k) {
        if (!s_any[k]) continue;
        const float *Wk = W + (size_t)k * Cin * COUT;
        for (int c0 = 0; c0 < Cin; c0 += SRF_KC) {
            __syncthreads();
            srf_stage_tile<TM, COUT>(in, Cin, Wk, c0, s_nbr + k * TM, s_a, s_w);
            __syncthreads();
            const int kc = (Cin - c0) < SRF_KC ? (Cin - c0) : SRF_KC;
            for (int kk = 0; kk < kc; kk += 4) {
                const float a = s_a[ar][kk + kq];
                const float b = s_w[kk + kq][lane & 15];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            }
        }
    }
    // C/D layout of 16x16: col = lane & 15, row = (lane >> 4) * 4 + j
    const int col = lane & 15;
    const float al = alpha ? alpha[col] : 1.0f;
    const float be = alpha ? beta[col] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = row0 + wave * 16 + kq * 4 + j;
        if (row < A_out)
            out[(size_t)row * COUT + col] = srf_spconv_epilogue(acc[j], alpha, al, be, residual, [&] { return residual[(size_t)row * COUT + col]; }, relu);
    }
}

// COUT = 16, Cin <= 16 (the 41 x 1472 x 1472 level: conv_input and the first two basic blocks).  These layers are bound by
// the gathers, not by arithmetic (27 x 64 B per output row out of L2), so the kernel has no LDS and no barriers at all:
// a wave owns 16 output rows; its B operands -- all K x Cin x 16 weights, STEPS*K registers per lane -- are loaded once
// and stay in registers; the neighbour indices of all offsets are fetched up front, and the gathered A operands go
// global -> registers in MFMA order (v_mfma_f32_16x16x4_f32: lane (row, q) supplies channel 4j + q of step j), nine
// offsets in flight at a time.  Accumulation order as everywhere: offset ascending, channel ascending.
template <int STEPS>  // ceil(Cin / 4)
__global__ __launch_bounds__(256) void srf_spconv_c16_k(const float *__restrict__ in, int Cin, const float *__restrict__ W, int K,
                                                      const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                      const float *__restrict__ alpha, const float *__restrict__ beta,
                                                      const float *__restrict__ residual, int relu, float *__restrict__ out,
                                                      const int *__restrict__ rows_dev)
{
    constexpr int COUT = 16, KM = SRF_KMAX, G = 9;
    A_out = srf_live_rows(A_out, rows_dev);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * 16;
    if (row0 >= A_out) return;  // no barriers in this kernel: waves are independent
    const int r = lane & 15, q = lane >> 4;
    const int row = row0 + r;
    // weights: lane (col = r, q) holds W[k][4j + q][col]
    float wreg[KM][STEPS];
#pragma unroll
    for (int k = 0; k < KM; ++k)
#pragma unroll
        for (int j = 0; j < STEPS; ++j) {
            const int c = 4 * j + q;
            wreg[k][j] = (k < K && c < Cin) ? W[((size_t)k * Cin + c) * COUT + r] : 0.f;
        }
    int idx[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) idx[k] = (k < K && row < A_out) ? nbr[(size_t)k * nbr_stride + row] : -1;

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float a[2][G][STEPS];
#pragma unroll
    for (int t = 0; t < G; ++t)
#pragma unroll
        for (int j = 0; j < STEPS; ++j) {
            const int c = 4 * j + q;
            a[0][t][j] = (idx[t] >= 0 && c < Cin) ? in[(size_t)idx[t] * Cin + c] : 0.f;  // predicated: 9 of 10 neighbours are absent here
        }
#pragma unroll
    for (int g0 = 0; g0 < KM; g0 += G) {
        const int cur = (g0 / G) & 1;
        if (g0 + G < KM) {
#pragma unroll
            for (int t = 0; t < G; ++t)
#pragma unroll
                for (int j = 0; j < STEPS; ++j) {
                    const int k = g0 + G + t, c = 4 * j + q;
                    a[cur ^ 1][t][j] = (idx[k] >= 0 && c < Cin) ? in[(size_t)idx[k] * Cin + c] : 0.f;
                }
        }
#pragma unroll
        for (int t = 0; t < G; ++t) {
            const int k = g0 + t;
#pragma unroll
            for (int j = 0; j < STEPS; ++j) {
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur][t][j], wreg[k][j], acc, 0, 0, 0);
            }
        }
    }
    // C/D layout of 16x16: col = lane & 15, row = (lane >> 4) * 4 + i
    const float al = alpha ? alpha[r] : 1.f, be = alpha ? beta[r] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int orow = row0 + q * 4 + i;
        if (orow < A_out)
            out[(size_t)orow * COUT + r] = srf_spconv_epilogue(acc[i], alpha, al, be, residual, [&] { return residual[(size_t)orow * COUT + r]; }, relu);
    }
}

// srf_spconv_c16l_k: the same 16-row waves with the weights in LDS instead of 108 registers per lane, and the gathers in nine batches
// of three offsets, three batches in flight (36 registers): ~100 registers per lane = five waves per SIMD instead of two.  The kernel
// is bound by the latency of its gathers (three dependent batches per wave, two waves per SIMD to hide them): at nuScenes size every wave
// of the level is resident at once either way (26k rows = 6 waves per CU), at Waymo size (138k rows = 34 waves per CU) the register form
// runs 4.3 rounds of 8 waves per CU.  Same chain per output (offset ascending, channel ascending): identical bits.
template <int STEPS>  // ceil(Cin / 4)
__global__ __launch_bounds__(256) void srf_spconv_c16l_k(const float *__restrict__ in, int Cin, const float *__restrict__ W, int K,
                                                       const int *__restrict__ nbr, int nbr_stride, int A_out,
                                                       const float *__restrict__ alpha, const float *__restrict__ beta,
                                                       const float *__restrict__ residual, int relu, float *__restrict__ out,
                                                       const int *__restrict__ rows_dev)
{
    constexpr int COUT = 16, KM = SRF_KMAX, G = 3, NBATCH = KM / G, D = 3;
    __shared__ float s_w[KM * STEPS * 64];   // [k][j][lane]: lane (col r, q) holds W[k][4 j + q][r]
    A_out = srf_live_rows(A_out, rows_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    for (int e = tid; e < KM * STEPS * 64; e += 256) {
        const int l = e & 63, kj = e >> 6, k = kj / STEPS, j = kj - k * STEPS;
        const int c = 4 * j + (l >> 4);
        s_w[e] = (k < K && c < Cin) ? W[((size_t)k * Cin + c) * COUT + (l & 15)] : 0.f;
    }
    __syncthreads();   // the only barrier: the waves are independent from here on
    const int row0 = (blockIdx.x * 4 + wave) * 16;
    if (row0 >= A_out) return;
    const int row = row0 + r;
    const int row_ld = row < A_out ? row : A_out - 1;
    int idx[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) idx[k] = nbr[(size_t)(k < K ? k : K - 1) * nbr_stride + row_ld];
#pragma unroll
    for (int k = 0; k < KM; ++k) idx[k] = (k < K && row < A_out) ? idx[k] : -1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float a[D][G][STEPS];
#define C16L_LOAD(SET, B)                                                                                              \
    _Pragma("unroll") for (int t_ = 0; t_ < G; ++t_)                                                                   \
        _Pragma("unroll") for (int j_ = 0; j_ < STEPS; ++j_) {                                                         \
            const int k_ = (B) * G + t_, c_ = 4 * j_ + q;                                                              \
            a[SET][t_][j_] = (idx[k_] >= 0 && c_ < Cin) ? in[(size_t)idx[k_] * Cin + c_] : 0.f;                        \
        }
    C16L_LOAD(0, 0)
    C16L_LOAD(1, 1)
#pragma unroll
    for (int b = 0; b < NBATCH; ++b) {
        if (b + 2 < NBATCH) { C16L_LOAD((b + 2) % D, b + 2) }
        float wv[G][STEPS];
#pragma unroll
        for (int t = 0; t < G; ++t)
#pragma unroll
            for (int j = 0; j < STEPS; ++j) wv[t][j] = s_w[((b * G + t) * STEPS + j) * 64 + lane];
#pragma unroll
        for (int t = 0; t < G; ++t)
#pragma unroll
            for (int j = 0; j < STEPS; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b % D][t][j], wv[t][j], acc, 0, 0, 0);
    }
#undef C16L_LOAD
    const float al = alpha ? alpha[r] : 1.f, be = alpha ? beta[r] : 0.f;
    float res[4] = {0.f, 0.f, 0.f, 0.f};
    if (residual) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int orow = row0 + q * 4 + i;
            res[i] = residual[(size_t)(orow < A_out ? orow : A_out - 1) * COUT + r];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int orow = row0 + q * 4 + i;
        const float v = srf_spconv_epilogue(acc[i], alpha, al, be, residual, [&] { return res[i]; }, relu);
        if (orow < A_out) out[(size_t)orow * COUT + r] = v;
    }
}

#ifndef SRF_C16L_MIN_ROWS
#define SRF_C16L_MIN_ROWS 60000   /* measured (MI355X): 26k rows 14.1 -> 14.7 us (every wave resident at once either way), 99k rows 47.9 -> 35.1 us */
#endif
extern "C" int srf_spconv_fwd(const float *in, int A_in, int Cin, const float *W, int K, const int *nbr, int nbr_stride,
                              int A_out, int Cout, const float *alpha, const float *beta, const float *residual,
                              int relu, float *out, const int *rows_dev, srf_stream_t stream)
{
    // the wide kernels gather whole float4s (quads); the output width is decided by the switch below
    const int rc = srf_spconv_check({true, true, false}, in, A_in, Cin, W, K, nbr, nbr_stride, A_out, Cout, alpha, beta, out);
    if (rc != SRF_OK || A_out == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
#define SRF_ARGS in, Cin, W, K, nbr, nbr_stride, A_out, alpha, beta, residual, relu, out, rows_dev
    switch (Cout) {
    case 16:
        if (Cin <= 16 && K == SRF_KMAX && A_in > 0) {  // register-resident weights, LDS-free gather
            // many rows (Waymo's first level): the LDS-weight form, five waves per SIMD; few rows: every wave is resident at once anyway
            const bool lds_w = A_out >= SRF_C16L_MIN_ROWS;
            if (Cin <= 8) {
                if (lds_w) hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_c16l_k<2>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0, st, SRF_ARGS);
                else hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_c16_k<2>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0, st, SRF_ARGS);
            } else {
                if (lds_w) hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_c16l_k<4>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0, st, SRF_ARGS);
                else hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_c16_k<4>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0, st, SRF_ARGS);
            }
        } else {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_mfma16_k<64>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0, st,
                               SRF_ARGS);
        }
        break;
    case 32:
        hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_mfma32_k<32, 128, 4, 1>), dim3(srf_ceil_div(A_out, 128)), dim3(256),
                           0, st, SRF_ARGS);
        break;
    case 64:
        hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_mfma32_k<64, 64, 2, 2>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0,
                           st, SRF_ARGS);
        break;
    case 128:
        hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_spconv_mfma32_k<128, 64, 2, 2>), dim3(srf_ceil_div(A_out, 64)), dim3(256), 0,
                           st, SRF_ARGS);
        break;
    default:
        return SRF_EUNSUPPORTED;
    }
#undef SRF_ARGS
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// K6 densify: (A, C) rows at (b, z, y, x) -> (B, C, D, H, W).  One thread per (row, channel): the read is coalesced,
// the write scatters one dword per channel plane.
// ---------------------------------------------------------------------------------------------------------------------
// 64 rows x 64 channels per workgroup through LDS: the features are read along the channels (coalesced), the dense
// (B, C, D, H, W) tensor is written with the ROW index fastest -- consecutive rows of the sorted active set are neighbours
// in x (and z), so a channel's 64 values land in a few cache lines instead of one line per value (3.1 M scattered 4-byte
// stores took 31 us for 12 MB).
__global__ __launch_bounds__(256) void srf_densify_k(const float *__restrict__ feats, const int4 *__restrict__ indices,
                                                   int A, int C, int D, int H, int W, float *__restrict__ out)
{
    __shared__ float s_f[64][65];
    __shared__ long long s_off[64];
    const int row0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tid = threadIdx.x;
    const size_t plane = (size_t)D * H * W;
    if (tid < 64) {
        const int a = row0 + tid;
        long long off = -1;
        if (a < A) {
            const int4 p = indices[a];
            if (p.x >= 0) off = (long long)((size_t)p.x * C * plane + ((size_t)p.y * H + p.z) * W + p.w);  // padding rows: b < 0
        }
        s_off[tid] = off;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + i * 256, r = e >> 6, c = e & 63;
        const int a = row0 + r;
        s_f[r][c] = (a < A && c0 + c < C) ? feats[(size_t)a * C + c0 + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + i * 256, c = e >> 6, r = e & 63;
        const long long off = s_off[r];
        if (off >= 0 && c0 + c < C) out[(size_t)off + (size_t)(c0 + c) * plane] = s_f[r][c];
    }
}

extern "C" int srf_densify(const float *feats, const int *indices, int A, int C, int B, int D, int H, int W, float *out,
                           int zero_fill, srf_stream_t stream)
{
    if (A < 0 || C <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0 || !out) return SRF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (zero_fill) SRF_HIP_TRY(srf_fill_bytes(out, 0, sizeof(float) * (size_t)B * C * D * H * W, st));
    if (A == 0) return SRF_OK;
    if (!feats || !indices) return SRF_EINVAL;
    hipLaunchKernelGGL(srf_densify_k, dim3(srf_ceil_div(A, 64), srf_ceil_div(C, 64)), dim3(256), 0, st, feats,
                       (const int4 *)indices, A, C, D, H, W, out);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
