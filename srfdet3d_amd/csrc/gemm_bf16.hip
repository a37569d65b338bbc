// gemm_bf16.hip -- srf_conv1x1_nhwc_bf16* / srf_conv_gemm_nhwc_bf16: the GEMM-shaped layers of the camera branch (VoVNet's 3x3 and
// `concat` layers, stem_3, the image FPN) with f32 tensors and ONE bf16 product per f32 product -- the opt-in reduced-precision mode
// of the image branch (`SRFDet.img_mfma_dtype`, nhwc.mfma_dtype), where gemm_split.hip spends six products to stay f32-accurate.
//
// Definition (tests/bf16_ref.py is this paragraph in numpy; tests/test_gpu_gemm_bf16.py holds the kernel to it).  Activations stay f32
// in HBM.  Each activation and each weight is rounded to bf16 ONCE, round to nearest even (v_cvt_pk_bf16_f32 =
// torch.Tensor.bfloat16()); the products run on v_mfma_f32_32x32x16_bf16, where every bf16 x bf16 product is exact in f32, and are
// accumulated in f32; the epilogue of the split family (scale / shift / ReLU, the FPN top-down add, the eSE column sums of the STORED
// outputs) is applied to the f32 accumulator and f32 is stored.  So  y = epilogue(sum_k bf16(x_k) bf16(w_k))  up to f32 accumulation
// error -- nothing else is rounded; against torch autocast, which also rounds every conv / BatchNorm / ReLU output to bf16, this is a
// strict subset of the roundings.  Against the UNROUNDED float64 product the error is <= (2^-7 + 2^-16 + acc) sum |a b| (two RNE
// roundings to 8 significant bits).  Fixed summation order, no float atomics: two launches give the same bits.
//
// Domain (every line has a test in tests/test_gpu_gemm_bf16.py):
//   * +-inf / NaN, and finite values above the largest bf16 (|x| > 0x1.FEp127 rounds to infinity): the output is what IEEE arithmetic
//     gives on the ROUNDED operands; its finiteness pattern is the definition's (an infinity times a zero of the same dot product is
//     NaN, as in the definition).
//   * operands whose bf16 rounding is subnormal (|x| < 2^-126): v_cvt_pk_bf16_f32 keeps them (the kernel mode keeps f32 subnormals)
//     and the MFMA does not flush its bf16 inputs (measured: subnormal operands against partners of 2^100 give the exact products).
//     The test holds only the derivable bound, which a flush would satisfy too: within sum over those terms of 2^-126 |partner| of
//     the definition.
//   * everything else finite is inside the domain.
//   * limits as the split family's (csrc/gemm_host.hpp): K % 32 == 0 / Cin % 32 == 0, x and W_packed 16-byte aligned, x_ld % 4 == 0,
//     32-bit ranges of one 128-row tile (1x1 forms) or of the whole input (conv form).
//
// Structure.  NOT srf_gemm_split_k with five products deleted: that kernel has 48 MFMAs per wave behind every pair of barriers, this one
// would have 8 (256 cycles), and the barriers and the staging would be the kernel.  Instead:
//   * workgroup tile 128 pixels x 128 channels, 4 waves = 2 x 2 wave tiles of 64 x 64, K in blocks of 64 (two 32-channel chunks: a
//     conv layer's chunk lies inside one tap, so the two halves of a block may belong to different taps; a K of 32 (mod 64) ends in a
//     half block whose missing chunk is loaded as zeros against zero-padded weights);
//   * two LDS stages of 32 KB (A 128 x 64 bf16 | B 128 x 64 bf16), ONE barrier per block of 64: block c + 1 is converted and written
//     into the other stage right behind the barrier that ended block c - 1 (write after the barrier, re-issue the loads of block c + 2
//     at once: cdna_hip_programming.md 5, "glds vs register staging", second row), then the 16 MFMAs (512 cycles) of block c are issued
//     from 16 ds_read_b128 -- one read per MFMA gap; 64 KB of LDS = two workgroups per CU;
//   * A is f32 in HBM and has to pass the vector ALU: thread (row = t / 8 + 32 j, oct = t % 8) loads 8 floats (2 buffer_load_b128),
//     rounds them with 4 v_cvt_pk_bf16_f32 (the split kernel: 11 instructions per pair) and writes one ds_write_b128;
//   * B is bf16, packed once per layer in the image order [block][column tile][col 128][slot 8][8 bf16], and copied linearly (16 bytes
//     per lane).  It goes through registers like A, not by LDS-DMA: both operands then sit in ONE queue that the compiler counts, where
//     an LDS-DMA beside ordinary loads makes hipcc drain the whole queue at every use of a load result (5, item 4(b)); at two
//     workgroups per CU the two stagings tie (same table, "128^2 tile ... at 2-3 blocks/CU: either");
//   * images: row r (128 bytes = 8 slots of 16) holds the channels 8 s .. 8 s + 7 of the block in slot s ^ ((r >> 1) & 7): sixteen
//     consecutive lanes of the loader's ds_write_b128 and of the fragment's ds_read_b128 cover every bank once (conflict-free);
//   * work item -> (column tile, row block) as in the split kernel: items b and b + 8 share an XCD, the column tiles of a row block
//     sit on one L2; all LDS in one __shared__ array; the epilogue is the split kernel's.
// Measured (tools/bench_img_bf16.py, the 28 distinct layer shapes of the LC camera branch, post-ReLU-like random data; DESIGN.md 4,
// profiles/img_bf16_layer_bench.json): 1x1 layers 417-563 TFLOP/s where the split GEMM reaches 173-206 (f32-equivalent), 3x3 layers
// 219-684 TFLOP/s of direct FLOPs where Winograd reaches 179-396; 0.05-0.27 of the 2.5 PFLOP/s dense peak, 15.9 ms against
// 26.1 ms for the 106 layers of a frame; the finest FPN lateral (256 -> 256 on 232 x 400, memory-bound) gains nothing (1.01x).
#include "common.hpp"
#include "gemm_tile128.hpp"

typedef __bf16 gb_bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 gb_bf8 __attribute__((ext_vector_type(8)));
typedef float gb_f2 __attribute__((ext_vector_type(2)));
typedef float gb_f4 __attribute__((ext_vector_type(4)));
typedef float gb_f16 __attribute__((ext_vector_type(16)));
typedef unsigned gb_u4 __attribute__((ext_vector_type(4)));

#define GB_IMG 16384              // bytes of one operand image: 128 rows x 64 bf16
#define GB_STAGE (2 * GB_IMG)     // A | B

// Not derived from SrfTile128Args: this family keeps its own argument struct and its own copy of the epilogue.  Its K loops are the
// one place where the compiler's choice between two forms of the weight-load address arithmetic flips with anything that changes
// around them (the struct's layout, a call that takes the accumulators): with the shared epilogue srf_gemm_bf16_k<GB_POOL> came out
// with other loads and waits inside the loop.  The decode and the whole host side are the shared ones (gemm_tile128.hpp).
struct GbArgs {
    const float *x;
    float *y;
    const unsigned char *Wp;
    const float *scale, *shift;
    long long x_ld, y_ld, M;
    int K, Cout, nchunk, nct, relu;   // nchunk: chunks of 32 channels (K / 32)
    int nblk;                         // blocks of 64: ceil(nchunk / 2)
    long long mblocks;
    // per-image row tiling + column sums of the stored outputs (eSE pooling), as GsArgs
    float *colsum;
    long long HW;
    int bpi;
    // FPN top-down step in the epilogue, as GsArgs
    const float *top;
    long long top_ld;
    int mapH, mapW, topH, topW;
    float sy, sx;
    // GB_CONV: implicit im2col, as GsArgs
    int H, W, Ho, Wo, kw, stride, pad, cin_chunks;
    long long x_bytes;
};
#define GB_PLAIN 0
#define GB_POOL 1
#define GB_TOPDOWN 2
#define GB_CONV 3

__device__ __forceinline__ unsigned gb_pk_bf16(float a, float b)
{
    const gb_f2 v = {a, b};
    const gb_bf2 h = __builtin_convertvector(v, gb_bf2);   // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
    return *reinterpret_cast<const unsigned *>(&h);
}

// W (Cout, K) row-major -> [block of 64][column tile of 128][col 128][slot 8][8 bf16]; slot s of column n holds the channels
// 8 (s ^ ((n >> 1) & 7)) .. + 7 of the block; columns >= Cout and channels >= K are zero
__global__ __launch_bounds__(256) void srf_gemm_bf16_pack_k(const float *__restrict__ Wt, int Cout, int K, int nct, unsigned short *__restrict__ P,
                                                           long long total)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int e = (int)(t & 7), s = (int)((t >> 3) & 7), n = (int)((t >> 6) & 127);
    const long long rest = t >> 13;
    const int ct = (int)(rest % nct), kb = (int)(rest / nct);
    const int oct = s ^ ((n >> 1) & 7);
    const int k = kb * 64 + oct * 8 + e, co = ct * 128 + n;
    const float x = (co < Cout && k < K) ? Wt[(size_t)co * K + k] : 0.f;
    P[t] = (unsigned short)(gb_pk_bf16(x, 0.f) & 0xffffu);
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void srf_gemm_bf16_k(GbArgs a)
{
    constexpr bool POOL = MODE == GB_POOL, TOPDOWN = MODE == GB_TOPDOWN, CONV = MODE == GB_CONV;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * GB_STAGE];   // stage 0 (A | B), stage 1 (A | B)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int ct;
    const long long mb = srf_tile128_row_block(a.nct, ct);
    if (mb >= a.mblocks) return;
    const SrfTile128Item it = srf_tile128_item<POOL>(ct, mb, a.M, a.HW, a.bpi);
    const long long p0 = it.p0, rows_here = it.rows_here;
    __amdgpu_buffer_rsrc_t xr = CONV ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, (int)a.x_bytes, 0x00020000)
                                     : __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x) + p0 * a.x_ld, 0, (int)(rows_here * a.x_ld * 4), 0x00020000);
    const int nblk = a.nblk, nchunk = a.nchunk;
    const size_t blk_stride = (size_t)a.nct * GB_IMG;
    const unsigned char *bsrc = a.Wp + (size_t)ct * GB_IMG + (size_t)tid * 16;

    // A loader: thread = (row r0 + 32 j, octet q of the block's 64 channels); its octet lies in chunk 2 c + (q >> 2)
    const int q = tid & 7, r0 = tid >> 3, half = q >> 2;
    const unsigned aoff0 = (unsigned)((r0 * a.x_ld + q * 8) * 4), aoff_step = (unsigned)(32 * a.x_ld * 4);   // rows past the block read as zero
    gb_f4 araw[4][2];
    gb_u4 braw[4];
    // CONV: the output pixel of each of this thread's rows as the input coordinates of tap (0, 0), and the (tap, chunk inside the
    // tap) of the thread's NEXT load, advanced by two chunks per block
    int cy[CONV ? 4 : 1], cx[CONV ? 4 : 1], cn[CONV ? 4 : 1];
    int l_c32 = half, l_cc = 0, l_ky = 0, l_kx = 0;
    if (CONV) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long p = p0 + r0 + 32 * j;
            const long long hw = (long long)a.Ho * a.Wo;
            const int n = (int)(p / hw);
            const int rem = (int)(p - n * hw);
            const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
            cn[j] = p < a.M ? n : -1;
            cy[j] = oy * a.stride - a.pad;
            cx[j] = ox * a.stride - a.pad;
        }
        const int tap = half / a.cin_chunks;
        l_cc = half - tap * a.cin_chunks;
        l_ky = tap / a.kw;
        l_kx = tap - l_ky * a.kw;
    }
    // loads of block C (called with C = 0, 1, 2, ... in order: the CONV state advances with every call)
#define GB_LOAD(C)                                                                                                         \
    do {                                                                                                                   \
        if (CONV) {                                                                                                        \
            const bool live_ = l_c32 < nchunk;                                                                             \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                                             \
                const int iy_ = cy[j_] + l_ky, ix_ = cx[j_] + l_kx;                                                        \
                const bool ok_ = live_ && cn[j_] >= 0 && iy_ >= 0 && iy_ < a.H && ix_ >= 0 && ix_ < a.W;                   \
                const unsigned off_ = ok_ ? (unsigned)(((((long long)cn[j_] * a.H + iy_) * a.W + ix_) * a.x_ld + l_cc * 32 + (q & 3) * 8) * 4) \
                                          : 0x80000000u;                                                                   \
                auto v0_ = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)off_, 0, 0);                                     \
                auto v1_ = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)(ok_ ? off_ + 16u : 0x80000000u), 0, 0);         \
                araw[j_][0] = *reinterpret_cast<gb_f4 *>(&v0_);                                                            \
                araw[j_][1] = *reinterpret_cast<gb_f4 *>(&v1_);                                                            \
            }                                                                                                              \
            l_c32 += 2;                                                                                                    \
            l_cc += 2;                                                                                                     \
            while (l_cc >= a.cin_chunks) {                                                                                 \
                l_cc -= a.cin_chunks;                                                                                      \
                if (++l_kx == a.kw) {                                                                                      \
                    l_kx = 0;                                                                                              \
                    ++l_ky;                                                                                                \
                }                                                                                                          \
            }                                                                                                              \
        } else {                                                                                                           \
            const bool live_ = 2 * (C) + half < nchunk;                                                                    \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                                             \
                const unsigned off_ = live_ ? aoff0 + j_ * aoff_step + (unsigned)(C) * 256u : 0x80000000u;                 \
                auto v0_ = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)off_, 0, 0);                                     \
                auto v1_ = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)(live_ ? off_ + 16u : 0x80000000u), 0, 0);       \
                araw[j_][0] = *reinterpret_cast<gb_f4 *>(&v0_);                                                            \
                araw[j_][1] = *reinterpret_cast<gb_f4 *>(&v1_);                                                            \
            }                                                                                                              \
        }                                                                                                                  \
        const gb_u4 *bb_ = reinterpret_cast<const gb_u4 *>(bsrc + (size_t)(C) * blk_stride);                               \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) braw[i_] = bb_[i_ * 256];                                         \
    } while (0)
    // round A (the one rounding of the definition) and write both operands into the stage at byte offset ST
#define GB_STORE(ST)                                                                                                       \
    do {                                                                                                                   \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                                                 \
            const int row_ = r0 + 32 * j_;                                                                                 \
            const gb_u4 w_ = {gb_pk_bf16(araw[j_][0][0], araw[j_][0][1]), gb_pk_bf16(araw[j_][0][2], araw[j_][0][3]),      \
                              gb_pk_bf16(araw[j_][1][0], araw[j_][1][1]), gb_pk_bf16(araw[j_][1][2], araw[j_][1][3])};     \
            *reinterpret_cast<gb_u4 *>(lds + (ST) + row_ * 128 + ((q ^ ((row_ >> 1) & 7)) << 4)) = w_;                     \
        }                                                                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) *reinterpret_cast<gb_u4 *>(lds + (ST) + GB_IMG + (tid + i_ * 256) * 16) = braw[i_]; \
    } while (0)

    const int wm = wave & 1, wn = wave >> 1;
    const int li = lane & 31, lh = lane >> 5;
    int a_off[2], b_off[2], swz_a[2], swz_b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + i * 32 + li, col = wn * 64 + i * 32 + li;
        a_off[i] = row * 128;
        b_off[i] = GB_IMG + col * 128;
        swz_a[i] = (row >> 1) & 7;
        swz_b[i] = (col >> 1) & 7;
    }
    gb_f16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    GB_LOAD(0);
    GB_STORE(0);
    if (nblk > 1) GB_LOAD(1);
    __syncthreads();
    for (int c = 0; c < nblk; ++c) {
        const int cur = (c & 1) * GB_STAGE;
        if (c + 1 < nblk) GB_STORE(cur ^ GB_STAGE);   // block c + 1; that stage was last read before the barrier that ended block c - 1
        if (c + 2 < nblk) GB_LOAD(c + 2);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            gb_bf8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const gb_bf8 *>(lds + cur + a_off[i] + (((2 * s + lh) ^ swz_a[i]) << 4));
                fb[i] = *reinterpret_cast<const gb_bf8 *>(lds + cur + b_off[i] + (((2 * s + lh) ^ swz_b[i]) << 4));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#undef GB_LOAD
#undef GB_STORE

    const long long rows_blk = it.rows_blk, slot = it.slot;
    // epilogue (a copy of srf_tile128_epilogue without the residual form, see GbArgs): lane = channel li of block j, accumulator register = pixel row (r & 3) + 8 (r >> 2) + 4 lh of block i
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
    int *s_top = reinterpret_cast<int *>(lds);   // [128]: offset (floats) of the top-level pixel each row of this block adds
    if (TOPDOWN) {
        // (the loop's last barrier is behind every fragment read of this workgroup)
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
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dr = i * 32 + (r & 3) + 8 * (r >> 2);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float v = __fmaf_rn(acc[i][j][r], sc[j], sh[j]);
                if (a.relu) v = fmaxf(v, 0.f);
                if (TOPDOWN && co_ok[j]) v = __fadd_rn(v, a.top[s_top[row_base + dr] + co0 + j * 32]);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yr, (int)(ybase[j] + (unsigned)dr * yrow_b), 0, 0);
                if (POOL) csum[j] += dr < rows_left ? v : 0.f;
            }
        }
    if (POOL) {
        // column sums of the block: the two lane halves of a wave (shuffle), then the two waves that share the columns (LDS), in a
        // fixed order: reproducible bit for bit
        float *red = reinterpret_cast<float *>(lds);   // [2][128]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float o = __shfl_xor(csum[j], 32);
            if (lh == 0) red[wm * 128 + wn * 64 + j * 32 + li] = csum[j] + o;
        }
        __syncthreads();
        if (tid < 128) {
            const int co = ct * 128 + tid;
            if (co < a.Cout) a.colsum[slot * a.Cout + co] = red[tid] + red[128 + tid];
        }
    }
}

extern "C" size_t srf_conv1x1_nhwc_bf16_packed_weight_bytes(int Cout, int K)
{
    if (Cout <= 0 || K <= 0 || (K & 31)) return 0;
    return (size_t)((K + 63) / 64) * srf_ceil_div(Cout, 128) * GB_IMG;
}

extern "C" int srf_conv1x1_nhwc_bf16_pack_weights(const float *W, int Cout, int K, void *packed, srf_stream_t stream)
{
    if (Cout <= 0 || K <= 0 || !W || !packed) return SRF_EINVAL;
    if (K & 31) return SRF_EUNSUPPORTED;
    const int nct = srf_ceil_div(Cout, 128);
    const long long total = (long long)(srf_conv1x1_nhwc_bf16_packed_weight_bytes(Cout, K) / 2);
    hipLaunchKernelGGL(srf_gemm_bf16_pack_k, dim3((unsigned)srf_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, W, Cout, K, nct,
                       (unsigned short *)packed, total);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

struct GbFamily {
    typedef GbArgs Args;
    static constexpr SrfGemmFamily limits = {128, true, 128};   // x and y through descriptors of one 128-row tile
    static constexpr void (*plain)(GbArgs) = srf_gemm_bf16_k<GB_PLAIN>, (*pool)(GbArgs) = srf_gemm_bf16_k<GB_POOL>,
                          (*topdown)(GbArgs) = srf_gemm_bf16_k<GB_TOPDOWN>, (*resid)(GbArgs) = nullptr,
                          (*conv)(GbArgs) = srf_gemm_bf16_k<GB_CONV>;
    static int set_weights(GbArgs &a, const void *W_packed)
    {
        a.Wp = (const unsigned char *)W_packed;
        a.nblk = (a.nchunk + 1) / 2;
        return SRF_OK;
    }
};

// srf_conv_gemm_nhwc_bf16: Conv2d(Cin, Cout, (kh, kw), stride, padding) on channels-last activations with an implicit im2col: in the
// bf16 mode the 3x3 / stride 1 layers too (no Winograd there: products of bf16-rounded TRANSFORMED data are another, worse arithmetic
// than the definition).  W_packed = srf_conv1x1_nhwc_bf16_pack_weights of the weight reordered to (Cout, kh * kw * Cin), tap slowest.
extern "C" int srf_conv_gemm_nhwc_bf16(const float *x, int N, int H, int W, int Cin, long long x_ld, const void *W_packed, int Cout, int kh,
                                       int kw, int stride, int pad, const float *scale, const float *shift, int relu, float *y,
                                       long long y_ld, srf_stream_t stream)
{
    return srf_tile128_conv<GbFamily>(x, N, H, W, Cin, x_ld, W_packed, Cout, kh, kw, stride, pad, scale, shift, relu, y, y_ld, stream);
}

extern "C" int srf_conv1x1_nhwc_bf16(const float *x, long long M, int K, long long x_ld, const void *W_packed, int Cout, const float *scale,
                                     const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream)
{
    return srf_tile128_plain<GbFamily>(x, M, K, x_ld, W_packed, Cout, scale, shift, relu, y, y_ld, stream);
}

extern "C" int srf_conv1x1_nhwc_bf16_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const void *W_packed, int Cout,
                                             const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt,
                                             long long top_ld, float *y, long long y_ld, srf_stream_t stream)
{
    return srf_tile128_topdown<GbFamily>(x, N, H, W, K, x_ld, W_packed, Cout, scale, shift, relu, top, Ht, Wt, top_ld, y, y_ld, stream);
}

// the pooled form: as srf_conv1x1_nhwc_split_pooled; workspace = srf_conv1x1_nhwc_pooled_workspace_bytes(N, HW, Cout)
extern "C" int srf_conv1x1_nhwc_bf16_pooled(const float *x, int N, long long HW, int K, long long x_ld, const void *W_packed, int Cout,
                                            const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean,
                                            void *workspace, size_t workspace_bytes, srf_stream_t stream)
{
    return srf_tile128_pooled<GbFamily>(x, N, HW, K, x_ld, W_packed, Cout, scale, shift, relu, y, y_ld, mean, workspace, workspace_bytes, stream);
}
