// wgrad_bf16.hip -- srf_conv_wgrad_nhwc_bf16: the weight gradient of a stride-1 convolution on ONE bf16 product per f32 product.
//
//     dW[co][ci][ky][kx] = sum over p of bf16(g[p][co]) * bf16(X[p + tap][ci])
//
//     p = (n, y, x) runs over the N H W output pixels; p + tap = (n, y + ky - pad, x + kx - pad); k = 1 (pad 0) or 3 (pad 1).
//     * Each operand is rounded once, to nearest even (v_cvt_pk_bf16_f32 = Tensor.bfloat16()).
//     * Every product is exact in f32 (v_mfma_f32_32x32x16_bf16); accumulation is f32.
//     * Pixels outside the image contribute zero: X is zero-padded (a NaN of g times such a zero is NaN).
//     * Pixel ranges are added in a fixed order; no atomics; two launches give the same bytes.
//     * Non-finite values behave as IEEE arithmetic on the rounded operands.
//
// (tests/wgrad_bf16_ref.py opens with the same text and states it in numpy.)  The reduced-precision sibling of wgrad.hip, the caller's
// explicit choice (train_conv.mfma_dtype): 8 MFMAs per 32-pixel chunk and wave instead of 48, no split arithmetic.
//
// Structure.  With one product the 128 x 128 tile of wgrad.hip fed from f32 is no longer MFMA-bound: a chunk would stage 32 KB of f32
// for 32 MFMAs (1024 B per MFMA).  Here a PRE-PASS (srf_wgrad_bf16_pack_k) rounds g and X once into dense bf16 planes [pixel][channels
// padded to 8] in the workspace, and the GEMM stages those: 16 KB per chunk = 512 B per MFMA, 16-byte loads stored to the LDS as they
// come (no VALU between load and store).  The planes are written once and read once per tile that needs them (g: by every column tile,
// 18 times for 256 -> 256 3x3; X: by every row tile and all nine taps), so the pre-pass is a small share of the traffic.
//   * a K chunk = 32 consecutive output pixels; a workgroup tile = 128 output channels x 128 columns of the (tap, input channel) axis (one
//     tap's channels, or `flat`: 128 consecutive columns of the flattened axis when Cin % 32 == 0, as wgrad.hip); 4 waves = 2 x 2 wave
//     tiles of 64 x 64;
//   * LDS: two buffers of [g image | X image], an image = [pixel 32][channel 128] bf16 (256-byte rows, 16-byte chunks XOR-swizzled by
//     ((row & 3) << 2) | ((row >> 2) & 3): layout (b) of T10); chunk c + 1 is stored into the other buffer while chunk c is multiplied,
//     chunk c + 2 is in flight in registers: ONE barrier per chunk;
//   * fragments: ds_read_b64_tr_b16 hands every lane 4 consecutive PIXELS of one channel (a column of the image); the 16 reads of a
//     chunk and their s_waitcnt are ONE asm statement, so nothing can be scheduled between a read's issue and its wait;
//   * pixel ranges -> partial sums in the workspace -> srf_wgrad_bf16_reduce_k adds them in order (the equal of srf_wgrad_reduce_k: the
//     library is built one object per file, without relocatable device code).
// Any map width is taken (the loader's pixel walk wraps as often as it has to), channel counts multiples of 4.
#include "common.hpp"

typedef __bf16 wb_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 wb_bf2 __attribute__((ext_vector_type(2)));
typedef float wb_f2 __attribute__((ext_vector_type(2)));
typedef float wb_f4 __attribute__((ext_vector_type(4)));
typedef float wb_f16 __attribute__((ext_vector_type(16)));
typedef unsigned wb_u2 __attribute__((ext_vector_type(2)));
typedef unsigned wb_u4 __attribute__((ext_vector_type(4)));

#define WB_IMG 8192          /* bytes of one operand image: 32 pixels x 256 B */
#define WB_BUF (2 * WB_IMG)  /* one buffer: g image | X image */
#define WB_OOB 0x80000000u   /* a buffer offset past every descriptor: the load returns zero */

struct WbArgs {
    const void *gp, *xp;   // the bf16 planes
    float *partial;
    long long P;
    int N, H, W, Cin, Cout, kw, pad, taps;
    int g_pitch, x_pitch;   // bytes of one pixel of a plane
    int mtiles, ctiles, nsplit, chunks_per_split, nchunks;
    int g_bytes, x_bytes;
    int flat;
};

__device__ __forceinline__ unsigned wb_pk_bf16(float a, float b)
{
    const wb_f2 v = {a, b};
    const wb_bf2 h = __builtin_convertvector(v, wb_bf2);   // v_cvt_pk_bf16_f32: round to nearest even
    return *reinterpret_cast<const unsigned *>(&h);
}

// src: P pixels of pitch ld floats, C channels (C % 4 == 0) -> dst: P pixels of C8 groups of 8 bf16, channels past C zero
__global__ __launch_bounds__(256) void srf_wgrad_bf16_pack_k(const float *__restrict__ src, long long ld, long long P, int C, int C8,
                                                             wb_u4 *__restrict__ dst)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= P * C8) return;
    const long long p = e / C8;
    const int c = 8 * (int)(e - p * C8);
    const float *s = src + p * ld + c;
    const wb_f4 z = {0.f, 0.f, 0.f, 0.f};
    const wb_f4 a = c < C ? *reinterpret_cast<const wb_f4 *>(s) : z;
    const wb_f4 b = c + 4 < C ? *reinterpret_cast<const wb_f4 *>(s + 4) : z;
    dst[e] = wb_u4{wb_pk_bf16(a[0], a[1]), wb_pk_bf16(a[2], a[3]), wb_pk_bf16(b[0], b[1]), wb_pk_bf16(b[2], b[3])};
}

__global__ __launch_bounds__(256, 2) void srf_wgrad_bf16_k(WbArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * WB_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // work item -> (pixel range, column tile, row tile), as wgrad.hip
    int b = blockIdx.x;
    const int mt = b % a.mtiles;
    b /= a.mtiles;
    const int ntiles = a.flat ? a.ctiles : a.taps * a.ctiles;
    const int nt = b % ntiles, sp = b / ntiles;
    const int co0 = mt * 128;
    // 32-channel group j of the tile -> its tap and its first input channel (computed where needed: no indexed array, no scratch)
    auto group = [&](int j, int &tap, int &c0) {
        if (a.flat) {
            const int f0 = nt * 128 + 32 * j;
            tap = f0 / a.Cin;
            c0 = f0 - tap * a.Cin;
            if (tap >= a.taps) {   // past the last column: nothing to load (channel a.Cin does not exist)
                tap = a.taps - 1;
                c0 = a.Cin;
            }
        } else {
            tap = nt / a.ctiles;
            c0 = (nt - tap * a.ctiles) * 128 + 32 * j;
        }
    };
    const int c_begin = sp * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    c_end = c_end < a.nchunks ? c_end : a.nchunks;

    __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.gp), 0, a.g_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.xp), 0, a.x_bytes, 0x00020000);

    // ---- loader: this thread's pixel of the chunk and its two 16-byte channel groups cq = qg + 8 j of either image ----
    const int pxl = tid >> 3, qg = tid & 7;
    long long p = (long long)c_begin * 32 + pxl;           // output pixel of the NEXT chunk to be loaded
    int ox, oy, n;
    {
        const long long hw = (long long)a.H * a.W;
        n = (int)(p / hw);
        const int rem = (int)(p - (long long)n * hw);
        oy = rem / a.W;
        ox = rem - oy * a.W;
    }
    const int g_c8 = a.g_pitch >> 4, x_c8 = a.x_pitch >> 4;   // 8-channel groups of a plane's pixel
    unsigned gcol[2], xcol[2];   // byte offset of the group inside a pixel of the plane, WB_OOB when the plane has no such channels
    int dyj[2], dxj[2];          // the tap's shift: that of the 32-channel group (qg >> 2) + 2 j
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cq = qg + 8 * j;
        const int gq = (co0 >> 3) + cq;
        gcol[j] = gq < g_c8 ? (unsigned)(gq * 16) : WB_OOB;
        int c0, tp;
        group((qg >> 2) + 2 * j, tp, c0);
        const int ch = c0 + 8 * (cq & 3);
        xcol[j] = (c0 < a.Cin && (ch >> 3) < x_c8) ? (unsigned)(ch * 2) : WB_OOB;
        const int ky = tp / a.kw;
        dyj[j] = ky - a.pad;
        dxj[j] = tp - ky * a.kw - a.pad;
    }
    wb_u4 graw[2], xraw[2];
#define WB_LOAD()                                                                                                          \
    do {                                                                                                                   \
        const bool pok_ = p < a.P;                                                                                         \
        const unsigned grow_ = pok_ ? (unsigned)(p * a.g_pitch) : WB_OOB;                                                  \
        _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                                                 \
            const int iy_ = oy + dyj[j_], ix_ = ox + dxj[j_];                                                              \
            const bool xok_ = pok_ && iy_ >= 0 && iy_ < a.H && ix_ >= 0 && ix_ < a.W;                                      \
            const unsigned xrow_ = xok_ ? (unsigned)((((long long)n * a.H + iy_) * a.W + ix_) * a.x_pitch) : WB_OOB;       \
            const unsigned go_ = ((grow_ | gcol[j_]) & WB_OOB) ? WB_OOB : grow_ + gcol[j_];                                \
            const unsigned xo_ = ((xrow_ | xcol[j_]) & WB_OOB) ? WB_OOB : xrow_ + xcol[j_];                                \
            auto vg_ = __builtin_amdgcn_raw_buffer_load_b128(gr, (int)go_, 0, 0);                                          \
            graw[j_] = *reinterpret_cast<wb_u4 *>(&vg_);                                                                   \
            auto vx_ = __builtin_amdgcn_raw_buffer_load_b128(xr, (int)xo_, 0, 0);                                          \
            xraw[j_] = *reinterpret_cast<wb_u4 *>(&vx_);                                                                   \
        }                                                                                                                  \
        p += 32;                                                                                                           \
        ox += 32;                                                                                                          \
        while (ox >= a.W) {                                                                                                \
            ox -= a.W;                                                                                                     \
            if (++oy >= a.H) {                                                                                             \
                oy = 0;                                                                                                    \
                ++n;                                                                                                       \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)
    // store addresses: row pxl, 16-byte chunk cq = qg + 8 j
    const int swr = ((pxl & 3) << 2) | ((pxl >> 2) & 3);
    unsigned sto[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) sto[j] = (unsigned)(256 * pxl + 16 * ((qg + 8 * j) ^ swr));
#define WB_STORE(BOFF)                                                                                                     \
    do {                                                                                                                   \
        _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                                                 \
            *reinterpret_cast<wb_u4 *>(lds + (BOFF) + sto[j_]) = graw[j_];                                                 \
            *reinterpret_cast<wb_u4 *>(lds + (BOFF) + WB_IMG + sto[j_]) = xraw[j_];                                        \
        }                                                                                                                  \
    } while (0)

    // ---- fragments: lane (group g = lane / 16, i = lane % 16 = 4 q + p) of a transposed read supplies the address of block row q,
    // columns 4 p .. 4 p + 3; the block of (k step, 32-row tile T, half h) starts at pixel 16 ks + 8 (g >> 1) + 4 h, channel
    // 32 T + 16 (g & 1) ----
    const int wm = wave & 1, wn = wave >> 1;
    const int grp = lane >> 4, li16 = lane & 15, tq = li16 >> 2, tp = li16 & 3;
    unsigned fad[2][2][2];   // [operand][tile of the wave's two][half], LDS byte address for k step 0, buffer 0
    const unsigned lds0 = (unsigned)(uintptr_t)lds;
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int T = (o == 0 ? wm : wn) * 2 + t;
                const int row = 8 * (grp >> 1) + 4 * h + tq;
                const int ch = T * 4 + 2 * (grp & 1) + (tp >> 1);
                const int sw = ((row & 3) << 2) | ((row >> 2) & 3);
                fad[o][t][h] = lds0 + (unsigned)(o * WB_IMG + 256 * row + 16 * (ch ^ sw) + 8 * (tp & 1));
            }
    wb_f16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the 16 transposed reads of a chunk (k step 1: rows + 16 = + 4096 bytes, the swizzle is unchanged by it) and their wait: one statement
#define WB_READ(BOFF)                                                                                                      \
    do {                                                                                                                   \
        const unsigned a0_ = fad[0][0][0] + (BOFF), a1_ = fad[0][0][1] + (BOFF), a2_ = fad[0][1][0] + (BOFF), a3_ = fad[0][1][1] + (BOFF); \
        const unsigned a4_ = fad[1][0][0] + (BOFF), a5_ = fad[1][0][1] + (BOFF), a6_ = fad[1][1][0] + (BOFF), a7_ = fad[1][1][1] + (BOFF); \
        asm volatile("ds_read_b64_tr_b16 %0, %16\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %1, %17\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %2, %18\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %3, %19\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %4, %20\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %5, %21\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %6, %22\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %7, %23\n\t"                                                                      \
                     "ds_read_b64_tr_b16 %8, %16 offset:4096\n\t"                                                          \
                     "ds_read_b64_tr_b16 %9, %17 offset:4096\n\t"                                                          \
                     "ds_read_b64_tr_b16 %10, %18 offset:4096\n\t"                                                         \
                     "ds_read_b64_tr_b16 %11, %19 offset:4096\n\t"                                                         \
                     "ds_read_b64_tr_b16 %12, %20 offset:4096\n\t"                                                         \
                     "ds_read_b64_tr_b16 %13, %21 offset:4096\n\t"                                                         \
                     "ds_read_b64_tr_b16 %14, %22 offset:4096\n\t"                                                         \
                     "ds_read_b64_tr_b16 %15, %23 offset:4096\n\t"                                                         \
                     "s_waitcnt lgkmcnt(0)"                                                                                \
                     : "=&v"(rd[0]), "=&v"(rd[1]), "=&v"(rd[2]), "=&v"(rd[3]), "=&v"(rd[4]), "=&v"(rd[5]), "=&v"(rd[6]), "=&v"(rd[7]),      \
                       "=&v"(rd[8]), "=&v"(rd[9]), "=&v"(rd[10]), "=&v"(rd[11]), "=&v"(rd[12]), "=&v"(rd[13]), "=&v"(rd[14]), "=&v"(rd[15]) \
                     : "v"(a0_), "v"(a1_), "v"(a2_), "v"(a3_), "v"(a4_), "v"(a5_), "v"(a6_), "v"(a7_)                          \
                     : "memory");                                                                                          \
    } while (0)
    // rd[8 ks + 4 o + 2 t + h] -> the fragment of (k step, operand, tile): its two halves side by side
#define WB_FRAG(KS, O, T) __builtin_bit_cast(wb_bf8, (wb_u4{rd[8 * (KS) + 4 * (O) + 2 * (T)][0], rd[8 * (KS) + 4 * (O) + 2 * (T)][1], \
                                                            rd[8 * (KS) + 4 * (O) + 2 * (T) + 1][0], rd[8 * (KS) + 4 * (O) + 2 * (T) + 1][1]}))
#define WB_MM()                                                                                                            \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 2; ++ks_) {                                                                  \
        const wb_bf8 fa0_ = WB_FRAG(ks_, 0, 0), fa1_ = WB_FRAG(ks_, 0, 1), fb0_ = WB_FRAG(ks_, 1, 0), fb1_ = WB_FRAG(ks_, 1, 1); \
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0_, fb0_, acc[0][0], 0, 0, 0);                               \
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0_, fb1_, acc[0][1], 0, 0, 0);                               \
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1_, fb0_, acc[1][0], 0, 0, 0);                               \
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1_, fb1_, acc[1][1], 0, 0, 0);                               \
    }

    if (c_begin < c_end) {
        wb_u2 rd[16];
        WB_LOAD();
        WB_STORE(0);
        WB_LOAD();   // (a chunk past the range reads pixels of the next range or none: loaded, stored, never multiplied)
        __syncthreads();
        unsigned boff = 0;
        for (int c = c_begin; c < c_end; ++c) {
            WB_READ(boff);
            WB_MM();
            WB_STORE(boff ^ WB_BUF);   // chunk c + 1 into the other buffer: its last readers passed the barrier of chunk c - 1
            WB_LOAD();                 // chunk c + 2
            __syncthreads();
            boff ^= WB_BUF;
        }
    }
#undef WB_LOAD
#undef WB_STORE
#undef WB_READ
#undef WB_FRAG
#undef WB_MM

    // ---- epilogue: accumulator register r of tile (i, j) = row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the 32 x 32 tile, column lane & 31 ----
    const int li = lane & 31, lh = lane >> 5;
    const long long NC = (long long)a.taps * a.Cin;
    float *dst = a.partial + (size_t)sp * a.Cout * NC;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int c0, tpj;
            group(wn * 2 + j, tpj, c0);   // the 32-channel group of the tile this accumulator tile holds
            const int ci = c0 + li;
            if (ci >= a.Cin) continue;
            const size_t col = (size_t)tpj * a.Cin + ci;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (co < a.Cout) dst[(size_t)co * NC + col] = acc[i][j][r];
            }
        }
}

// dW[co][ci][tap] = sum over the pixel ranges s = 0, 1, ... (in this order) of partial[s][co][tap Cin + ci]
__global__ __launch_bounds__(256) void srf_wgrad_bf16_reduce_k(const float *__restrict__ partial, int nsplit, int Cout, int Cin, int taps,
                                                             float *__restrict__ dW)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long NC = (long long)taps * Cin, total = (long long)Cout * NC;
    if (e >= total) return;
    const int co = (int)(e / NC);
    const int rem = (int)(e - (long long)co * NC);
    const int tap = rem / Cin, ci = rem - tap * Cin;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s = __fadd_rn(s, partial[(size_t)k * total + e]);
    dW[((size_t)co * Cin + ci) * taps + tap] = s;
}

static bool wb_flat(int Cin, int taps) { return taps > 1 && (Cin & 31) == 0 && (Cin & 127) != 0; }

struct WbPlan {
    int mtiles, ctiles, nsplit, cps, nchunks;
    size_t partial_bytes, g_off, x_off, total;   // the workspace: partial sums | g plane | X plane, each 256-byte aligned
    int g_pitch, x_pitch;
};

static size_t wb_up256(size_t v) { return (v + 255) & ~(size_t)255; }

static void wb_plan(long long P, int Cin, int Cout, int taps, WbPlan *pl)
{
    pl->mtiles = srf_ceil_div(Cout, 128);
    pl->ctiles = wb_flat(Cin, taps) ? srf_ceil_div(taps * Cin, 128) : srf_ceil_div(Cin, 128);
    const long long nch = (P + 31) / 32;            // P < 2^29 (P x 4 bytes x a pitch of at least 4 floats lies below 2^31)
    pl->nchunks = (int)nch;
    const int tiles = pl->mtiles * (wb_flat(Cin, taps) ? pl->ctiles : pl->ctiles * taps);
    int ns = srf_ceil_div(768, tiles);          // ~1.5 rounds of 512 co-resident workgroups
    const int most = (int)((nch + 15) / 16);    // a range is at least 16 chunks deep
    ns = ns > most ? most : ns;
    ns = ns < 1 ? 1 : ns;
    pl->cps = (int)((nch + ns - 1) / ns);
    pl->nsplit = (int)((nch + pl->cps - 1) / pl->cps);
    pl->g_pitch = ((Cout + 7) / 8) * 16;
    pl->x_pitch = ((Cin + 7) / 8) * 16;
    pl->partial_bytes = (size_t)pl->nsplit * Cout * (size_t)taps * Cin * sizeof(float);
    pl->g_off = wb_up256(pl->partial_bytes);
    pl->x_off = pl->g_off + wb_up256((size_t)P * pl->g_pitch);
    pl->total = pl->x_off + wb_up256((size_t)P * pl->x_pitch);
}

extern "C" size_t srf_conv_wgrad_bf16_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ksize)
{
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3)) return 0;
    const long long P = (long long)N * H * W;
    if (P * Cin * 4 >= (1ll << 31) || P * Cout * 4 >= (1ll << 31)) return 0;
    WbPlan pl;
    wb_plan(P, Cin, Cout, ksize * ksize, &pl);
    return pl.total;
}

// g: (N, H, W, g_ld) channels-last gradient of the layer's output (Cout channels); x: (N, H, W, x_ld) its input (Cin channels);
// dW: (Cout, Cin, ksize, ksize) contiguous.  ksize 1 (padding 0) or 3 (padding 1), stride 1.  Cin, Cout multiples of 4, every tensor
// below 2 GB, g_ld / x_ld multiples of 4 with 16-byte aligned bases and workspace; else SRF_EUNSUPPORTED.
extern "C" int srf_conv_wgrad_nhwc_bf16(const float *g, long long g_ld, const float *x, long long x_ld, int N, int H, int W, int Cin, int Cout,
                                        int ksize, void *workspace, size_t workspace_bytes, float *dW, srf_stream_t stream)
{
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || g_ld < Cout || x_ld < Cin || !g || !x || !dW || !workspace) return SRF_EINVAL;
    if ((ksize != 1 && ksize != 3) || (Cin & 3) || (Cout & 3) || (g_ld & 3) || (x_ld & 3)) return SRF_EUNSUPPORTED;
    if (((uintptr_t)g & 15) || ((uintptr_t)x & 15) || ((uintptr_t)workspace & 15)) return SRF_EUNSUPPORTED;
    const long long P = (long long)N * H * W;
    if (P * g_ld * 4 >= (1ll << 31) || P * x_ld * 4 >= (1ll << 31)) return SRF_EUNSUPPORTED;
    WbPlan pl;
    wb_plan(P, Cin, Cout, ksize * ksize, &pl);
    if (workspace_bytes < pl.total) return SRF_EWORKSPACE;
    WbArgs a;
    a.gp = (const char *)workspace + pl.g_off;
    a.xp = (const char *)workspace + pl.x_off;
    a.partial = (float *)workspace;
    a.P = P;
    a.N = N;
    a.H = H;
    a.W = W;
    a.Cin = Cin;
    a.Cout = Cout;
    a.kw = ksize;
    a.pad = ksize / 2;
    a.taps = ksize * ksize;
    a.g_pitch = pl.g_pitch;
    a.x_pitch = pl.x_pitch;
    a.mtiles = pl.mtiles;
    a.ctiles = pl.ctiles;
    a.nsplit = pl.nsplit;
    a.chunks_per_split = pl.cps;
    a.nchunks = pl.nchunks;
    a.g_bytes = (int)(P * pl.g_pitch);   // pitch <= 2 (C + 4) <= 4 C bytes: below 2^31 with the f32 tensor
    a.x_bytes = (int)(P * pl.x_pitch);
    a.flat = wb_flat(Cin, a.taps) ? 1 : 0;
    const long long blocks = (long long)a.nsplit * (a.flat ? a.ctiles : a.taps * a.ctiles) * a.mtiles;
    if (blocks >= (1ll << 31)) return SRF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int g8 = pl.g_pitch / 16, x8 = pl.x_pitch / 16;
    hipLaunchKernelGGL(srf_wgrad_bf16_pack_k, dim3((unsigned)srf_ceil_div(P * g8, 256)), dim3(256), 0, st, g, g_ld, P, Cout, g8,
                       (wb_u4 *)((char *)workspace + pl.g_off));
    hipLaunchKernelGGL(srf_wgrad_bf16_pack_k, dim3((unsigned)srf_ceil_div(P * x8, 256)), dim3(256), 0, st, x, x_ld, P, Cin, x8,
                       (wb_u4 *)((char *)workspace + pl.x_off));
    hipLaunchKernelGGL(srf_wgrad_bf16_k, dim3((unsigned)blocks), dim3(256), 0, st, a);
    const long long total = (long long)Cout * a.taps * Cin;
    hipLaunchKernelGGL(srf_wgrad_bf16_reduce_k, dim3((unsigned)srf_ceil_div(total, 256)), dim3(256), 0, st, a.partial, a.nsplit, Cout, Cin, a.taps, dW);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
