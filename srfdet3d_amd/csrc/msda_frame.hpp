// msda_frame.hpp -- the frame the multi-scale deformable attention forward (msda.hip) and backward (msda_bwd.hip) share.  The backward
// is the gradient of the forward "as that definition is written" (include/srfdet3d.h) and recomputes its softmax, sample positions,
// inside rule and corner addresses bit for bit: both kernels take them from here, so the two agree by construction.  Stated once:
//   * MsdaFrame: the argument fields both kernels read.  MsdaArgs and MsdaBwdArgs derive from it and add their own tensors;
//   * msda_item_index, msda_item, msda_batch: blockIdx.x -> XCD-contiguous workgroup -> (row, head), the lane of the head's segment;
//   * msda_softmax, msda_level_weights, msda_level_offsets, msda_sample, msda_value_rsrc: the definition's arithmetic;
//   * msda_frame_fill: every argument check in the order that is part of the ABI, the pyramid's prefix sums and the grid.  An entry
//     point states only the tensors of its own (MsdaTensor);
//   * msda_launch: runtime (head_dim, L, P) -> the instance of a kernel template.
// Each kernel's file keeps its own strategy: what a lane owns, when the loads are issued, how the results leave.
// The device functions take the fields they read as values, never a reference to the kernel's argument struct (gemm_tile128.hpp says
// why), and everything here is static inline / __device__ __forceinline__: the library is built one object per file.
#pragma once
#include <utility>

#include "common.hpp"

typedef float msda_f32x4 __attribute__((ext_vector_type(4)));
typedef float msda_f32x2 __attribute__((ext_vector_type(2)));

#define MSDA_OOB 0x80000000u   // a byte offset beyond every value table (each is below 2 GiB): the buffer load answers with zeros
#define MSDA_MAXL 4
#define MSDA_MAXP 4

struct MsdaFrame {
    const float *value, *ref, *offs, *logits;
    long long value_ld, offs_ld, logits_ld;
    long long items;                      // B Q heads
    long long value_bytes;
    int Q, S, heads;
    int H[MSDA_MAXL], W[MSDA_MAXL], start[MSDA_MAXL];
    unsigned per_xcd;                     // workgroups per XCD
};

// ---- device side ----------------------------------------------------------------------------------------------------------------
struct MsdaItem {
    long long r;       // row b Q + q
    int h;             // head
};

// Workgroups are handed out so that each XCD walks one contiguous eighth of the rows (blockIdx & 7 is the XCD): neighbouring queries
// sample neighbouring value rows, which then sit in that XCD's L2.  LPI lanes side by side share one (row, head): -> its index and
// the lane among the LPI.  A kernel leaves where the index is >= items, then decodes it (msda_item).  The two are apart, and the
// decode returns a value, so that the kernels keep the control flow they had with this text inline.
template <int LPI>
__device__ __forceinline__ long long msda_item_index(unsigned per_xcd, int &lane)
{
    const unsigned lb = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    const long long t = (long long)lb * 256 + threadIdx.x;
    lane = (int)(t & (LPI - 1));
    return t / LPI;
}

__device__ __forceinline__ MsdaItem msda_item(long long item, int heads)
{
    MsdaItem it;
    it.r = item / heads;
    it.h = (int)(item - it.r * heads);
    return it;
}

// the row's batch entry.  A 64-bit division is a branch: the kernels call this after msda_softmax, whose loads are then in flight
// across it (where hipcc had sunk the division while the softmax stood inline; before the softmax the 8 x 32 forward loses 0.7 %)
__device__ __forceinline__ int msda_batch(long long r, int Q) { return (int)(r / Q); }

// softmax over the L P logits of one (row, head): max-subtracted, summed in sample order, one reciprocal
template <int L, int P>
__device__ __forceinline__ void msda_softmax(const float *lrow, float (&w)[L * P])
{
    constexpr int NS = L * P;
    if constexpr (P == 4) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const msda_f32x4 v = *reinterpret_cast<const msda_f32x4 *>(lrow + 4 * l);
#pragma unroll
            for (int p = 0; p < 4; ++p) w[4 * l + p] = v[p];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) w[i] = lrow[i];
    }
    float m = w[0];
#pragma unroll
    for (int i = 1; i < NS; ++i) m = fmaxf(m, w[i]);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        w[i] = expf(w[i] - m);
        s += w[i];
    }
    const float rs = 1.f / s;
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] *= rs;
}

// level l's softmax weights: selects on the (uniform) level instead of a dynamically indexed register array
template <int L, int P>
__device__ __forceinline__ void msda_level_weights(const float (&w)[L * P], int l, float (&wl)[P])
{
#pragma unroll
    for (int p = 0; p < P; ++p) {
        wl[p] = w[p];
#pragma unroll
        for (int k = 1; k < L; ++k) wl[p] = l == k ? w[k * P + p] : wl[p];
    }
}

// level l's P (dx, dy) pixel offsets of one (row, head)
template <int P>
__device__ __forceinline__ void msda_level_offsets(const float *orow, int l, float (&dxy)[2 * P])
{
    if constexpr (P == 4) {
        const msda_f32x4 v0 = *reinterpret_cast<const msda_f32x4 *>(orow + 8 * l);
        const msda_f32x4 v1 = *reinterpret_cast<const msda_f32x4 *>(orow + 8 * l + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dxy[e] = v0[e];
            dxy[4 + e] = v1[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 2 * P; ++e) dxy[e] = orow[2 * P * l + e];
    }
}

// One sample of a level of Hl x Wl pixels whose first value row is row0.  Corners in the order (y0 x0), (y0 x1), (y1 x0), (y1 x1).
struct MsdaSample {
    bool in;          // the sample lies inside (-1, H) x (-1, W); outside, every ok[] is false
    bool ok[4];       // the corner is in the map
    long long row;    // value row of the corner (y0, x0); of use only where a corner is in the map
    float lx, ly;     // the fractions; hx = 1 - lx, hy = 1 - ly
    float cw[4];      // the corners' bilinear weights
};

__device__ __forceinline__ MsdaSample msda_sample(float rx, float ry, float dx, float dy, int Hl, int Wl, long long row0)
{
    MsdaSample s;
    const float Hf = (float)Hl, Wf = (float)Wl;
    // position: one fma and one subtraction (align_corners=False); the comparisons are false for NaN and for +-inf
    const float px = __fmaf_rn(rx, Wf, dx) - 0.5f;
    const float py = __fmaf_rn(ry, Hf, dy) - 0.5f;
    s.in = py > -1.f && py < Hf && px > -1.f && px < Wf;
    const float qx = s.in ? px : 0.f, qy = s.in ? py : 0.f;
    const float fx = floorf(qx), fy = floorf(qy);
    s.lx = qx - fx;
    s.ly = qy - fy;
    const float hx = 1.f - s.lx, hy = 1.f - s.ly;
    const int x0 = (int)fx, y0 = (int)fy;                               // in [-1, W - 1] x [-1, H - 1]
    const bool x0ok = s.in && x0 >= 0, x1ok = s.in && x0 + 1 < Wl;
    const bool y0ok = y0 >= 0, y1ok = y0 + 1 < Hl;
    s.ok[0] = y0ok && x0ok;
    s.ok[1] = y0ok && x1ok;
    s.ok[2] = y1ok && x0ok;
    s.ok[3] = y1ok && x1ok;
    s.row = row0 + (long long)y0 * Wl + x0;
    s.cw[0] = hy * hx;
    s.cw[1] = hy * s.lx;
    s.cw[2] = s.ly * hx;
    s.cw[3] = s.ly * s.lx;
    return s;
}

// the value table behind one buffer descriptor: a load at MSDA_OOB, or anywhere from value_bytes on, reads 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t msda_value_rsrc(const float *value, long long value_bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(value), 0, (int)value_bytes, 0x00020000);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// A tensor of an entry point's own, shaped like one of the forward's: value (B S rows of heads head_dim), offs (B Q rows of
// heads L P 2), logits (B Q rows of heads L P) or out (B Q rows of heads head_dim).
enum MsdaLike { MSDA_LIKE_VALUE, MSDA_LIKE_OFFS, MSDA_LIKE_LOGITS, MSDA_LIKE_OUT };

struct MsdaTensor {
    const void *ptr;
    long long ld;
    MsdaLike like;
    bool optional;   // may be NULL: its pitch is then ignored
};

#define MSDA_MAXOWN 4

// Checks the arguments in the order that is part of the ABI (signs; the domain; pitches against widths; the pyramid with its 2^31 row
// limit; each tensor below 2 GiB; nothing to do; null pointers; pitches % 4; 16-byte bases; the grid) and fills the frame.  `idle`:
// the entry point has nothing to write.  -> SRF_OK with the grid of LPI lanes per (row, head), 0 where there is nothing to do.
static inline int msda_frame_fill(MsdaFrame &f, const float *value, long long value_ld, int B, const int *shapes, int L, const float *ref,
                                  const float *offs, long long offs_ld, const float *logits, long long logits_ld, int Q, int heads,
                                  int head_dim, int P, const MsdaTensor *own, int nown, bool idle, int lpi, unsigned &grid)
{
    grid = 0;
    f = {value, ref, offs, logits, value_ld, offs_ld, logits_ld};   // the rest is filled as it is checked
    if (B < 0 || Q < 0 || L <= 0 || P <= 0 || heads <= 0 || head_dim <= 0 || !shapes) return SRF_EINVAL;
    if (L > MSDA_MAXL || P > MSDA_MAXP || (head_dim != 16 && head_dim != 32)) return SRF_EUNSUPPORTED;
    const long long C = (long long)heads * head_dim, NS = (long long)heads * L * P;
    const long long width[4] = {C, 2 * NS, NS, C};
    MsdaTensor t[3 + MSDA_MAXOWN] = {{value, value_ld, MSDA_LIKE_VALUE, false}, {offs, offs_ld, MSDA_LIKE_OFFS, false},
                                     {logits, logits_ld, MSDA_LIKE_LOGITS, false}};
    int nt = 3;
    for (int i = 0; i < nown && i < MSDA_MAXOWN; ++i)
        if (own[i].ptr || !own[i].optional) t[nt++] = own[i];   // a NULL optional tensor takes no further part
    for (int i = 0; i < nt; ++i)
        if (t[i].ld < width[t[i].like]) return SRF_EINVAL;
    long long S = 0;
    for (int l = 0; l < L; ++l) {
        const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
        if (Hl <= 0 || Wl <= 0) return SRF_EINVAL;
        if (S + (long long)Hl * Wl >= (1ll << 31)) return SRF_EUNSUPPORTED;
        f.H[l] = Hl;
        f.W[l] = Wl;
        f.start[l] = (int)S;
        S += (long long)Hl * Wl;
    }
    for (int l = L; l < MSDA_MAXL; ++l) f.H[l] = f.W[l] = f.start[l] = 0;
    const long long rows = (long long)B * Q, lim = 1ll << 31;
    // each tensor below 2 GiB: the value table is read through one buffer descriptor, the others are indexed in 32-bit-safe ranges
    auto fits = [](long long n, long long ld) { return n <= (lim / 4 - 1) / ld; };   // n ld floats stay below 2 GiB
    for (int i = 0; i < nt; ++i)
        if (!fits(t[i].like == MSDA_LIKE_VALUE ? (long long)B * S : rows, t[i].ld)) return SRF_EUNSUPPORTED;
    if (!fits(rows, 2 * L)) return SRF_EUNSUPPORTED;
    if (rows == 0 || idle) return SRF_OK;
    if (!ref) return SRF_EINVAL;
    for (int i = 0; i < nt; ++i)
        if (!t[i].ptr) return SRF_EINVAL;
    if ((uintptr_t)ref & 15) return SRF_EUNSUPPORTED;
    for (int i = 0; i < nt; ++i)
        if ((t[i].ld & 3) || ((uintptr_t)t[i].ptr & 15)) return SRF_EUNSUPPORTED;   // float4 rows on 16-byte bases
    f.items = rows * heads;
    f.value_bytes = (long long)B * S * value_ld * 4;
    f.Q = Q;
    f.S = (int)S;
    f.heads = heads;
    const long long nblk = (f.items * lpi + 255) / 256;
    const long long per_xcd = (nblk + 7) / 8;
    if (per_xcd * 8 >= lim) return SRF_EUNSUPPORTED;
    f.per_xcd = (unsigned)per_xcd;
    grid = (unsigned)(per_xcd * 8);
    return SRF_OK;
}

// runtime (head_dim, L, P) -> the kernel's instance K::get<head_dim, L, P>(), out of a table of all 2 x MSDA_MAXL x MSDA_MAXP
template <class K, class Args, int... I>
static inline void msda_launch_nth(std::integer_sequence<int, I...>, int i, unsigned grid, hipStream_t st, const Args &a)
{
    void (*const k[])(Args) = {K::template get<16 << (I / (MSDA_MAXL * MSDA_MAXP)), I / MSDA_MAXP % MSDA_MAXL + 1, I % MSDA_MAXP + 1>()...};
    hipLaunchKernelGGL(k[i], dim3(grid), dim3(256), 0, st, a);
}

template <class K, class Args>
static inline void msda_launch(int head_dim, int L, int P, unsigned grid, hipStream_t st, const Args &a)
{
    msda_launch_nth<K>(std::make_integer_sequence<int, 2 * MSDA_MAXL * MSDA_MAXP>(), ((head_dim == 32) * MSDA_MAXL + L - 1) * MSDA_MAXP + P - 1,
                       grid, st, a);
}
