// msda_bwd.hip -- multi-scale deformable attention, backward of the sampling core (csrc/msda.hip is the forward).  The definition is the
// one written out in include/srfdet3d.h under `srf_msda_bwd`; tests/msda_bwd_ref.py restates it in float64.
//
// Layout of the work.  The kernel is bound by the scatter into grad_value, and global float atomics run at their full rate when a
// wave-instruction adds whole row segments, one dword per lane.  So a thread is (row r = b Q + q, head h, channel c): D = head_dim lanes
// side by side own one head's segment of a value row (64 B at d = 16, 128 B at d = 32), a wave covers 4 (2) (row, head) pairs, and every
// atomic wave-instruction is 4 x 64 B or 2 x 128 B.  The forward's float4-per-lane layout would shape an atomic as 16 rows x 4 dwords at a
// 16-byte stride.  Every lane of a segment computes the softmax of its (row, head) and the sample positions itself, as the forward does.
// Samples are taken in chunks of at most two points of one level: the chunk's 8 corner dwords are gathered through the forward's buffer
// descriptor (a corner outside the map, and every corner of a sample outside (-1, H) x (-1, W), is an offset beyond its range and reads
// 0), the three inner products with grad_out are reduced over the segment's D lanes, then the chunk's 8 atomics go out.  The next chunk's
// gathers wait for them (loads and atomics share one counter), so at most 8 atomics of a wave are outstanding.
//   atomics: every one sits behind a branch on "sample inside and corner in the map"; none relies on a range check.
//   reduction over the channels: a butterfly over lane distances 1, 2, 4, 8 (, 16), the same for every launch; every lane ends with the
//   sum; lane p of the segment stores point p's pair of the level's grad_offs and, at the end, lane k level k of the row's grad_logits
//   (a select chain that picks "element e for lane e" becomes a scratch array under hipcc).
//   grad_logits: t[j] of all L P samples stay in registers; sum_j a[j] t[j] runs in sample order.
// Workgroups are handed out to the XCDs as in the forward, for the gathers' sake.
#include "common.hpp"

typedef float mb_f32x4 __attribute__((ext_vector_type(4)));
typedef float mb_f32x2 __attribute__((ext_vector_type(2)));

#define MB_OOB 0x80000000u
#define MB_MAXL 4

struct MsdaBwdArgs {
    const float *value, *ref, *offs, *logits, *gout;
    float *gvalue, *goffs, *glogits;      // each may be null
    long long value_ld, offs_ld, logits_ld, gout_ld, gvalue_ld, goffs_ld, glogits_ld;
    long long items;                      // B Q heads
    long long value_bytes;
    int Q, S, heads;
    int H[MB_MAXL], W[MB_MAXL], start[MB_MAXL];
    unsigned per_xcd;                     // workgroups per XCD
};

template <int D>
__device__ __forceinline__ float mb_seg_sum(float v)
{
#pragma unroll
    for (int m = 1; m < D; m <<= 1) v += __shfl_xor(v, m, D);
    return v;
}

template <int D, int L, int P>
__global__ __launch_bounds__(256) void srf_msda_bwd_k(MsdaBwdArgs a)
{
    constexpr int NS = L * P;
    static_assert(L <= D && P <= D, "one lane of the segment per stored point / level");
    const unsigned lb = (blockIdx.x & 7u) * a.per_xcd + (blockIdx.x >> 3);
    const long long t = (long long)lb * 256 + threadIdx.x;
    const long long item = t / D;
    if (item >= a.items) return;          // D divides 64: a segment's lanes leave together, the butterfly never meets a missing lane
    const int c = (int)(t & (D - 1));
    const long long r = item / a.heads;
    const int h = (int)(item - r * a.heads);
    const int b = (int)(r / a.Q);

    // ---- softmax over the L P logits of (r, h), exactly as the forward computes it ----
    const float *lrow = a.logits + r * a.logits_ld + h * NS;
    float w[NS];
    if constexpr (P == 4) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const mb_f32x4 v = *reinterpret_cast<const mb_f32x4 *>(lrow + 4 * l);
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

    __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.value), 0, (int)a.value_bytes, 0x00020000);
    const float *orow = a.offs + r * a.offs_ld + h * (NS * 2);
    const float *rrow = a.ref + r * (L * 2);
    const int ch = h * D + c;
    const float g = a.gout[r * a.gout_ld + ch];
    const unsigned px_b = (unsigned)(a.value_ld * 4);
    float tj[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) tj[i] = 0.f;
    // a real loop over the levels, as in the forward: one level's registers at a time
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        float wl[P];   // the level's softmax weights: selects on the (uniform) level instead of a dynamically indexed register array
#pragma unroll
        for (int p = 0; p < P; ++p) {
            wl[p] = w[p];
#pragma unroll
            for (int k = 1; k < L; ++k) wl[p] = l == k ? w[k * P + p] : wl[p];
        }
        const int Hl = a.H[l], Wl = a.W[l];
        const float Hf = (float)Hl, Wf = (float)Wl;
        const float rx = rrow[2 * l], ry = rrow[2 * l + 1];
        const long long row0 = (long long)b * a.S + a.start[l];
        float dxy[2 * P];
        if constexpr (P == 4) {
            const mb_f32x4 v0 = *reinterpret_cast<const mb_f32x4 *>(orow + 8 * l);
            const mb_f32x4 v1 = *reinterpret_cast<const mb_f32x4 *>(orow + 8 * l + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dxy[e] = v0[e];
                dxy[4 + e] = v1[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2 * P; ++e) dxy[e] = orow[2 * P * l + e];
        }
        float tl[P], gxy[2 * P];
#pragma unroll
        for (int p0 = 0; p0 < P; p0 += 2) {
            constexpr int CH = 2;
            long long row[CH];           // value row of the corner (y0, x0); used only where a corner is in the map
            bool ok[CH][4], in[CH];
            float cw[CH][4], lxs[CH], lys[CH], v[CH][4];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int p = p0 + k;
                if (p >= P) continue;
                // position: one fma and one subtraction (align_corners=False); the comparisons are false for NaN and for +-inf
                const float px = __fmaf_rn(rx, Wf, dxy[2 * p]) - 0.5f;
                const float py = __fmaf_rn(ry, Hf, dxy[2 * p + 1]) - 0.5f;
                in[k] = py > -1.f && py < Hf && px > -1.f && px < Wf;
                const float qx = in[k] ? px : 0.f, qy = in[k] ? py : 0.f;
                const float fx = floorf(qx), fy = floorf(qy);
                const float lx = qx - fx, ly = qy - fy, hx = 1.f - lx, hy = 1.f - ly;
                const int x0 = (int)fx, y0 = (int)fy;                   // in [-1, W - 1] x [-1, H - 1]
                const bool x0ok = in[k] && x0 >= 0, x1ok = in[k] && x0 + 1 < Wl;
                const bool y0ok = y0 >= 0, y1ok = y0 + 1 < Hl;
                ok[k][0] = y0ok && x0ok;
                ok[k][1] = y0ok && x1ok;
                ok[k][2] = y1ok && x0ok;
                ok[k][3] = y1ok && x1ok;
                row[k] = row0 + (long long)y0 * Wl + x0;
                cw[k][0] = hy * hx;
                cw[k][1] = hy * lx;
                cw[k][2] = ly * hx;
                cw[k][3] = ly * lx;
                lxs[k] = lx;
                lys[k] = ly;
                const unsigned b0 = (unsigned)(row[k] * a.value_ld * 4) + (unsigned)(ch * 4);
                const unsigned row_b = (unsigned)Wl * px_b;
                const unsigned go[4] = {b0, b0 + px_b, b0 + row_b, b0 + row_b + px_b};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    auto ld = __builtin_amdgcn_raw_buffer_load_b32(vrsrc, (int)(ok[k][q] ? go[q] : MB_OOB), 0, 0);
                    v[k][q] = *reinterpret_cast<float *>(&ld);
                }
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int p = p0 + k;
                if (p >= P) continue;
                const float hx = 1.f - lxs[k], hy = 1.f - lys[k];
                float sm = v[k][0] * cw[k][0];
                sm = __fmaf_rn(v[k][1], cw[k][1], sm);
                sm = __fmaf_rn(v[k][2], cw[k][2], sm);
                sm = __fmaf_rn(v[k][3], cw[k][3], sm);
                const float ddx = __fmaf_rn(lys[k], v[k][3] - v[k][2], hy * (v[k][1] - v[k][0]));
                const float ddy = __fmaf_rn(lxs[k], v[k][3] - v[k][1], hx * (v[k][2] - v[k][0]));
                const float ts = mb_seg_sum<D>(g * sm), xs = mb_seg_sum<D>(g * ddx), ys = mb_seg_sum<D>(g * ddy);
                tl[p] = in[k] ? ts : 0.f;
                gxy[2 * p] = in[k] ? wl[p] * xs : 0.f;
                gxy[2 * p + 1] = in[k] ? wl[p] * ys : 0.f;
            }
            if (a.gvalue) {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int p = p0 + k;
                    if (p >= P) continue;
                    const float ag = wl[p] * g;
                    float *dst = a.gvalue + ch;
                    const long long off[4] = {row[k], row[k] + 1, row[k] + Wl, row[k] + Wl + 1};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (ok[k][q]) atomicAdd(dst + off[q] * a.gvalue_ld, ag * cw[k][q]);
                }
            }
        }
        if (a.goffs) {   // lane p of the segment stores point p's pair
            float *orow_g = a.goffs + r * a.goffs_ld + h * (NS * 2) + l * (2 * P);
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (c == p) *reinterpret_cast<mb_f32x2 *>(orow_g + 2 * p) = mb_f32x2{gxy[2 * p], gxy[2 * p + 1]};
        }
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int k = 0; k < L; ++k) tj[k * P + p] += l == k ? tl[p] : 0.f;   // 0 + t, once: exact (the select-and-keep form goes to scratch at P = 3)
    }
    if (a.glogits) {
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NS; ++i) dot = __fmaf_rn(w[i], tj[i], dot);
#pragma unroll
        for (int i = 0; i < NS; ++i) tj[i] = w[i] * (tj[i] - dot);
        float *grow = a.glogits + r * a.glogits_ld + h * NS;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            if (c != k) continue;
            if constexpr (P == 4) {
                *reinterpret_cast<mb_f32x4 *>(grow + 4 * k) = mb_f32x4{tj[4 * k], tj[4 * k + 1], tj[4 * k + 2], tj[4 * k + 3]};
            } else {
#pragma unroll
                for (int p = 0; p < P; ++p) grow[k * P + p] = tj[k * P + p];
            }
        }
    }
}

template <int D, int L>
static void srf_msda_bwd_launch_p(int P, unsigned grid, hipStream_t st, const MsdaBwdArgs &a)
{
    switch (P) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_bwd_k<D, L, 1>), dim3(grid), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_bwd_k<D, L, 2>), dim3(grid), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_bwd_k<D, L, 3>), dim3(grid), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_bwd_k<D, L, 4>), dim3(grid), dim3(256), 0, st, a); break;
    }
}

template <int D>
static void srf_msda_bwd_launch(int L, int P, unsigned grid, hipStream_t st, const MsdaBwdArgs &a)
{
    switch (L) {
    case 1: srf_msda_bwd_launch_p<D, 1>(P, grid, st, a); break;
    case 2: srf_msda_bwd_launch_p<D, 2>(P, grid, st, a); break;
    case 3: srf_msda_bwd_launch_p<D, 3>(P, grid, st, a); break;
    default: srf_msda_bwd_launch_p<D, 4>(P, grid, st, a); break;
    }
}

extern "C" int srf_msda_bwd(const float *value, long long value_ld, int B, const int *shapes, int L, const float *ref, const float *offs,
                            long long offs_ld, const float *logits, long long logits_ld, int Q, int heads, int head_dim, int P,
                            const float *grad_out, long long grad_out_ld, float *grad_value, long long grad_value_ld, float *grad_offs,
                            long long grad_offs_ld, float *grad_logits, long long grad_logits_ld, srf_stream_t stream)
{
    if (B < 0 || Q < 0 || L <= 0 || P <= 0 || heads <= 0 || head_dim <= 0 || !shapes) return SRF_EINVAL;
    if (L > MB_MAXL || P > 4 || (head_dim != 16 && head_dim != 32)) return SRF_EUNSUPPORTED;
    const long long C = (long long)heads * head_dim, NS = (long long)heads * L * P;
    if (value_ld < C || grad_out_ld < C || offs_ld < 2 * NS || logits_ld < NS) return SRF_EINVAL;
    if ((grad_value && grad_value_ld < C) || (grad_offs && grad_offs_ld < 2 * NS) || (grad_logits && grad_logits_ld < NS)) return SRF_EINVAL;
    MsdaBwdArgs a;
    long long S = 0;
    for (int l = 0; l < L; ++l) {
        const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
        if (Hl <= 0 || Wl <= 0) return SRF_EINVAL;
        if (S + (long long)Hl * Wl >= (1ll << 31)) return SRF_EUNSUPPORTED;
        a.H[l] = Hl;
        a.W[l] = Wl;
        a.start[l] = (int)S;
        S += (long long)Hl * Wl;
    }
    for (int l = L; l < MB_MAXL; ++l) a.H[l] = a.W[l] = a.start[l] = 0;
    const long long rows = (long long)B * Q, lim = 1ll << 31;
    auto fits = [lim](long long n, long long ld) { return n <= (lim / 4 - 1) / ld; };   // n ld floats stay below 2 GiB
    if (!fits((long long)B * S, value_ld) || !fits(rows, offs_ld) || !fits(rows, logits_ld) || !fits(rows, grad_out_ld) || !fits(rows, 2 * L))
        return SRF_EUNSUPPORTED;
    if ((grad_value && !fits((long long)B * S, grad_value_ld)) || (grad_offs && !fits(rows, grad_offs_ld)) ||
        (grad_logits && !fits(rows, grad_logits_ld)))
        return SRF_EUNSUPPORTED;
    if (rows == 0 || (!grad_value && !grad_offs && !grad_logits)) return SRF_OK;
    if (!value || !ref || !offs || !logits || !grad_out) return SRF_EINVAL;
    if ((value_ld & 3) || (offs_ld & 3) || (logits_ld & 3) || (grad_out_ld & 3)) return SRF_EUNSUPPORTED;
    if ((grad_value && (grad_value_ld & 3)) || (grad_offs && (grad_offs_ld & 3)) || (grad_logits && (grad_logits_ld & 3)))
        return SRF_EUNSUPPORTED;
    if (((uintptr_t)value & 15) || ((uintptr_t)ref & 15) || ((uintptr_t)offs & 15) || ((uintptr_t)logits & 15) ||
        ((uintptr_t)grad_out & 15) || ((uintptr_t)grad_value & 15) || ((uintptr_t)grad_offs & 15) || ((uintptr_t)grad_logits & 15))
        return SRF_EUNSUPPORTED;
    a.value = value;
    a.ref = ref;
    a.offs = offs;
    a.logits = logits;
    a.gout = grad_out;
    a.gvalue = grad_value;
    a.goffs = grad_offs;
    a.glogits = grad_logits;
    a.value_ld = value_ld;
    a.offs_ld = offs_ld;
    a.logits_ld = logits_ld;
    a.gout_ld = grad_out_ld;
    a.gvalue_ld = grad_value_ld;
    a.goffs_ld = grad_offs_ld;
    a.glogits_ld = grad_logits_ld;
    a.items = rows * heads;
    a.value_bytes = (long long)B * S * value_ld * 4;
    a.Q = Q;
    a.S = (int)S;
    a.heads = heads;
    const long long nblk = (a.items * head_dim + 255) / 256;
    const long long per_xcd = (nblk + 7) / 8;
    if (per_xcd * 8 >= lim) return SRF_EUNSUPPORTED;
    a.per_xcd = (unsigned)per_xcd;
    if (head_dim == 16)
        srf_msda_bwd_launch<16>(L, P, (unsigned)(per_xcd * 8), (hipStream_t)stream, a);
    else
        srf_msda_bwd_launch<32>(L, P, (unsigned)(per_xcd * 8), (hipStream_t)stream, a);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
