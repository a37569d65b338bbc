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
#include "msda_frame.hpp"

struct MsdaBwdArgs : MsdaFrame {
    const float *gout;
    float *gvalue, *goffs, *glogits;      // each may be null
    long long gout_ld, gvalue_ld, goffs_ld, glogits_ld;
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
    int c;
    const long long item = msda_item_index<D>(a.per_xcd, c);
    if (item >= a.items) return;          // D divides 64: a segment's lanes leave together, the butterfly never meets a missing lane
    const MsdaItem it = msda_item(item, a.heads);
    const long long r = it.r;
    const int h = it.h;

    float w[NS];
    msda_softmax<L, P>(a.logits + r * a.logits_ld + h * NS, w);
    const int b = msda_batch(r, a.Q);   // here, behind the softmax: msda_frame.hpp says why

    __amdgpu_buffer_rsrc_t vrsrc = msda_value_rsrc(a.value, a.value_bytes);
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
        float wl[P], dxy[2 * P];
        msda_level_weights<L, P>(w, l, wl);
        const int Hl = a.H[l], Wl = a.W[l];
        const float rx = rrow[2 * l], ry = rrow[2 * l + 1];
        const long long row0 = (long long)b * a.S + a.start[l];
        msda_level_offsets<P>(orow, l, dxy);
        float tl[P], gxy[2 * P];
#pragma unroll
        for (int p0 = 0; p0 < P; p0 += 2) {
            constexpr int CH = 2;
            MsdaSample s[CH];
            float v[CH][4];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int p = p0 + k;
                if (p >= P) continue;
                s[k] = msda_sample(rx, ry, dxy[2 * p], dxy[2 * p + 1], Hl, Wl, row0);
                const unsigned b0 = (unsigned)(s[k].row * a.value_ld * 4) + (unsigned)(ch * 4);
                const unsigned row_b = (unsigned)Wl * px_b;
                const unsigned go[4] = {b0, b0 + px_b, b0 + row_b, b0 + row_b + px_b};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    auto ld = __builtin_amdgcn_raw_buffer_load_b32(vrsrc, (int)(s[k].ok[q] ? go[q] : MSDA_OOB), 0, 0);
                    v[k][q] = *reinterpret_cast<float *>(&ld);
                }
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int p = p0 + k;
                if (p >= P) continue;
                const float hx = 1.f - s[k].lx, hy = 1.f - s[k].ly;
                float sm = v[k][0] * s[k].cw[0];
                sm = __fmaf_rn(v[k][1], s[k].cw[1], sm);
                sm = __fmaf_rn(v[k][2], s[k].cw[2], sm);
                sm = __fmaf_rn(v[k][3], s[k].cw[3], sm);
                const float ddx = __fmaf_rn(s[k].ly, v[k][3] - v[k][2], hy * (v[k][1] - v[k][0]));
                const float ddy = __fmaf_rn(s[k].lx, v[k][3] - v[k][1], hx * (v[k][2] - v[k][0]));
                const float ts = mb_seg_sum<D>(g * sm), xs = mb_seg_sum<D>(g * ddx), ys = mb_seg_sum<D>(g * ddy);
                tl[p] = s[k].in ? ts : 0.f;
                gxy[2 * p] = s[k].in ? wl[p] * xs : 0.f;
                gxy[2 * p + 1] = s[k].in ? wl[p] * ys : 0.f;
            }
            if (a.gvalue) {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int p = p0 + k;
                    if (p >= P) continue;
                    const float ag = wl[p] * g;
                    float *dst = a.gvalue + ch;
                    const long long off[4] = {s[k].row, s[k].row + 1, s[k].row + Wl, s[k].row + Wl + 1};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (s[k].ok[q]) atomicAdd(dst + off[q] * a.gvalue_ld, ag * s[k].cw[q]);
                }
            }
        }
        if (a.goffs) {   // lane p of the segment stores point p's pair
            float *orow_g = a.goffs + r * a.goffs_ld + h * (NS * 2) + l * (2 * P);
#pragma unroll
            for (int p = 0; p < P; ++p)
                if (c == p) *reinterpret_cast<msda_f32x2 *>(orow_g + 2 * p) = msda_f32x2{gxy[2 * p], gxy[2 * p + 1]};
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
                *reinterpret_cast<msda_f32x4 *>(grow + 4 * k) = msda_f32x4{tj[4 * k], tj[4 * k + 1], tj[4 * k + 2], tj[4 * k + 3]};
            } else {
#pragma unroll
                for (int p = 0; p < P; ++p) grow[k * P + p] = tj[k * P + p];
            }
        }
    }
}

struct MsdaBwdKernel {
    template <int D, int L, int P>
    static constexpr auto get() { return &srf_msda_bwd_k<D, L, P>; }
};

extern "C" int srf_msda_bwd(const float *value, long long value_ld, int B, const int *shapes, int L, const float *ref, const float *offs,
                            long long offs_ld, const float *logits, long long logits_ld, int Q, int heads, int head_dim, int P,
                            const float *grad_out, long long grad_out_ld, float *grad_value, long long grad_value_ld, float *grad_offs,
                            long long grad_offs_ld, float *grad_logits, long long grad_logits_ld, srf_stream_t stream)
{
    MsdaBwdArgs a = {{}, grad_out, grad_value, grad_offs, grad_logits, grad_out_ld, grad_value_ld, grad_offs_ld, grad_logits_ld};
    const MsdaTensor own[] = {{grad_out, grad_out_ld, MSDA_LIKE_OUT, false},
                              {grad_value, grad_value_ld, MSDA_LIKE_VALUE, true},
                              {grad_offs, grad_offs_ld, MSDA_LIKE_OFFS, true},
                              {grad_logits, grad_logits_ld, MSDA_LIKE_LOGITS, true}};
    unsigned grid;
    const int rc = msda_frame_fill(a, value, value_ld, B, shapes, L, ref, offs, offs_ld, logits, logits_ld, Q, heads, head_dim, P, own, 4,
                                   !grad_value && !grad_offs && !grad_logits, head_dim, grid);
    if (rc != SRF_OK || grid == 0) return rc;
    msda_launch<MsdaBwdKernel>(head_dim, L, P, grid, (hipStream_t)stream, a);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
