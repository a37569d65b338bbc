// msda.hip -- multi-scale deformable attention, forward (the sampling core of mmcv's `MultiScaleDeformableAttention`).
//
// Reference call site: the two `BaseTransformerLayer`s of `encoder_lidar`, mmdet3d_plugin/models/sparse_heads/srfdet_head.py:241-263 and
// :657-758 (`_get_lidar_encoder_feats`, behind `with_lidar_encoder=True`).  The operator's definition is the one written out in
// include/srfdet3d.h; tests/msda_ref.py restates it in float64.
//
// Layout of the work.  The unit of reading is one head's segment of a value row: head_dim floats = 64 B (d = 16) or 128 B (d = 32), read
// as LPS = d / 4 lanes x float4.  A thread is (row r = b Q + q, head h, float4 c4 of the head): a 256-thread workgroup covers 256 / LPS
// (row, head) pairs = 8 (4) whole queries of 8 heads, and a wave's store is 1 KiB of consecutive output.  Every lane of a segment computes
// the softmax of its (row, head) and the sample positions itself (the LPS lanes read the same logits and offsets: one request); the 16
// weights stay in registers.  Per level the P samples' corner addresses and weights are set up first, then all 4 P loads are issued, then
// the fma chain runs: no branch sits between a load and its use.  A corner outside the map, and every corner of a sample outside
// (-1, H) x (-1, W), is a load at an offset beyond the buffer descriptor's range, which the hardware answers with zeros.
//   summation order, fixed: level, then point, then the corners (y0 x0), (y0 x1), (y1 x0), (y1 x1); one fma chain per output, no atomics.
// Workgroups are handed out so that each XCD walks one contiguous eighth of the rows (blockIdx & 7 is the XCD): neighbouring queries sample
// neighbouring value rows, which then sit in that XCD's L2.
#include "common.hpp"

typedef float ms_f32x4 __attribute__((ext_vector_type(4)));

#define MS_OOB 0x80000000u
#define MS_MAXL 4

struct MsdaArgs {
    const float *value, *ref, *offs, *logits;
    float *out;
    long long value_ld, offs_ld, logits_ld, out_ld;
    long long items;                      // B Q heads
    long long value_bytes;
    int Q, S, heads;
    int H[MS_MAXL], W[MS_MAXL], start[MS_MAXL];
    unsigned per_xcd;                     // workgroups per XCD
};

template <int LPS, int L, int P>
__global__ __launch_bounds__(256, 3) void srf_msda_fwd_k(MsdaArgs a)
{
    constexpr int D = LPS * 4, NS = L * P;
    const unsigned lb = (blockIdx.x & 7u) * a.per_xcd + (blockIdx.x >> 3);
    const long long t = (long long)lb * 256 + threadIdx.x;
    const long long item = t / LPS;
    if (item >= a.items) return;
    const int c4 = (int)(t & (LPS - 1));
    const long long r = item / a.heads;
    const int h = (int)(item - r * a.heads);
    const int b = (int)(r / a.Q);

    // ---- softmax over the L P logits of (r, h): max-subtracted, summed in sample order, one reciprocal ----
    const float *lrow = a.logits + r * a.logits_ld + h * NS;
    float w[NS];
    if constexpr (P == 4) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const ms_f32x4 v = *reinterpret_cast<const ms_f32x4 *>(lrow + 4 * l);
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
    const unsigned seg_b = (unsigned)((h * D + c4 * 4) * 4);
    const unsigned px_b = (unsigned)(a.value_ld * 4);
    ms_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // a real loop over the levels: unrolled, hipcc hoists every level's loads to the top (256 VGPRs, one wave per SIMD, spills under a
    // tighter bound).  One level's 4 P loads are in flight per lane at a time; 130 VGPRs, three waves per SIMD, no scratch.
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
        const unsigned row_b = (unsigned)Wl * px_b;
        const long long row0 = (long long)b * a.S + a.start[l];
        float dxy[2 * P];
        if constexpr (P == 4) {
            const ms_f32x4 v0 = *reinterpret_cast<const ms_f32x4 *>(orow + 8 * l);
            const ms_f32x4 v1 = *reinterpret_cast<const ms_f32x4 *>(orow + 8 * l + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dxy[e] = v0[e];
                dxy[4 + e] = v1[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2 * P; ++e) dxy[e] = orow[2 * P * l + e];
        }
        unsigned go[P][4];
        float gw[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            // position: one fma and one subtraction (align_corners=False); the comparisons are false for NaN and for +-inf
            const float px = __fmaf_rn(rx, Wf, dxy[2 * p]) - 0.5f;
            const float py = __fmaf_rn(ry, Hf, dxy[2 * p + 1]) - 0.5f;
            const bool in = py > -1.f && py < Hf && px > -1.f && px < Wf;
            const float qx = in ? px : 0.f, qy = in ? py : 0.f;
            const float fx = floorf(qx), fy = floorf(qy);
            const float lx = qx - fx, ly = qy - fy, hx = 1.f - lx, hy = 1.f - ly;
            const int x0 = (int)fx, y0 = (int)fy;                       // in [-1, W - 1] x [-1, H - 1]
            const bool x0ok = in && x0 >= 0, x1ok = in && x0 + 1 < Wl;
            const bool y0ok = y0 >= 0, y1ok = y0 + 1 < Hl;
            const unsigned b0 = (unsigned)((row0 + (long long)y0 * Wl + x0) * a.value_ld * 4) + seg_b;
            go[p][0] = y0ok && x0ok ? b0 : MS_OOB;
            go[p][1] = y0ok && x1ok ? b0 + px_b : MS_OOB;
            go[p][2] = y1ok && x0ok ? b0 + row_b : MS_OOB;
            go[p][3] = y1ok && x1ok ? b0 + row_b + px_b : MS_OOB;
            const float aw = in ? wl[p] : wl[p] * 0.f;   // a NaN weight stays a NaN
            gw[p][0] = aw * (hy * hx);
            gw[p][1] = aw * (hy * lx);
            gw[p][2] = aw * (ly * hx);
            gw[p][3] = aw * (ly * lx);
        }
        ms_f32x4 v[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                auto ld = __builtin_amdgcn_raw_buffer_load_b128(vrsrc, (int)go[p][c], 0, 0);
                v[p][c] = *reinterpret_cast<ms_f32x4 *>(&ld);
            }
        __builtin_amdgcn_sched_barrier(0);   // all 4 P loads are issued before the first fma waits: left alone hipcc keeps 3 in flight
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(v[p][c][e], gw[p][c], acc[e]);
    }
    *reinterpret_cast<ms_f32x4 *>(a.out + r * a.out_ld + h * D + c4 * 4) = acc;
}

template <int LPS, int L>
static void srf_msda_launch_p(int P, unsigned grid, hipStream_t st, const MsdaArgs &a)
{
    switch (P) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_fwd_k<LPS, L, 1>), dim3(grid), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_fwd_k<LPS, L, 2>), dim3(grid), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_fwd_k<LPS, L, 3>), dim3(grid), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_msda_fwd_k<LPS, L, 4>), dim3(grid), dim3(256), 0, st, a); break;
    }
}

template <int LPS>
static void srf_msda_launch(int L, int P, unsigned grid, hipStream_t st, const MsdaArgs &a)
{
    switch (L) {
    case 1: srf_msda_launch_p<LPS, 1>(P, grid, st, a); break;
    case 2: srf_msda_launch_p<LPS, 2>(P, grid, st, a); break;
    case 3: srf_msda_launch_p<LPS, 3>(P, grid, st, a); break;
    default: srf_msda_launch_p<LPS, 4>(P, grid, st, a); break;
    }
}

extern "C" int srf_msda_fwd(const float *value, long long value_ld, int B, const int *shapes, int L, const float *ref, const float *offs,
                            long long offs_ld, const float *logits, long long logits_ld, int Q, int heads, int head_dim, int P, float *out,
                            long long out_ld, srf_stream_t stream)
{
    if (B < 0 || Q < 0 || L <= 0 || P <= 0 || heads <= 0 || head_dim <= 0 || !shapes) return SRF_EINVAL;
    if (L > MS_MAXL || P > 4 || (head_dim != 16 && head_dim != 32)) return SRF_EUNSUPPORTED;
    const long long C = (long long)heads * head_dim, NS = (long long)heads * L * P;
    if (value_ld < C || out_ld < C || offs_ld < 2 * NS || logits_ld < NS) return SRF_EINVAL;
    MsdaArgs a;
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
    for (int l = L; l < MS_MAXL; ++l) a.H[l] = a.W[l] = a.start[l] = 0;
    const long long rows = (long long)B * Q, lim = 1ll << 31;
    // each tensor below 2 GiB: the value table is read through one buffer descriptor, the others are indexed in 32-bit-safe ranges
    auto fits = [lim](long long n, long long ld) { return n <= (lim / 4 - 1) / ld; };   // n ld floats stay below 2 GiB
    if (!fits((long long)B * S, value_ld) || !fits(rows, offs_ld) || !fits(rows, logits_ld) || !fits(rows, out_ld) || !fits(rows, 2 * L))
        return SRF_EUNSUPPORTED;
    if (rows == 0) return SRF_OK;
    if (!value || !ref || !offs || !logits || !out) return SRF_EINVAL;
    if ((value_ld & 3) || (offs_ld & 3) || (logits_ld & 3) || (out_ld & 3)) return SRF_EUNSUPPORTED;
    if (((uintptr_t)value & 15) || ((uintptr_t)ref & 15) || ((uintptr_t)offs & 15) || ((uintptr_t)logits & 15) || ((uintptr_t)out & 15))
        return SRF_EUNSUPPORTED;
    a.value = value;
    a.ref = ref;
    a.offs = offs;
    a.logits = logits;
    a.out = out;
    a.value_ld = value_ld;
    a.offs_ld = offs_ld;
    a.logits_ld = logits_ld;
    a.out_ld = out_ld;
    a.items = rows * heads;
    a.value_bytes = (long long)B * S * value_ld * 4;
    a.Q = Q;
    a.S = (int)S;
    a.heads = heads;
    const int lps = head_dim / 4;
    const long long nblk = (a.items * lps + 255) / 256;
    const long long per_xcd = (nblk + 7) / 8;
    if (per_xcd * 8 >= lim) return SRF_EUNSUPPORTED;
    a.per_xcd = (unsigned)per_xcd;
    if (lps == 4)
        srf_msda_launch<4>(L, P, (unsigned)(per_xcd * 8), (hipStream_t)stream, a);
    else
        srf_msda_launch<8>(L, P, (unsigned)(per_xcd * 8), (hipStream_t)stream, a);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
