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
// msda_frame.hpp holds what the backward (msda_bwd.hip) must recompute exactly: the item decode, the softmax, the sample and its inside rule.
#include "msda_frame.hpp"

struct MsdaArgs : MsdaFrame {
    float *out;
    long long out_ld;
};

template <int LPS, int L, int P>
__global__ __launch_bounds__(256, 3) void srf_msda_fwd_k(MsdaArgs a)
{
    constexpr int D = LPS * 4, NS = L * P;
    int c4;
    const long long item = msda_item_index<LPS>(a.per_xcd, c4);
    if (item >= a.items) return;
    const MsdaItem it = msda_item(item, a.heads);
    const long long r = it.r;
    const int h = it.h;

    float w[NS];
    msda_softmax<L, P>(a.logits + r * a.logits_ld + h * NS, w);
    const int b = msda_batch(r, a.Q);   // here, behind the softmax: msda_frame.hpp says why

    __amdgpu_buffer_rsrc_t vrsrc = msda_value_rsrc(a.value, a.value_bytes);
    const float *orow = a.offs + r * a.offs_ld + h * (NS * 2);
    const float *rrow = a.ref + r * (L * 2);
    const unsigned seg_b = (unsigned)((h * D + c4 * 4) * 4);
    const unsigned px_b = (unsigned)(a.value_ld * 4);
    msda_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // a real loop over the levels: unrolled, hipcc hoists every level's loads to the top (256 VGPRs, one wave per SIMD, spills under a
    // tighter bound).  One level's 4 P loads are in flight per lane at a time; 130 VGPRs, three waves per SIMD, no scratch.
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        float wl[P], dxy[2 * P];
        msda_level_weights<L, P>(w, l, wl);
        const int Hl = a.H[l], Wl = a.W[l];
        const float rx = rrow[2 * l], ry = rrow[2 * l + 1];
        const unsigned row_b = (unsigned)Wl * px_b;
        const long long row0 = (long long)b * a.S + a.start[l];
        msda_level_offsets<P>(orow, l, dxy);
        unsigned go[P][4];
        float gw[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const MsdaSample s = msda_sample(rx, ry, dxy[2 * p], dxy[2 * p + 1], Hl, Wl, row0);
            const unsigned b0 = (unsigned)(s.row * a.value_ld * 4) + seg_b;
            go[p][0] = s.ok[0] ? b0 : MSDA_OOB;
            go[p][1] = s.ok[1] ? b0 + px_b : MSDA_OOB;
            go[p][2] = s.ok[2] ? b0 + row_b : MSDA_OOB;
            go[p][3] = s.ok[3] ? b0 + row_b + px_b : MSDA_OOB;
            const float aw = s.in ? wl[p] : wl[p] * 0.f;   // a NaN weight stays a NaN
#pragma unroll
            for (int c = 0; c < 4; ++c) gw[p][c] = aw * s.cw[c];
        }
        msda_f32x4 v[P][4];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                auto ld = __builtin_amdgcn_raw_buffer_load_b128(vrsrc, (int)go[p][c], 0, 0);
                v[p][c] = *reinterpret_cast<msda_f32x4 *>(&ld);
            }
        __builtin_amdgcn_sched_barrier(0);   // all 4 P loads are issued before the first fma waits: left alone hipcc keeps 3 in flight
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(v[p][c][e], gw[p][c], acc[e]);
    }
    *reinterpret_cast<msda_f32x4 *>(a.out + r * a.out_ld + h * D + c4 * 4) = acc;
}

struct MsdaFwdKernel {
    template <int D, int L, int P>
    static constexpr auto get() { return &srf_msda_fwd_k<D / 4, L, P>; }
};

extern "C" int srf_msda_fwd(const float *value, long long value_ld, int B, const int *shapes, int L, const float *ref, const float *offs,
                            long long offs_ld, const float *logits, long long logits_ld, int Q, int heads, int head_dim, int P, float *out,
                            long long out_ld, srf_stream_t stream)
{
    MsdaArgs a = {{}, out, out_ld};
    const MsdaTensor own[] = {{out, out_ld, MSDA_LIKE_OUT, false}};
    unsigned grid;
    const int rc = msda_frame_fill(a, value, value_ld, B, shapes, L, ref, offs, offs_ld, logits, logits_ld, Q, heads, head_dim, P, own, 1,
                                   false, head_dim / 4, grid);
    if (rc != SRF_OK || grid == 0) return rc;
    msda_launch<MsdaFwdKernel>(head_dim, L, P, grid, (hipStream_t)stream, a);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
