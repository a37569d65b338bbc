// dvfe.hip -- the encoder of the dynamic-voxelization configs for gfx950: DynamicVFECustom.forward in eval mode (cluster centre through
// the centroid-aware position encoder, voxel centre, one or two VFE layers, mode="max") in two launches behind the voxel map.
//
// Reference: mmdet3d_plugin/models/voxel_encoders/voxel_encoder.py:162-240 (DynamicVFECustom.forward), utils.py:8-45 (DynamicVFELayer);
// srfdet3d_amd/plugin/voxel_encoders.py restates them op by op in torch.
//
// DEFINITION of srf_dvfe_fwd (tests/dvfe_ref.py is the same text in numpy).  fl() = one rounding to nearest in f32.  A point i with
// m = point2voxel[i] < 0 belongs to no voxel and touches nothing.  For the others, with L(m) the point list of voxel m in ascending order:
//   cluster mean     mean_d(m) = fl(s_d / fl(|L|)), s_d the __fadd_rn sum of coordinate d over L(m) in that order, starting from 0
//                    (what srf_scatter_reduce_k mode 0 gives)
//   voxel centre     c_x(m) = fl(fl(fl(x_idx) * vx) + off_x), likewise y and z: a product and a sum, two roundings, never an fma
//   decoration       rel = fl(xyz - mean), cen = fl(xyz - c): one f32 subtraction each
//   position encoder h   = tanh(fma(W1 . rel, scale1, shift1))                         (d values)
//                    pos = tanh(fma(W2 . h,   scale2, shift2))                         (d values)
//   layer 0          x  = [the nf raw features | pos | cen (when voxel_center)],  p0 = relu(fma(Wa . x, scale_a, shift_a))   (C0 values)
//                    v0(m) = max of p0 over L(m)
//   layer 1 (C1 > 0) p1 = relu(fma(Wb . [p0 | v0(m)], scale_b, shift_b)),  out(m) = max of p1 over L(m);   C1 == 0: out = v0
//   relu             v < 0 ? 0 : v: a NaN stays a NaN (torch.relu)
//   max              srf_scatter_reduce_k mode 1: start at -inf, take v only if v > acc: a NaN is never taken
//   padding rows     m >= min(*num_voxels, rows) are written as zeros
// The decoration is pinned bit for bit; the dot products are f32 fma chains in a fixed order, held to the float64 network on that decoration
// within the running bound tests/dvfe_ref.py carries along.  No atomics, fixed order: two launches give the same bytes.
//
// SHAPE.  srf_dvfe_point_k, one thread per point: its features, a walk over its voxel's list for the mean, the position encoder and layer 0
// out of registers, p0 (n, C0) to the workspace.  h_i is produced one at a time in a rolled loop and spread over the d running sums of the
// second layer (d registers, d independent fma chains); the sums are parked in the thread's own LDS column so that the loop that takes
// their tanh and folds pos_j into the CP accumulators of layer 0 is rolled too: two tanh bodies in the code instead of 2 d, and no run of
// d x CP hoisted weight reads (the fully unrolled forms took 128 registers and 140-4300 bytes of scratch at d = 64).
// All weights (< 24 KB) are put into LDS once per workgroup and read at wave-uniform addresses: every read is a broadcast.  W2 is held
// transposed ([i][j]) and the layer-0 operand k-major ([k][CP], raw features padded to 8 slots, channels padded to CP in {4, 8, 16} with
// zero weights), so that what one step needs is a run of 16-byte reads.
// srf_dvfe_voxel_k, one thread per voxel: the max over p0, for two layers the voxel's half of Wb once, then per point the p0 half, the
// epilogue and the max; zero rows behind the live count.  The only per-point intermediate in global memory is p0.
// The arithmetic is ~1300 fma and 2 d tanh per point (0.25 GFLOP on a 180 000-point sweep): the launches and p0's 2 x n x C0 x 4 bytes are
// what it costs, so no MFMA.
#include "common.hpp"

#define SRF_DV_THREADS 256
#define SRF_DV_RAW 8     // raw-feature slots of the layer-0 operand (nf <= 8)

struct DvfeArgs {
    const float *points;
    const int *p2v, *order, *offsets, *counts, *num_voxels, *vcoors;
    int n, nf, rows;
    float vx, vy, vz, ox, oy, oz;
    int centre;
    const float *W1, *s1, *h1, *W2, *s2, *h2;
    const float *Wa, *sa, *ha;
    const float *Wb, *sb, *hb;
    int C0, C1;
    float *p0, *out;
};

// the list of voxel m, or an empty one if it does not lie inside order[0..n)
__device__ __forceinline__ void srf_dv_list(const DvfeArgs &a, int m, int &off, int &cnt)
{
    off = a.offsets[m];
    cnt = a.counts[m];
    if (off < 0 || cnt < 0 || (long long)off + cnt > a.n) cnt = 0;
}

template <int D, int CP>
__global__ __launch_bounds__(SRF_DV_THREADS) void srf_dvfe_point_k(DvfeArgs a)
{
    constexpr int KA = SRF_DV_RAW + D + 3;   // slots of the layer-0 operand: raw | pos | centre
    __shared__ __attribute__((aligned(16))) float s_w2t[D * D];   // [i][j] = W2[j][i]
    __shared__ __attribute__((aligned(16))) float s_wa[KA * CP];
    __shared__ __attribute__((aligned(16))) float s_w1[D * 4];   // [j]: W1[j][0..2], unused
    __shared__ float s_s1[D], s_h1[D], s_s2[D], s_h2[D], s_sa[CP], s_ha[CP];
    __shared__ float s_z[D * SRF_DV_THREADS];   // [j][thread]: the second layer's sums, each thread its own column

    const int tid = threadIdx.x;
    for (int t = tid; t < D * D; t += SRF_DV_THREADS) s_w2t[(t % D) * D + t / D] = a.W2[t];
    for (int t = tid; t < D * 4; t += SRF_DV_THREADS) s_w1[t] = (t & 3) < 3 ? a.W1[(t >> 2) * 3 + (t & 3)] : 0.f;
    for (int t = tid; t < D; t += SRF_DV_THREADS) {
        s_s1[t] = a.s1[t];
        s_h1[t] = a.h1[t];
        s_s2[t] = a.s2[t];
        s_h2[t] = a.h2[t];
    }
    const int kin = a.nf + D + 3 * a.centre;   // row length of Wa
    for (int t = tid; t < KA * CP; t += SRF_DV_THREADS) {
        const int k = t / CP, c = t % CP;
        int col;
        if (k < SRF_DV_RAW)
            col = k < a.nf ? k : -1;
        else if (k < SRF_DV_RAW + D)
            col = a.nf + (k - SRF_DV_RAW);
        else
            col = a.centre ? a.nf + D + (k - SRF_DV_RAW - D) : -1;
        s_wa[t] = (c < a.C0 && col >= 0) ? a.Wa[(size_t)c * kin + col] : 0.f;
    }
    for (int t = tid; t < CP; t += SRF_DV_THREADS) {
        s_sa[t] = t < a.C0 ? a.sa[t] : 0.f;
        s_ha[t] = t < a.C0 ? a.ha[t] : 0.f;
    }
    __syncthreads();

    const int i = blockIdx.x * SRF_DV_THREADS + tid;
    if (i >= a.n) return;
    const int live = min(*a.num_voxels, a.rows);
    const int m = a.p2v[i];
    if (m < 0 || m >= live) return;

    const float *pt = a.points + (size_t)i * a.nf;
    float x[SRF_DV_RAW];
#pragma unroll
    for (int k = 0; k < SRF_DV_RAW; ++k) x[k] = k < a.nf ? pt[k] : 0.f;

    // the cluster mean: the sequential f32 sum over the voxel's list in ascending point order
    int off, cnt;
    srf_dv_list(a, m, off, cnt);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int j = 0; j < cnt; ++j) {
        const int q = a.order[off + j];
        if ((unsigned)q >= (unsigned)a.n) continue;
        const float *pq = a.points + (size_t)q * a.nf;
        sx = __fadd_rn(sx, pq[0]);
        sy = __fadd_rn(sy, pq[1]);
        sz = __fadd_rn(sz, pq[2]);
    }
    const float fn = (float)cnt;
    const float rx = __fsub_rn(x[0], __fdiv_rn(sx, fn)), ry = __fsub_rn(x[1], __fdiv_rn(sy, fn)), rz = __fsub_rn(x[2], __fdiv_rn(sz, fn));

    // position encoder: h_i one at a time (a rolled loop, one tanh in the code), spread at once over the d sums of the second layer, each
    // of which so runs over i ascending
    float z2[D];
#pragma unroll
    for (int j = 0; j < D; ++j) z2[j] = 0.f;
#pragma unroll 1
    for (int i2 = 0; i2 < D; ++i2) {
        float acc = __fmul_rn(rx, s_w1[4 * i2]);
        acc = fmaf(ry, s_w1[4 * i2 + 1], acc);
        acc = fmaf(rz, s_w1[4 * i2 + 2], acc);
        const float hi = tanhf(fmaf(acc, s_s1[i2], s_h1[i2]));
        const float *w2 = s_w2t + i2 * D;
#pragma unroll
        for (int j = 0; j < D; ++j) z2[j] = fmaf(hi, w2[j], z2[j]);
    }

    // the d sums are parked in the thread's own LDS column so that the loop over them can be a rolled one as well (a second tanh in the
    // code, not d of them; a register array cannot be indexed by a loop counter)
#pragma unroll
    for (int j = 0; j < D; ++j) s_z[j * SRF_DV_THREADS + tid] = z2[j];

    // layer 0: the raw features, then every pos_j as its tanh comes out, then the centre offsets
    float acc0[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) acc0[c] = 0.f;
#pragma unroll
    for (int k = 0; k < SRF_DV_RAW; ++k) {
        if (k < a.nf) {   // wave-uniform
#pragma unroll
            for (int c = 0; c < CP; ++c) acc0[c] = fmaf(x[k], s_wa[k * CP + c], acc0[c]);
        }
    }
#pragma unroll 1
    for (int j = 0; j < D; ++j) {
        const float pj = tanhf(fmaf(s_z[j * SRF_DV_THREADS + tid], s_s2[j], s_h2[j]));
        const float *wa = s_wa + (SRF_DV_RAW + j) * CP;
#pragma unroll
        for (int c = 0; c < CP; ++c) acc0[c] = fmaf(pj, wa[c], acc0[c]);
    }
    if (a.centre) {
        const int *vc = a.vcoors + (size_t)m * 4;   // (b, z, y, x)
        const float dx = __fsub_rn(x[0], __fadd_rn(__fmul_rn((float)vc[3], a.vx), a.ox));
        const float dy = __fsub_rn(x[1], __fadd_rn(__fmul_rn((float)vc[2], a.vy), a.oy));
        const float dz = __fsub_rn(x[2], __fadd_rn(__fmul_rn((float)vc[1], a.vz), a.oz));
        const float *wa = s_wa + (SRF_DV_RAW + D) * CP;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            acc0[c] = fmaf(dx, wa[c], acc0[c]);
            acc0[c] = fmaf(dy, wa[CP + c], acc0[c]);
            acc0[c] = fmaf(dz, wa[2 * CP + c], acc0[c]);
        }
    }
    float *dst = a.p0 + (size_t)i * a.C0;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        if (c < a.C0) {
            const float v = fmaf(acc0[c], s_sa[c], s_ha[c]);
            dst[c] = v < 0.f ? 0.f : v;   // a NaN stays
        }
    }
}

// CP1 == 0: one layer, out = v0
template <int CP0, int CP1>
__global__ __launch_bounds__(SRF_DV_THREADS, 4) void srf_dvfe_voxel_k(DvfeArgs a)
{
    constexpr int NB = CP1 > 0 ? CP1 : 1;
    __shared__ __attribute__((aligned(16))) float s_wb[2 * CP0 * NB];   // [k][c1]: k < CP0 the p0 half, then the v0 half
    __shared__ float s_sb[NB], s_hb[NB];
    const int tid = threadIdx.x;
    if (CP1 > 0) {
        for (int t = tid; t < 2 * CP0 * NB; t += SRF_DV_THREADS) {
            const int k = t / NB, c = t % NB;
            const int kk = k < CP0 ? k : k - CP0;
            const int col = kk < a.C0 ? (k < CP0 ? kk : a.C0 + kk) : -1;
            s_wb[t] = (c < a.C1 && col >= 0) ? a.Wb[(size_t)c * 2 * a.C0 + col] : 0.f;
        }
        for (int t = tid; t < NB; t += SRF_DV_THREADS) {
            s_sb[t] = t < a.C1 ? a.sb[t] : 0.f;
            s_hb[t] = t < a.C1 ? a.hb[t] : 0.f;
        }
        __syncthreads();
    }
    const int m = blockIdx.x * SRF_DV_THREADS + tid;
    if (m >= a.rows) return;
    const int cl = CP1 > 0 ? a.C1 : a.C0;
    float *dst = a.out + (size_t)m * cl;
    if (m >= min(*a.num_voxels, a.rows)) {
        for (int c = 0; c < cl; ++c) dst[c] = 0.f;
        return;
    }
    int off, cnt;
    srf_dv_list(a, m, off, cnt);
    const int *lst = a.order + off;

    float v0[CP0];
#pragma unroll
    for (int c = 0; c < CP0; ++c) v0[c] = c < a.C0 ? -INFINITY : 0.f;   // the padded channels meet zero weights only
    for (int j = 0; j < cnt; ++j) {
        const int q = lst[j];
        if ((unsigned)q >= (unsigned)a.n) continue;
        const float *row = a.p0 + (size_t)q * a.C0;
#pragma unroll
        for (int c = 0; c < CP0; ++c) {
            if (c < a.C0) {
                const float v = row[c];
                v0[c] = v > v0[c] ? v : v0[c];
            }
        }
    }
    if (CP1 == 0) {
#pragma unroll
        for (int c = 0; c < CP0; ++c)
            if (c < a.C0) dst[c] = v0[c];
        return;
    }

    // the voxel's half of Wb . [p0 | v0], once
    float t1[NB], v1[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        t1[c] = 0.f;
        v1[c] = -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < CP0; ++k) {
        if (k < a.C0) {
#pragma unroll
            for (int c = 0; c < NB; ++c) t1[c] = fmaf(v0[k], s_wb[(CP0 + k) * NB + c], t1[c]);
        }
    }
    for (int j = 0; j < cnt; ++j) {
        const int q = lst[j];
        if ((unsigned)q >= (unsigned)a.n) continue;
        const float *row = a.p0 + (size_t)q * a.C0;
        float acc[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) acc[c] = t1[c];
#pragma unroll 1
        for (int k = 0; k < a.C0; ++k) {   // rolled: the weights stay in LDS, a row of NB per step
            const float pk = row[k];
#pragma unroll
            for (int c = 0; c < NB; ++c) acc[c] = fmaf(pk, s_wb[k * NB + c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            float v = fmaf(acc[c], s_sb[c], s_hb[c]);
            v = v < 0.f ? 0.f : v;
            v1[c] = v > v1[c] ? v : v1[c];
        }
    }
#pragma unroll
    for (int c = 0; c < NB; ++c)
        if (c < a.C1) dst[c] = v1[c];
}

// a tensor of a * b floats below 2^31 bytes; the factors are non-negative ints
static bool srf_dv_fits(long long a, long long b) { return a * b < (1ll << 31) / 4; }

static int srf_dv_pad(int c) { return c <= 4 ? 4 : c <= 8 ? 8 : 16; }

extern "C" size_t srf_dvfe_workspace_bytes(int n, int C0)
{
    if (n <= 0 || C0 <= 0) return 0;
    return srf_align256((size_t)n * (size_t)C0 * sizeof(float));
}

template <int D>
static void srf_dv_launch_point(const DvfeArgs &a, hipStream_t st)
{
    const dim3 grid(srf_ceil_div(a.n, SRF_DV_THREADS)), block(SRF_DV_THREADS);
    switch (srf_dv_pad(a.C0)) {
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_point_k<D, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_point_k<D, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_point_k<D, 16>), grid, block, 0, st, a); break;
    }
}

template <int CP0>
static void srf_dv_launch_voxel(const DvfeArgs &a, hipStream_t st)
{
    const dim3 grid(srf_ceil_div(a.rows, SRF_DV_THREADS)), block(SRF_DV_THREADS);
    switch (a.C1 > 0 ? srf_dv_pad(a.C1) : 0) {
    case 0: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_voxel_k<CP0, 0>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_voxel_k<CP0, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_voxel_k<CP0, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_dvfe_voxel_k<CP0, 16>), grid, block, 0, st, a); break;
    }
}

extern "C" int srf_dvfe_fwd(const float *points, int n, int nf, const int *point2voxel, const int *order, const int *offsets,
                            const int *counts, const int *num_voxels, const int *voxel_coors, int rows, const float *voxel_size,
                            const float *offset, int voxel_center, const float *W1, const float *scale1, const float *shift1,
                            const float *W2, const float *scale2, const float *shift2, int d, const float *Wa, const float *scale_a,
                            const float *shift_a, int C0, const float *Wb, const float *scale_b, const float *shift_b, int C1, float *out,
                            void *workspace, size_t workspace_bytes, srf_stream_t stream)
{
    if (n < 0 || rows < 0 || nf <= 0 || d <= 0 || C0 <= 0 || C1 < 0) return SRF_EINVAL;
    if (n == 0 || rows == 0) return SRF_OK;
    if (!points || !point2voxel || !order || !offsets || !counts || !num_voxels || !voxel_coors || !voxel_size || !offset || !W1 ||
        !scale1 || !shift1 || !W2 || !scale2 || !shift2 || !Wa || !scale_a || !shift_a || !out || !workspace)
        return SRF_EINVAL;
    if (C1 > 0 && (!Wb || !scale_b || !shift_b)) return SRF_EINVAL;
    if (nf < 3 || nf > SRF_DV_RAW || (d != 16 && d != 32 && d != 64) || C0 > 16 || C1 > 16 || !srf_dv_fits(n, nf) || !srf_dv_fits(n, C0) ||
        !srf_dv_fits(rows, C1 > 0 ? C1 : C0))
        return SRF_EUNSUPPORTED;
    if (workspace_bytes < srf_dvfe_workspace_bytes(n, C0)) return SRF_EWORKSPACE;

    DvfeArgs a;
    a.points = points;
    a.p2v = point2voxel, a.order = order, a.offsets = offsets, a.counts = counts, a.num_voxels = num_voxels, a.vcoors = voxel_coors;
    a.n = n, a.nf = nf, a.rows = rows;
    a.vx = voxel_size[0], a.vy = voxel_size[1], a.vz = voxel_size[2];
    a.ox = offset[0], a.oy = offset[1], a.oz = offset[2];
    a.centre = voxel_center != 0;
    a.W1 = W1, a.s1 = scale1, a.h1 = shift1, a.W2 = W2, a.s2 = scale2, a.h2 = shift2;
    a.Wa = Wa, a.sa = scale_a, a.ha = shift_a;
    a.Wb = Wb, a.sb = scale_b, a.hb = shift_b;
    a.C0 = C0, a.C1 = C1;
    a.p0 = (float *)workspace;
    a.out = out;
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
    case 16: srf_dv_launch_point<16>(a, st); break;
    case 32: srf_dv_launch_point<32>(a, st); break;
    default: srf_dv_launch_point<64>(a, st); break;
    }
    switch (srf_dv_pad(C0)) {
    case 4: srf_dv_launch_voxel<4>(a, st); break;
    case 8: srf_dv_launch_voxel<8>(a, st); break;
    default: srf_dv_launch_voxel<16>(a, st); break;
    }
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
