// pillar.hip -- the encoder of the pillar configs for gfx950: the single-layer, mode="max" pillar feature net in one launch
// (srf_pillar_vfe) and PointPillarsScatter writing its canvas channels-last (srf_pillar_scatter_nhwc).
//
// Reference: mmdet3d_plugin/models/voxel_encoders/pillar_encoder_custom.py:108-161 (PillarFeatureNetCustom.forward), utils.py:63-146
// (PFNLayer) and mmdet3d's PointPillarsScatter; srfdet3d_amd/plugin/pillar.py restates them op by op in torch.
//
// DEFINITION of srf_pillar_vfe (tests/pillar_ref.py is the same text in numpy).  For pillar r with n = min(num[r], P) points, all
// arithmetic in f32, fl() = one rounding to nearest:
//   cluster mean    mean_d = fl(s_d / fl(n)), s_d the sum of coordinate d over the points 0..n-1 in ascending order
//   voxel centre    c_x = fl(fl(fl(x_idx) * vx) + off_x), likewise y and z: a product and a sum, two roundings, never an fma
//   decorated point (K = nf + 3 * cluster + 3 * centre values, k ascending)
//                   [the nf raw features, xyz replaced by xyz - c when legacy (and centre)], then xyz - mean, then xyz - c;
//                   every difference is one f32 subtraction of the raw coordinate
//   point p < n, channel c
//                   acc = fma chain over k ascending, starting from 0:  acc = fma(x_k, W[c][k], acc)
//                   v   = fma(acc, scale_c, shift_c);  v = v < 0 ? 0 : v          (a NaN stays a NaN, as F.relu)
//   out[r][c]       = max over p < n of v, and, when n < P, also over relu(shift_c): the reference masks the padded slots to zero BEFORE
//                   the linear layer, so each contributes relu(bn(0)); a pillar whose real activations all lie below a positive shift
//                   returns the shift.  The max propagates NaN (torch.max).
//   padding rows    (r >= *rows_dev, or b < 0, or n <= 0) write zeros.  The torch route divides 0 by 0 there; nothing downstream reads them.
// Fixed order, no atomics: two launches give the same bits.
//
// SHAPE of the kernel.  lane = output channel (a wave covers 64 channels; Cout / 64 channel groups are separate work items), the K
// weights, scale and shift of the lane in registers.  A work item is SRF_PV_G = 4 consecutive pillars of one channel group: the wave reads
// their counts and coordinates (lanes 0..3), then the LIVE points of all four (n * nf contiguous floats each, the first 128 floats of
// every pillar in flight together -- 20 x 5 fits), parks them in its own LDS slabs and reads them back as broadcasts (every lane the
// same address: conflict-free).  The trip count over points is the pillar's own n: work ~ sum(num), not rows * P.  No block-level
// barrier: a slab belongs to one wave, whose LDS operations execute in order.
// It is memory-sized (rows * (n_mean * nf + Cout) * 4 bytes against a few hundred thousand FMAs per CU), so no MFMA.
#include "common.hpp"

#define SRF_PV_G 4          // pillars of a work item
#define SRF_PV_WAVES 4      // waves of a workgroup
#define SRF_PV_MAX_BLOCKS 2048

struct PillarVfeArgs {
    const float *voxels;
    const int *num;
    const int *coors;   // (rows, 4) (b, z, y, x)
    const int *rows_dev;
    int rows, P, Cout, ncg;
    float vx, vy, vz, ox, oy, oz;
    int cluster, centre, legacy;
    const float *W, *scale, *shift;
    float *out;
    int slab;      // floats of one LDS slab (P * nf)
    int items;     // ceil(rows / G) * ncg
};

template <int NF>
__global__ __launch_bounds__(SRF_PV_WAVES * 64) void srf_pillar_vfe_k(PillarVfeArgs a)
{
    extern __shared__ float s_pts[];   // [wave][g][slab]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *slab0 = s_pts + (size_t)wave * SRF_PV_G * a.slab;
    const int K = NF + 3 * a.cluster + 3 * a.centre;
    const int rows_live = a.rows_dev ? min(*a.rows_dev, a.rows) : a.rows;
    const int pn = a.P * NF;
    const bool legacy = a.legacy && a.centre;

    // the lane's weights; a channel group is fixed per work item, and items of one wave may differ in it, so they are reloaded when it changes
    float w[NF], wm[3] = {0.f, 0.f, 0.f}, wc[3] = {0.f, 0.f, 0.f}, sc = 0.f, sh = 0.f;
    int cg_held = -1;

    const int wave_global = blockIdx.x * SRF_PV_WAVES + wave, wave_stride = gridDim.x * SRF_PV_WAVES;
    for (int item = wave_global; item < a.items; item += wave_stride) {   // wave-uniform
        const int cg = item % a.ncg, r0 = (item / a.ncg) * SRF_PV_G;
        const int c = cg * 64 + lane;
        if (cg != cg_held) {
            const float *wr = a.W + (size_t)c * K;
#pragma unroll
            for (int k = 0; k < NF; ++k) w[k] = wr[k];
            if (a.cluster) {
#pragma unroll
                for (int d = 0; d < 3; ++d) wm[d] = wr[NF + d];
            }
            if (a.centre) {
#pragma unroll
                for (int d = 0; d < 3; ++d) wc[d] = wr[NF + 3 * a.cluster + d];
            }
            sc = a.scale[c];
            sh = a.shift[c];
            cg_held = cg;
        }

        // counts and coordinates of the G pillars: lanes 0..G-1 read, everyone gets them as wave-uniform values
        int my_n = 0;
        int4 my_c = make_int4(-1, 0, 0, 0);
        if (lane < SRF_PV_G && r0 + lane < rows_live) {
            my_n = a.num[r0 + lane];
            const int *cr = a.coors + (size_t)(r0 + lane) * 4;
            my_c = make_int4(cr[0], cr[1], cr[2], cr[3]);
        }
        int n[SRF_PV_G], ix[SRF_PV_G], iy[SRF_PV_G], iz[SRF_PV_G];
#pragma unroll
        for (int g = 0; g < SRF_PV_G; ++g) {
            const int ng = __builtin_amdgcn_readlane(my_n, g), bg = __builtin_amdgcn_readlane(my_c.x, g);
            iz[g] = __builtin_amdgcn_readlane(my_c.y, g);
            iy[g] = __builtin_amdgcn_readlane(my_c.z, g);
            ix[g] = __builtin_amdgcn_readlane(my_c.w, g);
            n[g] = (bg < 0 || ng <= 0) ? 0 : min(ng, a.P);
        }

        // the live points: the first 128 floats of every pillar in flight together, the rest (n * nf > 128) pillar by pillar
        float t0[SRF_PV_G], t1[SRF_PV_G];
#pragma unroll
        for (int g = 0; g < SRF_PV_G; ++g) {
            const int cnt = n[g] * NF;
            const float *src = a.voxels + (size_t)(r0 + g) * pn;
            t0[g] = lane < cnt ? src[lane] : 0.f;
            t1[g] = 64 + lane < cnt ? src[64 + lane] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < SRF_PV_G; ++g) {
            const int cnt = n[g] * NF;
            float *slab = slab0 + g * a.slab;
            if (lane < cnt) slab[lane] = t0[g];
            if (64 + lane < cnt) slab[64 + lane] = t1[g];
            const float *src = a.voxels + (size_t)(r0 + g) * pn;
            for (int i = 128 + lane; i < cnt; i += 64) slab[i] = src[i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

#pragma unroll
        for (int g = 0; g < SRF_PV_G; ++g) {
            const int r = r0 + g;
            if (r >= a.rows) break;   // wave-uniform
            const int ng = n[g];
            const float *slab = slab0 + g * a.slab;
            float res = 0.f;          // padding rows
            if (ng > 0) {
                float mx = 0.f, my = 0.f, mz = 0.f;
                if (a.cluster) {
                    float sx = 0.f, sy = 0.f, sz = 0.f;
                    for (int p = 0; p < ng; ++p) {
                        sx = __fadd_rn(sx, slab[p * NF + 0]);
                        sy = __fadd_rn(sy, slab[p * NF + 1]);
                        sz = __fadd_rn(sz, slab[p * NF + 2]);
                    }
                    const float fn = (float)ng;
                    mx = __fdiv_rn(sx, fn);
                    my = __fdiv_rn(sy, fn);
                    mz = __fdiv_rn(sz, fn);
                }
                const float cx = __fadd_rn(__fmul_rn((float)ix[g], a.vx), a.ox);
                const float cy = __fadd_rn(__fmul_rn((float)iy[g], a.vy), a.oy);
                const float cz = __fadd_rn(__fmul_rn((float)iz[g], a.vz), a.oz);
                float best;
                if (ng < a.P)
                    best = sh < 0.f ? 0.f : sh;   // the padded slots: relu(bn(0))
                else
                    best = -INFINITY;
                for (int p = 0; p < ng; ++p) {
                    float x[NF];
#pragma unroll
                    for (int k = 0; k < NF; ++k) x[k] = slab[p * NF + k];
                    const float dx = __fsub_rn(x[0], cx), dy = __fsub_rn(x[1], cy), dz = __fsub_rn(x[2], cz);
                    float acc = 0.f;
                    acc = fmaf(legacy ? dx : x[0], w[0], acc);
                    acc = fmaf(legacy ? dy : x[1], w[1], acc);
                    acc = fmaf(legacy ? dz : x[2], w[2], acc);
#pragma unroll
                    for (int k = 3; k < NF; ++k) acc = fmaf(x[k], w[k], acc);
                    if (a.cluster) {
                        acc = fmaf(__fsub_rn(x[0], mx), wm[0], acc);
                        acc = fmaf(__fsub_rn(x[1], my), wm[1], acc);
                        acc = fmaf(__fsub_rn(x[2], mz), wm[2], acc);
                    }
                    if (a.centre) {
                        acc = fmaf(dx, wc[0], acc);
                        acc = fmaf(dy, wc[1], acc);
                        acc = fmaf(dz, wc[2], acc);
                    }
                    float v = fmaf(acc, sc, sh);
                    v = v < 0.f ? 0.f : v;
                    best = (v > best || v != v) ? v : best;   // a NaN enters and then stays: NaN compares false both ways
                }
                res = best;
            }
            a.out[(size_t)r * a.Cout + c] = res;
        }
        // the next item's slab writes must not overtake this item's reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// a tensor of a * b * c * d floats inside a 32-bit byte range (below 2^31 bytes); the factors are positive ints
static bool srf_fits_i32_bytes(long long a, long long b = 1, long long c = 1, long long d = 1)
{
    const long long lim = (1ll << 31) / 4;
    long long e = a;
    if (e >= lim) return false;
    e *= b;
    if (e >= lim) return false;
    e *= c;
    if (e >= lim) return false;
    e *= d;
    return e < lim;
}

extern "C" int srf_pillar_vfe(const float *voxels, const int *num, const int *coors4, const int *rows_dev, int rows, int P, int nf,
                              const float *voxel_size, const float *offset, int cluster_center, int voxel_center, int legacy,
                              const float *W, const float *scale, const float *shift, int Cout, float *out, srf_stream_t stream)
{
    if (rows < 0 || P <= 0 || nf <= 0 || Cout <= 0 || !voxel_size || !offset) return SRF_EINVAL;
    if (Cout % 64 != 0 || Cout > 256 || nf < 3 || nf > 8 || P > 64 || !srf_fits_i32_bytes(rows, P, nf) || !srf_fits_i32_bytes(rows, Cout))
        return SRF_EUNSUPPORTED;
    if (rows == 0) return SRF_OK;
    if (!voxels || !num || !coors4 || !W || !scale || !shift || !out) return SRF_EINVAL;

    PillarVfeArgs a;
    a.voxels = voxels;
    a.num = num;
    a.coors = coors4;
    a.rows_dev = rows_dev;
    a.rows = rows;
    a.P = P;
    a.Cout = Cout;
    a.ncg = Cout / 64;
    a.vx = voxel_size[0], a.vy = voxel_size[1], a.vz = voxel_size[2];
    a.ox = offset[0], a.oy = offset[1], a.oz = offset[2];
    a.cluster = cluster_center != 0;
    a.centre = voxel_center != 0;
    a.legacy = legacy != 0;
    a.W = W, a.scale = scale, a.shift = shift;
    a.out = out;
    a.slab = P * nf;
    a.items = srf_ceil_div(rows, SRF_PV_G) * a.ncg;
    int blocks = srf_ceil_div(a.items, SRF_PV_WAVES);
    if (blocks > SRF_PV_MAX_BLOCKS) blocks = SRF_PV_MAX_BLOCKS;
    const size_t lds = (size_t)SRF_PV_WAVES * SRF_PV_G * a.slab * sizeof(float);   // <= 4 * 4 * 512 * 4 = 32 KB
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks), block(SRF_PV_WAVES * 64);
    switch (nf) {
    case 3: hipLaunchKernelGGL(srf_pillar_vfe_k<3>, grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL(srf_pillar_vfe_k<4>, grid, block, lds, st, a); break;
    case 5: hipLaunchKernelGGL(srf_pillar_vfe_k<5>, grid, block, lds, st, a); break;
    case 6: hipLaunchKernelGGL(srf_pillar_vfe_k<6>, grid, block, lds, st, a); break;
    case 7: hipLaunchKernelGGL(srf_pillar_vfe_k<7>, grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(srf_pillar_vfe_k<8>, grid, block, lds, st, a); break;
    }
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// srf_pillar_scatter_nhwc: PointPillarsScatter with a channels-last canvas.  out (B, H, W, C) is zero-filled with 16-byte stores, then
// row r of feats goes to pixel (b, y, x) of coors4[r] as C / 4 whole float4s (a pillar's 256 bytes are one contiguous run; the NCHW
// canvas took 64 strided dwords).  The z column is ignored.  Rows with b < 0 or r >= *rows_dev are skipped, as srf_densify skips them;
// so are rows whose (b, y, x) lies outside the canvas.  Coordinates are DISTINCT by construction (one pillar per occupied cell: the
// voxelization emits each cell once), so no two rows write the same pixel and the result does not depend on any order.  A bit copy.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srf_pillar_zero_k(uint4 *__restrict__ p, size_t nquads)
{
    const size_t stride = (size_t)gridDim.x * 256;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nquads; i += stride) p[i] = z;
}

__global__ __launch_bounds__(256) void srf_pillar_scatter_k(const uint4 *__restrict__ feats, const int *__restrict__ coors,
                                                          const int *__restrict__ rows_dev, int rows, int Q, int B, int H, int W,
                                                          uint4 *__restrict__ out)
{
    const int live = rows_dev ? min(*rows_dev, rows) : rows;
    const long long total = (long long)live * Q, stride = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const int r = (int)(t / Q), q = (int)(t % Q);
        const int b = coors[(size_t)r * 4], y = coors[(size_t)r * 4 + 2], x = coors[(size_t)r * 4 + 3];
        if (b < 0 || b >= B || y < 0 || y >= H || x < 0 || x >= W) continue;
        out[(((size_t)b * H + y) * W + x) * Q + q] = feats[t];
    }
}

extern "C" int srf_pillar_scatter_nhwc(const float *feats, const int *coors4, const int *rows_dev, int rows, int C, int B, int H, int W,
                                       float *out, srf_stream_t stream)
{
    if (rows < 0 || C <= 0 || B <= 0 || H <= 0 || W <= 0) return SRF_EINVAL;
    if (C % 4 != 0 || !srf_fits_i32_bytes(rows, C) || !srf_fits_i32_bytes(B, H, W, C)) return SRF_EUNSUPPORTED;
    if (!out || (rows > 0 && (!feats || !coors4))) return SRF_EINVAL;
    if (((uintptr_t)out & 15) || ((uintptr_t)feats & 15)) return SRF_EINVAL;   // whole float4s
    hipStream_t st = (hipStream_t)stream;
    const int Q = C / 4;
    const size_t nquads = (size_t)B * H * W * Q;
    size_t zb = (nquads + 255) / 256;
    hipLaunchKernelGGL(srf_pillar_zero_k, dim3((unsigned)(zb > 4096 ? 4096 : zb)), dim3(256), 0, st, (uint4 *)out, nquads);
    if (rows > 0) {
        const long long sb = ((long long)rows * Q + 255) / 256;
        hipLaunchKernelGGL(srf_pillar_scatter_k, dim3((unsigned)(sb > 4096 ? 4096 : sb)), dim3(256), 0, st, (const uint4 *)feats,
                           coors4, rows_dev, rows, Q, B, H, W, (uint4 *)out);
    }
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
