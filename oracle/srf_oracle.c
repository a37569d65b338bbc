/*
 * oracle/srf_oracle.c -- CPU restatement of the SRFDet3D hot-path operators.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in srfdet3d_amd/ (the product) may link, load or call
 * this file; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do, and
 * only as the checker / the reported CPU baseline.
 *
 * What it restates.  The reference (gopi-erabati/SRFDet3D) contains no native code; the
 * operators below are the ones its Python reaches in un-vendored third-party wheels
 * (mmcv-full 1.7.0, mmdet 2.28.2, mmdet3d 1.0.0rc6, spconv-cu117; README.md:54-60,
 * requirements.txt:1-5).  Each function cites the reference call site it serves and restates
 * the published algorithm of the third-party op.
 *
 * PARITY STATUS: "parity unpinned" for every function in this file.  The reference ships no
 * tests, golden vectors or fixtures, and none of the four wheels is installed or installable
 * here, so nothing pins these third-party boundaries.  They are checked against brute-force
 * numpy definitions (tests/test_oracle_*.py) and, where torch has the same op
 * (conv3d/batch-norm on a densified grid), against torch CPU.  The decoder-stage arithmetic,
 * which IS pinned by fixtures generated from the reference's own Python, lives in
 * oracle/decoder_oracle.py, not here.
 *
 * Numerics.  All arithmetic is IEEE binary32 with no contraction except where fmaf() is
 * written explicitly; compile with -ffp-contract=off (oracle/Makefile does).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORC_OK 0
#define ORC_EINVAL (-1)
#define ORC_ENOMEM (-2)
#define ORC_EOVERFLOW (-3)

/* ------------------------------------------------------------------------------------------
 * small open-addressing map int64 -> int32 (sequential; the oracle's stand-in for the dense
 * coor_to_voxelidx LUT of mmcv and the index grid of spconv 1.x)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int64_t *keys;
    int32_t *vals;
    uint64_t cap; /* power of two */
} orc_map;

static int map_init(orc_map *m, uint64_t n)
{
    uint64_t cap = 16;
    while (cap < 2 * n + 2) cap <<= 1;
    m->cap = cap;
    m->keys = (int64_t *)malloc(cap * sizeof(int64_t));
    m->vals = (int32_t *)malloc(cap * sizeof(int32_t));
    if (!m->keys || !m->vals) return ORC_ENOMEM;
    for (uint64_t i = 0; i < cap; ++i) m->keys[i] = -1;
    return ORC_OK;
}
static void map_free(orc_map *m)
{
    free(m->keys);
    free(m->vals);
}
static inline uint64_t map_hash(int64_t k) { return (uint64_t)k * 0x9E3779B97F4A7C15ull; }
static inline int32_t map_get(const orc_map *m, int64_t k)
{
    uint64_t h = map_hash(k) & (m->cap - 1);
    while (m->keys[h] != -1) {
        if (m->keys[h] == k) return m->vals[h];
        h = (h + 1) & (m->cap - 1);
    }
    return -1;
}
static inline void map_put(orc_map *m, int64_t k, int32_t v)
{
    uint64_t h = map_hash(k) & (m->cap - 1);
    while (m->keys[h] != -1 && m->keys[h] != k) h = (h + 1) & (m->cap - 1);
    m->keys[h] = k;
    m->vals[h] = v;
}

/* ------------------------------------------------------------------------------------------
 * K2  dynamic voxelization
 * reference call site: SRFDet.voxelize, dynamic branch, mmdet3d_plugin/models/detectors/srfdet.py:233-247
 * third-party op: mmcv.ops.Voxelization(max_num_points=-1) -> dynamic_voxelize_forward (CPU kernel
 * semantics): c_j = floor((p_j - range_j) / vs_j) in binary32, row is
 * (-1,-1,-1) when any c_j is outside [0, grid_j); stored reversed (z,y,x).
 * ---------------------------------------------------------------------------------------- */
static inline int voxel_coord(const float *p, const float *vs, const float *range, const int *grid, int *zyx)
{
    for (int j = 0; j < 3; ++j) {
        float d = p[j] - range[j];
        float q = d / vs[j];
        float f = floorf(q);
        if (!(f >= 0.0f && f < (float)grid[j])) return 0;
        zyx[2 - j] = (int)f;
    }
    return 1;
}

int orc_dynamic_voxelize(const float *points, int n, int nf, const float *vs, const float *range,
                         const int *grid, int *coors /* n x 3 (z,y,x) */)
{
    if (n < 0 || nf < 3) return ORC_EINVAL;
    for (int i = 0; i < n; ++i) {
        int c[3];
        if (voxel_coord(points + (size_t)i * nf, vs, range, grid, c)) {
            coors[3 * i] = c[0];
            coors[3 * i + 1] = c[1];
            coors[3 * i + 2] = c[2];
        } else {
            coors[3 * i] = coors[3 * i + 1] = coors[3 * i + 2] = -1;
        }
    }
    return ORC_OK;
}

/* ------------------------------------------------------------------------------------------
 * K1  hard voxelization
 * reference call site: SRFDet.voxelize, hard branch, srfdet.py:218-232 (module built at srfdet.py:58,
 * config configs/nus/srfdet_voxel_nusc_L.py:37-39).
 * third-party op: mmcv hard_voxelize_forward, CPU kernel / CUDA deterministic=True semantics
 * (SURVEY.md Appendix B.1): voxels numbered in first-seen point order, at most max_points points
 * per voxel in point order, at most max_voxels voxels (later new voxels are dropped, later points
 * of existing voxels are still added), unused slots zero.
 * ---------------------------------------------------------------------------------------- */
int orc_hard_voxelize(const float *points, int n, int nf, const float *vs, const float *range,
                      const int *grid, int max_points, int max_voxels, float *voxels /* max_voxels x max_points x nf */,
                      int *coors /* max_voxels x 3 */, int *num /* max_voxels */, int *voxel_num_out)
{
    if (n < 0 || nf < 3 || max_points <= 0 || max_voxels <= 0) return ORC_EINVAL;
    orc_map lut;
    if (map_init(&lut, (uint64_t)n)) return ORC_ENOMEM;
    memset(voxels, 0, sizeof(float) * (size_t)max_voxels * max_points * nf);
    memset(num, 0, sizeof(int) * (size_t)max_voxels);
    int M = 0;
    for (int i = 0; i < n; ++i) {
        int c[3];
        const float *p = points + (size_t)i * nf;
        if (!voxel_coord(p, vs, range, grid, c)) continue;
        int64_t key = ((int64_t)c[0] * grid[1] + c[1]) * grid[0] + c[2];
        int idx = map_get(&lut, key);
        if (idx == -1) {
            if (M >= max_voxels) continue;
            idx = M++;
            map_put(&lut, key, idx);
            coors[3 * idx] = c[0];
            coors[3 * idx + 1] = c[1];
            coors[3 * idx + 2] = c[2];
        }
        int k = num[idx];
        if (k < max_points) {
            memcpy(voxels + ((size_t)idx * max_points + k) * nf, p, sizeof(float) * nf);
            num[idx] = k + 1;
        }
    }
    *voxel_num_out = M;
    map_free(&lut);
    return ORC_OK;
}

/* ------------------------------------------------------------------------------------------
 * a3  HardSimpleVFE
 * reference: config configs/nus/srfdet_voxel_nusc_L.py:40 -> mmdet3d HardSimpleVFE (Appendix B.6):
 * voxels[:, :, :F].sum(1) / num.view(-1, 1).  Sum order is slot order 0..max_points-1.
 * ---------------------------------------------------------------------------------------- */
int orc_vfe_mean(const float *voxels, const int *num, int M, int max_points, int nf, int F, float *out)
{
    for (int m = 0; m < M; ++m)
        for (int c = 0; c < F; ++c) {
            float s = 0.0f;
            for (int k = 0; k < max_points; ++k) s = s + voxels[((size_t)m * max_points + k) * nf + c];
            out[(size_t)m * F + c] = s / (float)num[m];
        }
    return ORC_OK;
}

/* ------------------------------------------------------------------------------------------
 * K3  DynamicScatter (mean | max)
 * reference call sites: mmdet3d_plugin/models/voxel_encoders/voxel_encoder.py:82,99-102,189,232
 * third-party op: mmcv.ops.DynamicScatter -> dynamic_point_to_voxel_forward (Appendix B.3):
 * rows with any negative coord are dropped (and, given a batch count, rows outside the grid); unique voxel coords sorted lexicographically over
 * (b,z,y,x); per voxel mean (sum in point order / count) or max of the point features.
 * point2voxel[i] = row of point i in the output, or -1.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int64_t key;
    int32_t idx;
} orc_kv;
static int kv_cmp(const void *a, const void *b)
{
    const orc_kv *x = (const orc_kv *)a, *y = (const orc_kv *)b;
    if (x->key != y->key) return x->key < y->key ? -1 : 1;
    return x->idx < y->idx ? -1 : (x->idx > y->idx);
}

int orc_dynamic_scatter_batch(const float *feats, const int *coors /* n x 4 (b,z,y,x) */, int n, int C,
                              const int *grid_zyx /* D,H,W */, int batch /* > 0: rows outside the grid are dropped too */,
                              int mode /* 0 mean, 1 max */, float *out_feats /* n x C */, int *out_coors /* n x 4 */,
                              int *point2voxel, int *M_out)
{
    orc_kv *kv = (orc_kv *)malloc(sizeof(orc_kv) * (size_t)(n > 0 ? n : 1));
    if (!kv) return ORC_ENOMEM;
    int nv = 0;
    for (int i = 0; i < n; ++i) {
        const int *c = coors + 4 * i;
        point2voxel[i] = -1;
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[3] < 0) continue;
        /* the coordinate rule of the library (include/srfdet3d.h, K3): a row that names no cell of the
         * batch x D x H x W grid is dropped, not filed under the cell its linearised key happens to hit */
        if (batch > 0 && (c[0] >= batch || c[1] >= grid_zyx[0] || c[2] >= grid_zyx[1] || c[3] >= grid_zyx[2])) continue;
        kv[nv].key = (((int64_t)c[0] * grid_zyx[0] + c[1]) * grid_zyx[1] + c[2]) * grid_zyx[2] + c[3];
        kv[nv].idx = i;
        ++nv;
    }
    qsort(kv, (size_t)nv, sizeof(orc_kv), kv_cmp);
    int M = 0;
    int j = 0;
    while (j < nv) {
        int e = j;
        while (e < nv && kv[e].key == kv[j].key) ++e;
        const int *c0 = coors + 4 * kv[j].idx;
        memcpy(out_coors + 4 * M, c0, sizeof(int) * 4);
        float *o = out_feats + (size_t)M * C;
        for (int c = 0; c < C; ++c) {
            float acc = mode == 0 ? 0.0f : -INFINITY;
            for (int t = j; t < e; ++t) { /* point order: kv sorted by (key, idx) */
                float v = feats[(size_t)kv[t].idx * C + c];
                if (mode == 0)
                    acc = acc + v;
                else
                    acc = v > acc ? v : acc;
            }
            o[c] = mode == 0 ? acc / (float)(e - j) : acc;
        }
        for (int t = j; t < e; ++t) point2voxel[kv[t].idx] = M;
        ++M;
        j = e;
    }
    *M_out = M;
    free(kv);
    return ORC_OK;
}

/* the op as mmcv defines it, with no batch count: only rows with a negative entry are dropped */
int orc_dynamic_scatter(const float *feats, const int *coors, int n, int C, const int *grid_zyx, int mode,
                        float *out_feats, int *out_coors, int *point2voxel, int *M_out)
{
    return orc_dynamic_scatter_batch(feats, coors, n, C, grid_zyx, 0, mode, out_feats, out_coors, point2voxel, M_out);
}

/* ------------------------------------------------------------------------------------------
 * K4  sparse-conv rulebooks
 * reference call sites: SparseConvTensor built at mmdet3d_plugin/models/middle_encoders/
 * sparse_encoder_custom.py:123-124; SubMConv3d / SparseConv3d layers built at :73-107 and :182-201.
 * third-party op: spconv indice-pair generation (Appendix B.4).
 *
 * The rulebook is held output-stationary: nbr[k * A_out + o] = input row feeding output row o
 * through kernel offset k (k = (kz*KH + ky)*KW + kx), or -1.  The reference's pair lists are the
 * sets {(nbr[k][o], o) : nbr[k][o] >= 0}; SURVEY.md 8(a) "canonical form" compares those sets.
 * Output rows of a strided conv are numbered in first-seen order over (input row, k) ascending,
 * which is what a sequential spconv-1.x style build produces.
 * ---------------------------------------------------------------------------------------- */
static inline int64_t coord_key(int b, int z, int y, int x, const int *shape)
{
    return (((int64_t)b * shape[0] + z) * shape[1] + y) * shape[2] + x;
}

int orc_rulebook_subm(const int *indices /* A x 4 (b,z,y,x) */, int A, const int *shape /* D,H,W */,
                      const int *ksize, int *nbr /* K x A */, int *pair_counts /* K */)
{
    int K = ksize[0] * ksize[1] * ksize[2];
    orc_map m;
    if (map_init(&m, (uint64_t)A)) return ORC_ENOMEM;
    for (int i = 0; i < A; ++i) {
        const int *c = indices + 4 * i;
        map_put(&m, coord_key(c[0], c[1], c[2], c[3], shape), i);
    }
    for (int k = 0; k < K; ++k) pair_counts[k] = 0;
    for (int o = 0; o < A; ++o) {
        const int *c = indices + 4 * o;
        int k = 0;
        for (int kz = 0; kz < ksize[0]; ++kz)
            for (int ky = 0; ky < ksize[1]; ++ky)
                for (int kx = 0; kx < ksize[2]; ++kx, ++k) {
                    int z = c[1] + kz - ksize[0] / 2, y = c[2] + ky - ksize[1] / 2, x = c[3] + kx - ksize[2] / 2;
                    int v = -1;
                    if (z >= 0 && z < shape[0] && y >= 0 && y < shape[1] && x >= 0 && x < shape[2])
                        v = map_get(&m, coord_key(c[0], z, y, x, shape));
                    nbr[(size_t)k * A + o] = v;
                    if (v >= 0) pair_counts[k]++;
                }
    }
    map_free(&m);
    return ORC_OK;
}

/* out_shape[d] = floor((shape[d] + 2*pad[d] - ksize[d]) / stride[d]) + 1 */
int orc_rulebook_strided(const int *indices, int A, const int *shape, const int *ksize, const int *stride,
                         const int *pad, int cap_out, int *out_indices /* cap_out x 4 */, int *A_out,
                         int *nbr /* K x cap_out, row stride cap_out */, int *pair_counts)
{
    int K = ksize[0] * ksize[1] * ksize[2];
    int oshape[3];
    for (int d = 0; d < 3; ++d) {
        /* a window larger than the padded grid has no output: C's division would turn (-1) / 2 + 1 into 1 */
        if (stride[d] <= 0 || shape[d] + 2 * pad[d] < ksize[d]) return ORC_EINVAL;
        oshape[d] = (shape[d] + 2 * pad[d] - ksize[d]) / stride[d] + 1;
    }
    orc_map m;
    if (map_init(&m, (uint64_t)cap_out)) return ORC_ENOMEM;
    for (size_t t = 0; t < (size_t)K * cap_out; ++t) nbr[t] = -1;
    for (int k = 0; k < K; ++k) pair_counts[k] = 0;
    int M = 0;
    for (int i = 0; i < A; ++i) {
        const int *c = indices + 4 * i;
        int k = 0;
        for (int kz = 0; kz < ksize[0]; ++kz)
            for (int ky = 0; ky < ksize[1]; ++ky)
                for (int kx = 0; kx < ksize[2]; ++kx, ++k) {
                    int kk[3] = {kz, ky, kx};
                    int q[3], ok = 1;
                    for (int d = 0; d < 3; ++d) {
                        int t = c[1 + d] + pad[d] - kk[d];
                        if (t < 0 || t % stride[d] != 0) {
                            ok = 0;
                            break;
                        }
                        q[d] = t / stride[d];
                        if (q[d] >= oshape[d]) {
                            ok = 0;
                            break;
                        }
                    }
                    if (!ok) continue;
                    int64_t key = coord_key(c[0], q[0], q[1], q[2], oshape);
                    int o = map_get(&m, key);
                    if (o == -1) {
                        if (M >= cap_out) {
                            map_free(&m);
                            return ORC_EOVERFLOW;
                        }
                        o = M++;
                        map_put(&m, key, o);
                        out_indices[4 * o] = c[0];
                        out_indices[4 * o + 1] = q[0];
                        out_indices[4 * o + 2] = q[1];
                        out_indices[4 * o + 3] = q[2];
                    }
                    nbr[(size_t)k * cap_out + o] = i;
                    pair_counts[k]++;
                }
    }
    *A_out = M;
    map_free(&m);
    return ORC_OK;
}

/* ------------------------------------------------------------------------------------------
 * K5  sparse convolution forward (+ eval BatchNorm1d + residual + ReLU as the reference chains them)
 * reference call sites: every conv of SparseEncoderCustom.forward, sparse_encoder_custom.py:125-134;
 * module chain conv -> BN1d(eps 1e-3) -> ReLU from make_sparse_convmodule (Appendix B.4), and
 * SparseBasicBlock conv1-BN-ReLU-conv2-BN-(+identity)-ReLU.
 * out[o][co] = sum over k ascending, c ascending of in[nbr[k][o]][c] * W[k][c][co], accumulated as a
 * binary32 fmaf chain (the order the MI355X f32 MFMA uses, so the device result can be compared
 * exactly).  BN in eval is applied as y = fmaf(x, alpha, beta) with alpha = gamma / sqrt(var + eps),
 * beta = bias - mean * alpha (the folded form torch's CPU batch-norm uses); pass alpha = NULL to skip.
 * ---------------------------------------------------------------------------------------- */
int orc_spconv_fwd(const float *in, int A_in, int Cin, const float *W /* K x Cin x Cout */, int K,
                   const int *nbr, int nbr_stride, int A_out, int Cout, const float *alpha, const float *beta,
                   const float *residual, int relu, float *out)
{
    (void)A_in;
#pragma omp parallel for schedule(static)
    for (int o = 0; o < A_out; ++o) {
        float acc[512];
        for (int co = 0; co < Cout; ++co) acc[co] = 0.0f;
        for (int k = 0; k < K; ++k) {
            int i = nbr[(size_t)k * nbr_stride + o];
            if (i < 0) continue;
            const float *x = in + (size_t)i * Cin;
            const float *w = W + (size_t)k * Cin * Cout;
            for (int c = 0; c < Cin; ++c) {
                float xv = x[c];
                const float *wr = w + (size_t)c * Cout;
                for (int co = 0; co < Cout; ++co) acc[co] = fmaf(xv, wr[co], acc[co]);
            }
        }
        float *y = out + (size_t)o * Cout;
        for (int co = 0; co < Cout; ++co) {
            float v = acc[co];
            if (alpha) v = fmaf(v, alpha[co], beta[co]);
            if (residual) v = v + residual[(size_t)o * Cout + co];
            if (relu) v = v > 0.0f ? v : 0.0f;
            y[co] = v;
        }
    }
    return ORC_OK;
}

/* ------------------------------------------------------------------------------------------
 * K6  SparseConvTensor.dense() followed by view(N, C*D, H, W)
 * reference: sparse_encoder_custom.py:135-138.  out is (B, C, D, H, W) contiguous, zero elsewhere.
 * ---------------------------------------------------------------------------------------- */
int orc_densify(const float *feats, const int *indices, int A, int C, int B, int D, int H, int W, float *out)
{
    memset(out, 0, sizeof(float) * (size_t)B * C * D * H * W);
    for (int a = 0; a < A; ++a) {
        const int *c = indices + 4 * a;
        for (int ch = 0; ch < C; ++ch)
            out[((((size_t)c[0] * C + ch) * D + c[1]) * H + c[2]) * W + c[3]] = feats[(size_t)a * C + ch];
    }
    return ORC_OK;
}

/* ------------------------------------------------------------------------------------------
 * K7  RoIAlign (avg, aligned=True) behind mmdet SingleRoIExtractor
 * reference call sites: mmdet3d_plugin/models/sparse_heads/srfdet_head.py:1685, :2548, :2626;
 * config configs/nus/srfdet_voxel_nusc_LC.py:169-178.
 * third-party ops: mmcv roi_align_forward + mmdet SingleRoIExtractor.map_roi_levels (Appendix B.5).
 * feats are NCHW contiguous per level; out is (R, C, PH, PW), zero for RoIs mapped to no level.
 * ---------------------------------------------------------------------------------------- */
static inline float bilinear(const float *plane, int H, int W, float y, float x)
{
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return 0.0f;
    if (!(y == y) || !(x == x)) return 0.0f; /* a NaN coordinate passes every comparison above and (int)NaN is no index: the
                                                sample contributes nothing, as in the device kernel */
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) {
        y_high = y_low = H - 1;
        y = (float)y_low;
    } else
        y_high = y_low + 1;
    if (x_low >= W - 1) {
        x_high = x_low = W - 1;
        x = (float)x_low;
    } else
        x_high = x_low + 1;
    float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
    float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
    return w1 * plane[y_low * W + x_low] + w2 * plane[y_low * W + x_high] + w3 * plane[y_high * W + x_low] +
           w4 * plane[y_high * W + x_high];
}

int orc_roi_level(const float *rois, int R, int num_levels, float finest_scale, int *lvl)
{
    for (int r = 0; r < R; ++r) {
        const float *b = rois + 5 * r;
        float scale = sqrtf((b[3] - b[1]) * (b[4] - b[2]));
        float t = floorf(log2f(scale / finest_scale + 1e-6f));
        int l = t < 0.0f ? 0 : (t > (float)(num_levels - 1) ? num_levels - 1 : (int)t);
        if (!(t == t)) l = 0; /* NaN area (degenerate projected boxes): clamp(min=0) keeps NaN in torch; .long() of NaN is
                                 implementation-defined -- pinned to level 0 here and in the device kernel */
        lvl[r] = l;
    }
    return ORC_OK;
}

int orc_roi_align_level(const float *feat /* N x C x H x W */, int N, int C, int H, int W, const float *rois, int R,
                        const int *lvl, int this_level, float spatial_scale, int PH, int PW, int sampling_ratio,
                        int aligned, float *out /* R x C x PH x PW, accumulated into */)
{
    float off = aligned ? 0.5f : 0.0f;
#pragma omp parallel for schedule(dynamic, 4)
    for (int r = 0; r < R; ++r) {
        if (lvl && lvl[r] != this_level) continue;
        const float *b = rois + 5 * r;
        int n = (int)b[0];
        if (n < 0 || n >= N) continue;
        float x1 = b[1] * spatial_scale - off, y1 = b[2] * spatial_scale - off;
        float x2 = b[3] * spatial_scale - off, y2 = b[4] * spatial_scale - off;
        float rw = x2 - x1, rh = y2 - y1;
        if (!aligned) {
            rw = rw > 1.0f ? rw : 1.0f;
            rh = rh > 1.0f ? rh : 1.0f;
        }
        float bin_h = rh / (float)PH, bin_w = rw / (float)PW;
        int gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)PH);
        int gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)PW);
        float count = (float)(gh * gw > 1 ? gh * gw : 1);
        for (int c = 0; c < C; ++c) {
            const float *plane = feat + ((size_t)n * C + c) * H * W;
            for (int ph = 0; ph < PH; ++ph)
                for (int pw = 0; pw < PW; ++pw) {
                    float acc = 0.0f;
                    for (int iy = 0; iy < gh; ++iy) {
                        float y = y1 + (float)ph * bin_h + ((float)iy + 0.5f) * bin_h / (float)gh;
                        for (int ix = 0; ix < gw; ++ix) {
                            float x = x1 + (float)pw * bin_w + ((float)ix + 0.5f) * bin_w / (float)gw;
                            acc += bilinear(plane, H, W, y, x);
                        }
                    }
                    out[(((size_t)r * C + c) * PH + ph) * PW + pw] = acc / count;
                }
        }
    }
    return ORC_OK;
}
