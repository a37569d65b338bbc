// augment.hip -- the train-time augmentation of the reference's train pipelines on the device (gfx950):
//   GlobalRotScaleTrans -> RandomFlip3D -> PointsRangeFilter on the points (srf_points_augment),
//   the same steps -> ObjectRangeFilter (+ limit_yaw) -> ObjectNameFilter on the GT boxes and labels (srf_boxes_augment),
//   and the mask multiplication of GridMask (mmdet3d_plugin/models/utils/grid_mask.py:72-128, srf_grid_mask).
//
// Reference call sites: the `train_pipeline` of configs/nus/srfdet_voxel_nusc_L.py (and the other LiDAR-only configs), the
// ObjectRangeFilter / ObjectNameFilter of every LC train pipeline, and SRFDet.extract_img_feat (srfdet.py:189-190).
// The 3-D transforms follow mmdet3d 1.0.0rc6 (LiDARPoints / LiDARInstance3DBoxes rotate, scale, translate, flip,
// in_range_bev, limit_yaw): third party, restated here, parity unpinned.
//
// Numerics: every random draw and every sin / cos / arctan2 is done by the caller on the host.  The kernels only do
// correctly rounded + - * / floor in the reference's order (the library builds with -ffp-contract=off); the 3 x 3 product
// keeps its zero terms so a NaN / inf coordinate spreads as it does through `p @ rot_mat_T`.  A step whose bit is clear is
// skipped, not applied as an identity: that keeps a fused run bit-identical to the transforms run one by one.
//
// Points and boxes are a flag + exclusive scan + ordered copy (srf_device_scan); the transform is recomputed in the copy
// pass instead of being staged (12 flops per point against a row of 16-20 bytes).  GridMask is pure streaming work.
#include "common.hpp"

enum {
    SRF_AUG_ROTATE = 1,
    SRF_AUG_SCALE = 2,
    SRF_AUG_TRANSLATE = 4,
    SRF_AUG_FLIP_H = 8,
    SRF_AUG_FLIP_V = 16,
};

struct AugParams {
    float s, c, yaw_add, scale, t[3];
    int steps;
};

static bool aug_params(int steps, const float *aug, AugParams *a)
{
    if (steps & ~31) return false;
    if (steps && !aug) return false;
    a->steps = steps;
    a->s = aug ? aug[0] : 0.0f;
    a->c = aug ? aug[1] : 0.0f;
    a->yaw_add = aug ? aug[2] : 0.0f;
    a->scale = aug ? aug[3] : 0.0f;
    for (int d = 0; d < 3; ++d) a->t[d] = aug ? aug[4 + d] : 0.0f;
    return true;
}

// p[:, :3] @ rot_mat_T with rot_mat_T = [[c, s, 0], [-s, c, 0], [0, 0, 1]]: products rounded one by one, summed left to right
__device__ __forceinline__ void aug_rotate(float s, float c, float &x, float &y, float &z)
{
    const float ns = -s;
    const float nx = __fadd_rn(__fadd_rn(__fmul_rn(x, c), __fmul_rn(y, ns)), __fmul_rn(z, 0.0f));
    const float ny = __fadd_rn(__fadd_rn(__fmul_rn(x, s), __fmul_rn(y, c)), __fmul_rn(z, 0.0f));
    const float nz = __fadd_rn(__fadd_rn(__fmul_rn(x, 0.0f), __fmul_rn(y, 0.0f)), __fmul_rn(z, 1.0f));
    x = nx;
    y = ny;
    z = nz;
}

// rotate -> scale -> translate -> horizontal flip -> vertical flip of one point's x, y, z
__device__ __forceinline__ void aug_xyz(const AugParams &a, float &x, float &y, float &z)
{
    if (a.steps & SRF_AUG_ROTATE) aug_rotate(a.s, a.c, x, y, z);
    if (a.steps & SRF_AUG_SCALE) {
        x = __fmul_rn(x, a.scale);
        y = __fmul_rn(y, a.scale);
        z = __fmul_rn(z, a.scale);
    }
    if (a.steps & SRF_AUG_TRANSLATE) {
        x = __fadd_rn(x, a.t[0]);
        y = __fadd_rn(y, a.t[1]);
        z = __fadd_rn(z, a.t[2]);
    }
    if (a.steps & SRF_AUG_FLIP_H) y = -y;
    if (a.steps & SRF_AUG_FLIP_V) x = -x;
}

// ---------------------------------------------------------------------------------------------------------------------
// points
// ---------------------------------------------------------------------------------------------------------------------
struct PaKeep {
    const float *p;
    int nf;
    AugParams a;
    float lo[3], hi[3];
    int use_range;
    __device__ int operator()(int i) const
    {
        if (!use_range) return 1;
        float x = p[(size_t)i * nf], y = p[(size_t)i * nf + 1], z = p[(size_t)i * nf + 2];
        aug_xyz(a, x, y, z);
        return (x > lo[0] && y > lo[1] && z > lo[2] && x < hi[0] && y < hi[1] && z < hi[2]) ? 1 : 0;
    }
};

struct PaCopy {
    const float *p;
    float *out;
    int *index;
    int nf;
    AugParams a;
    __device__ void operator()(int i, int v, int prefix) const
    {
        if (!v) return;
        const float *src = p + (size_t)i * nf;
        float *dst = out + (size_t)prefix * nf;
        float x = src[0], y = src[1], z = src[2];
        aug_xyz(a, x, y, z);
        dst[0] = x;
        dst[1] = y;
        dst[2] = z;
        for (int c = 3; c < nf; ++c) dst[c] = src[c];
        if (index) index[prefix] = i;
    }
};

extern "C" size_t srf_points_augment_workspace_bytes(int n) { return n < 0 ? 0 : ((size_t)srf_scan_blocks(n) + 2) * sizeof(int); }

extern "C" int srf_points_augment(const float *points, int n, int nf, int steps, const float *aug, const float *pc_range,
                                  float *out_points, int *out_index, int *num_out, void *workspace, srf_stream_t stream)
{
    AugParams a;
    if (n < 0 || nf < 3 || !num_out || !aug_params(steps, aug, &a)) return SRF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        SRF_HIP_TRY(srf_fill_bytes(num_out, 0, sizeof(int), st));
        return SRF_OK;
    }
    if (!points || !out_points || !workspace) return SRF_EINVAL;
    PaKeep keep;
    keep.p = points;
    keep.nf = nf;
    keep.a = a;
    keep.use_range = pc_range != nullptr;
    for (int d = 0; d < 3; ++d) {
        keep.lo[d] = pc_range ? pc_range[d] : 0.0f;
        keep.hi[d] = pc_range ? pc_range[3 + d] : 0.0f;
    }
    PaCopy copy{points, out_points, out_index, nf, a};
    return srf_device_scan(n, keep, copy, (int *)workspace, num_out, -1, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// boxes: (n, 7 | 9) [x, y, z, dx, dy, dz, yaw (, vx, vy)] + int64 labels
// ---------------------------------------------------------------------------------------------------------------------
#define SRF_AUG_MAX_BOX_DIM 9

struct BoxAug {
    AugParams a;
    int dim;
    float bev[4];  // xmin, ymin, xmax, ymax
    int use_bev;
    int num_classes;

    // the transformed row in r[0..dim); returns whether the box survives the range and name filters
    __device__ bool apply(const float *src, long long label, float *r) const
    {
        for (int c = 0; c < dim; ++c) r[c] = src[c];
        if (a.steps & SRF_AUG_ROTATE) {
            aug_rotate(a.s, a.c, r[0], r[1], r[2]);
            r[6] = __fadd_rn(r[6], a.yaw_add);
            if (dim == 9) {  // [vx, vy] @ rot_mat_T[:2, :2]
                const float vx = r[7], vy = r[8];
                r[7] = __fadd_rn(__fmul_rn(vx, a.c), __fmul_rn(vy, -a.s));
                r[8] = __fadd_rn(__fmul_rn(vx, a.s), __fmul_rn(vy, a.c));
            }
        }
        if (a.steps & SRF_AUG_SCALE) {
            for (int c = 0; c < 6; ++c) r[c] = __fmul_rn(r[c], a.scale);
            for (int c = 7; c < dim; ++c) r[c] = __fmul_rn(r[c], a.scale);
        }
        if (a.steps & SRF_AUG_TRANSLATE)
            for (int c = 0; c < 3; ++c) r[c] = __fadd_rn(r[c], a.t[c]);
        if (a.steps & SRF_AUG_FLIP_H) {  // columns 1::7, yaw = -yaw
            r[1] = -r[1];
            if (dim == 9) r[8] = -r[8];
            r[6] = -r[6];
        }
        if (a.steps & SRF_AUG_FLIP_V) {  // columns 0::7, yaw = -yaw + float32(pi)
            r[0] = -r[0];
            if (dim == 9) r[7] = -r[7];
            r[6] = __fadd_rn(-r[6], 3.14159265358979323846f);
        }
        bool keep = true;
        if (use_bev) {
            keep = r[0] > bev[0] && r[1] > bev[1] && r[0] < bev[2] && r[1] < bev[3];
            const float P = 6.28318530717958647692f;  // limit_yaw(offset=0.5, period=2 pi)
            r[6] = __fsub_rn(r[6], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(r[6], P), 0.5f)), P));
        }
        if (num_classes > 0) keep = keep && label >= 0 && label < num_classes;
        return keep;
    }
};

struct BaKeep {
    const float *b;
    const long long *labels;
    BoxAug f;
    __device__ int operator()(int i) const
    {
        if (!f.use_bev && f.num_classes <= 0) return 1;
        float r[SRF_AUG_MAX_BOX_DIM];
        return f.apply(b + (size_t)i * f.dim, labels[i], r) ? 1 : 0;
    }
};

struct BaCopy {
    const float *b;
    const long long *labels;
    float *out;
    long long *out_labels;
    int *index;
    BoxAug f;
    __device__ void operator()(int i, int v, int prefix) const
    {
        if (!v) return;
        float r[SRF_AUG_MAX_BOX_DIM];
        f.apply(b + (size_t)i * f.dim, labels[i], r);
        for (int c = 0; c < f.dim; ++c) out[(size_t)prefix * f.dim + c] = r[c];
        out_labels[prefix] = labels[i];
        if (index) index[prefix] = i;
    }
};

extern "C" size_t srf_boxes_augment_workspace_bytes(int n) { return n < 0 ? 0 : ((size_t)srf_scan_blocks(n) + 2) * sizeof(int); }

extern "C" int srf_boxes_augment(const float *boxes, const long long *labels, int n, int box_dim, int steps, const float *aug,
                                 const float *bev_range, int num_classes, float *out_boxes, long long *out_labels, int *out_index,
                                 int *num_out, void *workspace, srf_stream_t stream)
{
    BoxAug f;
    if (n < 0 || (box_dim != 7 && box_dim != 9) || !num_out || !aug_params(steps, aug, &f.a)) return SRF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        SRF_HIP_TRY(srf_fill_bytes(num_out, 0, sizeof(int), st));
        return SRF_OK;
    }
    if (!boxes || !labels || !out_boxes || !out_labels || !workspace) return SRF_EINVAL;
    f.dim = box_dim;
    f.use_bev = bev_range != nullptr;
    for (int d = 0; d < 4; ++d) f.bev[d] = bev_range ? bev_range[d] : 0.0f;
    f.num_classes = num_classes;
    BaKeep keep{boxes, labels, f};
    BaCopy copy{boxes, labels, out_boxes, out_labels, out_index, f};
    return srf_device_scan(n, keep, copy, (int *)workspace, num_out, -1, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// GridMask: out = in * mask, the mask evaluated per pixel from the stripe parameters (never materialised)
// ---------------------------------------------------------------------------------------------------------------------
// The reference draws a (hh, ww) = (int(1.5 h), int(1.5 w)) mask of ones, zeroes hh // d row stripes [d i + st_h, d i + st_h + l)
// (and the same for columns), rotates it by 0 degrees and crops the centred (h, w) window; mode 1 takes 1 - mask.  Pixel (y, x)
// of the crop is mask row yy = y + (hh - h) // 2: in a stripe iff q = yy - st_h >= 0, q // d < hh // d and q % d < l (l < d, so
// the stripes never overlap and the min(s + l, hh) clip changes nothing inside the window).
struct GmStripes {
    int off, st, n, d, l, use;
    __device__ __forceinline__ bool in(int v) const
    {
        const int q = v + off - st;
        return use && q >= 0 && (unsigned)q / (unsigned)d < (unsigned)n && (unsigned)q % (unsigned)d < (unsigned)l;
    }
};

// one thread = 4 consecutive pixels of one row: one 16-byte load and store when the rows are 16-byte aligned (W % 4 == 0)
__global__ __launch_bounds__(256) void srf_grid_mask_k(const float *__restrict__ in, long long rows, int H, int W, GmStripes rs,
                                                       GmStripes cs, int mode, int vec, float *__restrict__ out)
{
    const int wq = (W + 3) >> 2;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * wq) return;
    const long long row = t / wq;
    const int x0 = (int)(t - row * wq) * 4;
    const int y = (int)(row % H);
    const bool row_in = rs.in(y);
    float m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool stripe = row_in || cs.in(x0 + j);
        m[j] = (mode == 1 ? stripe : !stripe) ? 1.0f : 0.0f;
    }
    const size_t base = (size_t)row * W + x0;
    if (vec) {
        const float4 v = *reinterpret_cast<const float4 *>(in + base);
        *reinterpret_cast<float4 *>(out + base) =
            make_float4(__fmul_rn(v.x, m[0]), __fmul_rn(v.y, m[1]), __fmul_rn(v.z, m[2]), __fmul_rn(v.w, m[3]));
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < W) out[base + j] = __fmul_rn(in[base + j], m[j]);
}

extern "C" int srf_grid_mask(const float *in, int planes, int H, int W, int d, int l, int st_h, int st_w, int use_h, int use_w,
                             int mode, float *out, srf_stream_t stream)
{
    if (planes < 0 || H <= 0 || W <= 0 || d < 2 || l < 1 || l >= d || st_h < 0 || st_h >= d || st_w < 0 || st_w >= d ||
        (mode != 0 && mode != 1))
        return SRF_EINVAL;
    if (planes == 0) return SRF_OK;
    if (!in || !out) return SRF_EINVAL;
    const int hh = (int)(1.5 * (double)H), ww = (int)(1.5 * (double)W);
    GmStripes rs{(hh - H) / 2, st_h, hh / d, d, l, use_h ? 1 : 0};
    GmStripes cs{(ww - W) / 2, st_w, ww / d, d, l, use_w ? 1 : 0};
    const int vec = (W % 4 == 0) && ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0);
    const long long rows = (long long)planes * H;
    const long long total = rows * ((W + 3) >> 2);
    if (total > (1LL << 31) * 255) return SRF_EINVAL;  // the grid's block count must fit an int
    hipLaunchKernelGGL(srf_grid_mask_k, dim3(srf_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, in, rows, H, W, rs, cs,
                       mode, vec, out);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
