// objsample.hip -- the point- and pair-level work of the GT-database sampling (ObjectSample) and per-object noise (ObjectNoise)
// of the LiDAR-only train pipelines (configs/nus/srfdet_voxel_nusc_L.py, configs/kitti/srfdet_voxel_kitti_L.py) on the device:
//   srf_points_in_boxes        box_np_ops.points_in_rbbox: the first box whose six surface planes all have the point behind them
//   srf_box_collision_matrix   data_augment_utils.box_collision_test over every (box, qbox) pair
//   srf_box_collision_accept   DataBaseSampler.sample_class_v2's greedy rejection, class after class, in one workgroup
//   srf_object_sample_merge    cat([sampled points translated to their box, original points in no accepted box])
//   srf_object_noise           noise_per_box (first colliding-free try per box) + points_transform_ + box3d_transform_
// mmdet3d 1.0.0rc6 semantics (third party, restated here, parity unpinned); the host half is plugin/object_sample.py.
//
// Numerics: the host draws every random number and computes every sin / cos, the BEV corners and the surface planes (O(boxes),
// numpy float32).  The kernels do correctly rounded float32 + - * and compares in the reference's order (the library builds
// with -ffp-contract=off and the arithmetic below is spelled out with the _rn intrinsics), plus the float64 adds where the
// reference adds float64 noise to float32 coordinates.  So every result is bit-exact against a numpy restatement.
#include "common.hpp"

#define SRF_OS_MAX_BOXES 512      // srf_points_in_boxes / srf_object_noise: planes of up to 512 boxes in LDS (48 KiB + mask)
#define SRF_OS_MAX_COLL_BOXES 2048  // srf_box_collision_accept: fixed + candidate corners in LDS (64 KiB)
#define SRF_OS_SEL_THREADS 1024

// ---------------------------------------------------------------------------------------------------------------------
// points in boxes
// ---------------------------------------------------------------------------------------------------------------------
// planes (6 x [a, b, c, d]): inside iff ((x a + y b) + z c) + d < 0 for all six.  points_in_convex_polygon_3d_jit rejects on
// `sign >= 0` instead, which differs only for a NaN sign (that loop counts it inside, this test outside).
__device__ __forceinline__ bool os_inside(const float *pl, float x, float y, float z)
{
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const float *q = pl + 4 * f;
        const float s = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, q[0]), __fmul_rn(y, q[1])), __fmul_rn(z, q[2])), q[3]);
        if (!(s < 0.0f)) return false;
    }
    return true;
}

__device__ __forceinline__ int os_first_box(const float *s_pl, const int *s_mask, int m, float x, float y, float z)
{
    for (int b = 0; b < m; ++b)
        if (s_mask[b] && os_inside(s_pl + 24 * b, x, y, z)) return b;
    return -1;
}

// stage m boxes' planes (and the mask, 1 where NULL) in LDS; the caller syncs
__device__ __forceinline__ void os_stage_planes(const float *planes, const int *mask, int m, float *s_pl, int *s_mask)
{
    for (int t = threadIdx.x; t < 24 * m; t += blockDim.x) s_pl[t] = planes[t];
    for (int t = threadIdx.x; t < m; t += blockDim.x) s_mask[t] = mask ? (mask[t] != 0) : 1;
}

static size_t os_planes_lds(int m) { return (size_t)m * 25 * sizeof(float); }

__global__ __launch_bounds__(256) void srf_points_in_boxes_k(const float *__restrict__ points, int n, int nf,
                                                             const float *__restrict__ planes, int m, const int *__restrict__ mask,
                                                             int *__restrict__ out_box, int *__restrict__ num_outside)
{
    extern __shared__ float s_pl[];
    int *s_mask = (int *)(s_pl + 24 * m);
    os_stage_planes(planes, mask, m, s_pl, s_mask);
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    int outside = 0;
    if (i < n) {
        const float *p = points + (size_t)i * nf;
        const int b = os_first_box(s_pl, s_mask, m, p[0], p[1], p[2]);
        out_box[i] = b;
        outside = b < 0;
    }
    if (num_outside) {
        const int c = srf_wave_sum(outside);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(num_outside, c);
    }
}

extern "C" int srf_points_in_boxes(const float *points, int n, int nf, const float *planes, int m, const int *box_mask, int *out_box,
                                   int *num_outside, srf_stream_t stream)
{
    if (n < 0 || nf < 3 || m < 0) return SRF_EINVAL;
    if (m > SRF_OS_MAX_BOXES) return SRF_EUNSUPPORTED;
    if ((n > 0 && (!points || !out_box)) || (m > 0 && !planes)) return SRF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (num_outside) SRF_HIP_TRY(srf_fill_bytes(num_outside, 0, sizeof(int), st));
    if (n == 0) return SRF_OK;
    hipLaunchKernelGGL(srf_points_in_boxes_k, dim3(srf_ceil_div(n, 256)), dim3(256), os_planes_lds(m), st, points, n, nf, planes, m,
                       box_mask, out_box, num_outside);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// BEV box collision: data_augment_utils.box_collision_test(boxes, qboxes, clockwise=True) for one pair
// ---------------------------------------------------------------------------------------------------------------------
// a, q: 4 corners (x, y) each, in the clockwise order of center_to_corner_box2d.  The order of the tests is the reference's:
// standup (axis-aligned hull) overlap, else no collision; then any pair of crossing edges; then every corner of q strictly
// inside a, or every corner of a strictly inside q.  Edges that only touch and boxes that only share a face do not collide;
// nor do two identical boxes (the reference clears a box's own entry, but a duplicate of it passes).
__device__ __forceinline__ float os_min(float a, float b) { return b < a ? b : a; }  // Python's min / max
__device__ __forceinline__ float os_max(float a, float b) { return b > a ? b : a; }

__device__ __forceinline__ bool os_ccw_gt(const float *A, const float *C, const float *D)
{  // (D1 - A1) (C0 - A0) > (C1 - A1) (D0 - A0)
    return __fmul_rn(__fsub_rn(D[1], A[1]), __fsub_rn(C[0], A[0])) > __fmul_rn(__fsub_rn(C[1], A[1]), __fsub_rn(D[0], A[0]));
}

// every corner of q strictly inside the clockwise polygon a
__device__ __forceinline__ bool os_contains(const float (*a)[2], const float (*q)[2])
{
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const float v0 = -__fsub_rn(a[k][0], a[k1][0]), v1 = -__fsub_rn(a[k][1], a[k1][1]);  // vec = -(a[k] - a[k+1])
            const float cross = __fsub_rn(__fmul_rn(v1, __fsub_rn(a[k][0], q[l][0])), __fmul_rn(v0, __fsub_rn(a[k][1], q[l][1])));
            if (cross >= 0.0f) return false;
        }
    return true;
}

__device__ __forceinline__ bool os_collide(const float (*a)[2], const float (*q)[2])
{
    float amin[2], amax[2], qmin[2], qmax[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        amin[d] = os_min(os_min(os_min(a[0][d], a[1][d]), a[2][d]), a[3][d]);
        amax[d] = os_max(os_max(os_max(a[0][d], a[1][d]), a[2][d]), a[3][d]);
        qmin[d] = os_min(os_min(os_min(q[0][d], q[1][d]), q[2][d]), q[3][d]);
        qmax[d] = os_max(os_max(os_max(q[0][d], q[1][d]), q[2][d]), q[3][d]);
    }
    const float iw = __fsub_rn(os_min(amax[0], qmax[0]), os_max(amin[0], qmin[0]));
    if (!(iw > 0.0f)) return false;
    const float ih = __fsub_rn(os_min(amax[1], qmax[1]), os_max(amin[1], qmin[1]));
    if (!(ih > 0.0f)) return false;
    for (int k = 0; k < 4; ++k) {
        const float *A = a[k], *B = a[(k + 1) & 3];
        for (int l = 0; l < 4; ++l) {
            const float *C = q[l], *D = q[(l + 1) & 3];
            if (os_ccw_gt(A, C, D) != os_ccw_gt(B, C, D) && os_ccw_gt(A, B, C) != os_ccw_gt(A, B, D)) return true;
        }
    }
    return os_contains(a, q) || os_contains(q, a);
}

__device__ __forceinline__ void os_load4(const float *src, float (*c)[2])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k][0] = src[2 * k];
        c[k][1] = src[2 * k + 1];
    }
}

__global__ __launch_bounds__(256) void srf_box_collision_matrix_k(const float *__restrict__ boxes, int N, const float *__restrict__ qboxes,
                                                                  int K, unsigned char *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)N * K) return;
    const int i = (int)(t / K), j = (int)(t - (long long)i * K);
    float a[4][2], q[4][2];
    os_load4(boxes + 8 * (size_t)i, a);
    os_load4(qboxes + 8 * (size_t)j, q);
    out[t] = os_collide(a, q) ? 1 : 0;
}

extern "C" int srf_box_collision_matrix(const float *boxes, int N, const float *qboxes, int K, unsigned char *out, srf_stream_t stream)
{
    if (N < 0 || K < 0) return SRF_EINVAL;
    if ((long long)N * K == 0) return SRF_OK;
    if (!boxes || !qboxes || !out) return SRF_EINVAL;
    if ((long long)N * K > (1LL << 31) * 255) return SRF_EINVAL;  // the grid's block count must fit an int
    hipLaunchKernelGGL(srf_box_collision_matrix_k, dim3(srf_ceil_div((long long)N * K, 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                       N, qboxes, K, out);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// greedy acceptance of the sampled candidates (DataBaseSampler.sample_all + sample_class_v2), one workgroup
// ---------------------------------------------------------------------------------------------------------------------
// Candidates are grouped by class (class c = [off[c], off[c + 1])), classes in sampling order.  Candidate i of class c is tested
// against the fixed boxes, the accepted candidates of the earlier classes, and the candidates of its own class that are not
// rejected (the later ones included), itself excluded: it is rejected iff it collides (row i of box_collision_test) with any of
// them.  That is sample_class_v2's coll_mat walk (a rejected row and column are cleared), run against the growing avoid_coll_boxes.
__global__ __launch_bounds__(SRF_OS_SEL_THREADS) void srf_box_collision_accept_k(const float *__restrict__ fixed, int n_fixed,
                                                                                const float *__restrict__ cand, int n_cand,
                                                                                const int *__restrict__ off, int num_classes,
                                                                                int *__restrict__ accept)
{
    extern __shared__ float s_c[];  // (n_fixed + n_cand) * 8 corners, then n_cand states
    int *s_state = (int *)(s_c + 8 * (size_t)(n_fixed + n_cand));
    __shared__ int s_hit;
    for (int t = threadIdx.x; t < 8 * n_fixed; t += blockDim.x) s_c[t] = fixed[t];
    for (int t = threadIdx.x; t < 8 * n_cand; t += blockDim.x) s_c[8 * n_fixed + t] = cand[t];
    for (int t = threadIdx.x; t < n_cand; t += blockDim.x) s_state[t] = 0;  // 0 rejected / not sampled, 1 accepted
    if (threadIdx.x == 0) s_hit = 0;
    __syncthreads();
    int prev_end = 0;
    for (int c = 0; c < num_classes; ++c) {
        const int cb = min(max(off[c], prev_end), n_cand);  // clamped: the ranges stay in bounds and ordered whatever off holds
        const int ce = min(max(off[c + 1], cb), n_cand);
        prev_end = ce;
        for (int i = cb; i < ce; ++i) {
            float a[4][2];
            os_load4(s_c + 8 * (size_t)(n_fixed + i), a);
            bool hit = false;
            for (int j = threadIdx.x; j < n_fixed + ce && !hit; j += blockDim.x) {
                const int k = j - n_fixed;
                bool live = k < 0 || (k < cb && s_state[k]) || (k >= cb && k != i && (k > i || s_state[k]));
                if (!live) continue;
                float q[4][2];
                os_load4(s_c + 8 * (size_t)j, q);
                hit = os_collide(a, q);
            }
            if (hit) s_hit = 1;
            __syncthreads();
            if (threadIdx.x == 0) {
                s_state[i] = s_hit ? 0 : 1;
                s_hit = 0;
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < n_cand; t += blockDim.x) accept[t] = s_state[t];
}

extern "C" int srf_box_collision_accept(const float *fixed, int n_fixed, const float *cand, int n_cand, const int *class_offsets,
                                        int num_classes, int *accept, srf_stream_t stream)
{
    if (n_fixed < 0 || n_cand < 0 || num_classes < 0) return SRF_EINVAL;
    if ((long long)n_fixed + n_cand > SRF_OS_MAX_COLL_BOXES) return SRF_EUNSUPPORTED;
    if (n_cand == 0) return SRF_OK;
    if ((n_fixed > 0 && !fixed) || !cand || !accept || (num_classes > 0 && !class_offsets)) return SRF_EINVAL;
    const size_t lds = (size_t)(n_fixed + n_cand) * 8 * sizeof(float) + (size_t)n_cand * sizeof(int);
    hipLaunchKernelGGL(srf_box_collision_accept_k, dim3(1), dim3(SRF_OS_SEL_THREADS), lds, (hipStream_t)stream, fixed, n_fixed, cand,
                       n_cand, class_offsets, num_classes, accept);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// merge: rows [0, s) = the accepted objects' points + their box centre, rows [s, s + kept) = the original points whose
// srf_points_in_boxes result is -1, order kept.  One order-preserving compaction over s + n elements (srf_device_scan).
// ---------------------------------------------------------------------------------------------------------------------
struct OsMergeKeep {
    const int *point_box;
    int s;
    __device__ int operator()(int i) const { return i < s ? 1 : (point_box[i - s] < 0 ? 1 : 0); }
};

struct OsMergeCopy {
    const float *points, *sampled, *centres;
    const int *obj_off;
    int s, k, nf;
    float *out;
    __device__ void operator()(int i, int v, int prefix) const
    {
        if (!v) return;
        float *dst = out + (size_t)prefix * nf;
        if (i >= s) {
            const float *src = points + (size_t)(i - s) * nf;
            for (int c = 0; c < nf; ++c) dst[c] = src[c];
            return;
        }
        int lo = 0, hi = k;  // the object of sampled row i: the last o with obj_off[o] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (obj_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        const float *src = sampled + (size_t)i * nf;
        for (int c = 0; c < 3; ++c) dst[c] = __fadd_rn(src[c], centres[3 * lo + c]);
        for (int c = 3; c < nf; ++c) dst[c] = src[c];
    }
};

extern "C" size_t srf_object_sample_merge_workspace_bytes(int n, int s)
{
    return (n < 0 || s < 0) ? 0 : ((size_t)srf_scan_blocks((long long)n + s) + 2) * sizeof(int);
}

extern "C" int srf_object_sample_merge(const float *points, int n, int nf, const int *point_box, const float *sampled, int s,
                                       const int *obj_offsets, const float *obj_centres, int k, float *out, int *num_out, void *workspace,
                                       srf_stream_t stream)
{
    if (n < 0 || s < 0 || nf < 3 || k < 0 || (s > 0 && k == 0) || !num_out || (long long)n + s > 0x7fffffffLL) return SRF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n + s == 0) {
        SRF_HIP_TRY(srf_fill_bytes(num_out, 0, sizeof(int), st));
        return SRF_OK;
    }
    if ((n > 0 && (!points || !point_box)) || (s > 0 && (!sampled || !obj_offsets || !obj_centres)) || !out || !workspace)
        return SRF_EINVAL;
    OsMergeKeep keep{point_box, s};
    OsMergeCopy copy{points, sampled, obj_centres, obj_offsets, s, k, nf, out};
    return srf_device_scan(n + s, keep, copy, (int *)workspace, num_out, -1, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// ObjectNoise: noise_per_box selection (one workgroup), then points_transform_ + box3d_transform_ (one pass)
// ---------------------------------------------------------------------------------------------------------------------
// The corners of try j of box i (noise_per_box): cur = corners[i] - xy[i] (float32); cur = cur @ [[c, s], [-s, c]] with the
// float32 sin / cos of the float64 angle (products rounded one by one); cur = float32(float64(cur) + (float64(xy[i]) + loc[i, j, :2])).
__device__ __forceinline__ void os_try_corners(const float (*base)[2], float bx, float by, float s, float c, const double *loc,
                                               float (*cur)[2])
{
    const double tx = __dadd_rn((double)bx, loc[0]), ty = __dadd_rn((double)by, loc[1]);
    const float ns = -s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float x = __fsub_rn(base[k][0], bx), y = __fsub_rn(base[k][1], by);
        const float rx = __fadd_rn(__fmul_rn(x, c), __fmul_rn(y, ns));
        const float ry = __fadd_rn(__fmul_rn(x, s), __fmul_rn(y, c));
        cur[k][0] = __double2float_rn(__dadd_rn((double)rx, tx));
        cur[k][1] = __double2float_rn(__dadd_rn((double)ry, ty));
    }
}

// Box i (in index order) takes its first try j whose moved BEV box collides with no other box's CURRENT corners (boxes moved
// before it in their new place, the others where they are); chosen[i] = j, or -1 when all num_try tries collide.
__global__ __launch_bounds__(SRF_OS_SEL_THREADS) void srf_object_noise_select_k(const float *__restrict__ boxes, int m, int dim,
                                                                               const float *__restrict__ corners,
                                                                               const float *__restrict__ rot_sc,
                                                                               const double *__restrict__ loc, int num_try,
                                                                               int *__restrict__ chosen)
{
    __shared__ float s_c[SRF_OS_MAX_BOXES * 8];
    __shared__ float s_xy[SRF_OS_MAX_BOXES * 2];
    __shared__ int s_coll[SRF_OS_SEL_THREADS];
    __shared__ int s_pick;
    for (int t = threadIdx.x; t < 8 * m; t += blockDim.x) s_c[t] = corners[t];
    for (int t = threadIdx.x; t < 2 * m; t += blockDim.x) s_xy[t] = boxes[(size_t)(t >> 1) * dim + (t & 1)];
    __syncthreads();
    const int per_pass = max(1, (int)blockDim.x / m);  // tries per pass; thread t tests try t / m against box t % m
    const int jt = (int)threadIdx.x / m, k = (int)threadIdx.x % m;
    for (int i = 0; i < m; ++i) {
        const float bx = s_xy[2 * i], by = s_xy[2 * i + 1];
        float base[4][2];
        os_load4(s_c + 8 * i, base);
        int pick = -1;
        for (int j0 = 0; j0 < num_try && pick < 0; j0 += per_pass) {
            const int j = j0 + jt;
            if (threadIdx.x < per_pass) s_coll[threadIdx.x] = 0;
            __syncthreads();
            float cur[4][2];
            if (jt < per_pass && j < num_try) {
                const size_t ij = (size_t)i * num_try + j;
                os_try_corners(base, bx, by, rot_sc[2 * ij], rot_sc[2 * ij + 1], loc + 3 * ij, cur);
                if (k != i) {
                    float q[4][2];
                    os_load4(s_c + 8 * k, q);
                    if (os_collide(cur, q)) s_coll[jt] = 1;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int p = -1;
                for (int t = 0; t < per_pass && j0 + t < num_try; ++t)
                    if (!s_coll[t]) {
                        p = j0 + t;
                        break;
                    }
                s_pick = p;
            }
            __syncthreads();
            pick = s_pick;
            if (pick >= 0 && jt == pick - j0 && k == 0)  // the moved corners replace the box's (read again only after a barrier)
                for (int c = 0; c < 4; ++c) {
                    s_c[8 * i + 2 * c] = cur[c][0];
                    s_c[8 * i + 2 * c + 1] = cur[c][1];
                }
            __syncthreads();  // s_pick and s_coll are rewritten by the next pass
        }
        if (threadIdx.x == 0) chosen[i] = pick;
    }
}

// points_transform_: a point inside (the original) box b -- the first such box -- becomes
//   float32(float64(((p - centre) @ rot_mat_T) + centre) + loc)  with rot_mat_T the float32 rotation of the chosen angle,
// the angle and loc being 0 for a box without a successful try (the reference transforms those points too, by the identity).
// box3d_transform_: xyz = float32(float64(xyz) + loc), yaw = float32(float64(yaw) + angle); columns past 6 copied.
__global__ __launch_bounds__(256) void srf_object_noise_apply_k(const float *__restrict__ points, int n, int nf,
                                                                const float *__restrict__ boxes, int m, int dim,
                                                                const float *__restrict__ planes, const float *__restrict__ rot_sc,
                                                                const double *__restrict__ rot, const double *__restrict__ loc,
                                                                int num_try, const int *__restrict__ chosen,
                                                                float *__restrict__ out_points, float *__restrict__ out_boxes)
{
    extern __shared__ float s_pl[];
    int *s_mask = (int *)(s_pl + 24 * m);
    os_stage_planes(planes, nullptr, m, s_pl, s_mask);
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        const int j = chosen[i];
        const float *src = boxes + (size_t)i * dim;
        float *dst = out_boxes + (size_t)i * dim;
        const size_t ij = (size_t)i * num_try + (j < 0 ? 0 : j);
        for (int c = 0; c < 3; ++c) dst[c] = __double2float_rn(__dadd_rn((double)src[c], j < 0 ? 0.0 : loc[3 * ij + c]));
        for (int c = 3; c < 6; ++c) dst[c] = src[c];
        dst[6] = __double2float_rn(__dadd_rn((double)src[6], j < 0 ? 0.0 : rot[ij]));
        for (int c = 7; c < dim; ++c) dst[c] = src[c];
    }
    if (i >= n) return;
    const float *src = points + (size_t)i * nf;
    float *dst = out_points + (size_t)i * nf;
    float x = src[0], y = src[1], z = src[2];
    const int b = os_first_box(s_pl, s_mask, m, x, y, z);
    if (b >= 0) {
        const int j = chosen[b];
        const size_t ij = (size_t)b * num_try + (j < 0 ? 0 : j);
        const float s = j < 0 ? 0.0f : rot_sc[2 * ij], c = j < 0 ? 1.0f : rot_sc[2 * ij + 1];
        const float *ctr = boxes + (size_t)b * dim;
        x = __fsub_rn(x, ctr[0]);
        y = __fsub_rn(y, ctr[1]);
        z = __fsub_rn(z, ctr[2]);
        const float ns = -s;  // [x y z] @ [[c, s, 0], [-s, c, 0], [0, 0, 1]], as aug_rotate in augment.hip
        const float nx = __fadd_rn(__fadd_rn(__fmul_rn(x, c), __fmul_rn(y, ns)), __fmul_rn(z, 0.0f));
        const float ny = __fadd_rn(__fadd_rn(__fmul_rn(x, s), __fmul_rn(y, c)), __fmul_rn(z, 0.0f));
        const float nz = __fadd_rn(__fadd_rn(__fmul_rn(x, 0.0f), __fmul_rn(y, 0.0f)), __fmul_rn(z, 1.0f));
        x = __fadd_rn(nx, ctr[0]);
        y = __fadd_rn(ny, ctr[1]);
        z = __fadd_rn(nz, ctr[2]);
        const double lx = j < 0 ? 0.0 : loc[3 * ij], ly = j < 0 ? 0.0 : loc[3 * ij + 1], lz = j < 0 ? 0.0 : loc[3 * ij + 2];
        x = __double2float_rn(__dadd_rn((double)x, lx));
        y = __double2float_rn(__dadd_rn((double)y, ly));
        z = __double2float_rn(__dadd_rn((double)z, lz));
    }
    dst[0] = x;
    dst[1] = y;
    dst[2] = z;
    for (int c = 3; c < nf; ++c) dst[c] = src[c];
}

extern "C" int srf_object_noise(const float *points, int n, int nf, const float *boxes, int m, int box_dim, const float *corners,
                                const float *planes, const float *rot_sc, const double *rot, const double *loc, int num_try,
                                float *out_points, float *out_boxes, int *chosen, srf_stream_t stream)
{
    if (n < 0 || nf < 3 || m < 0 || (box_dim != 7 && box_dim != 9) || num_try < 1) return SRF_EINVAL;
    if (m > SRF_OS_MAX_BOXES) return SRF_EUNSUPPORTED;
    if (n > 0 && (!points || !out_points)) return SRF_EINVAL;
    if (m > 0 && (!boxes || !corners || !planes || !rot_sc || !rot || !loc || !out_boxes || !chosen)) return SRF_EINVAL;
    if (n + (long long)m == 0) return SRF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (m > 0) {
        hipLaunchKernelGGL(srf_object_noise_select_k, dim3(1), dim3(SRF_OS_SEL_THREADS), 0, st, boxes, m, box_dim, corners, rot_sc, loc,
                           num_try, chosen);
        SRF_LAUNCH_CHECK();
    }
    const int rows = n > m ? n : m;
    hipLaunchKernelGGL(srf_object_noise_apply_k, dim3(srf_ceil_div(rows, 256)), dim3(256), os_planes_lds(m), st, points, n, nf, boxes,
                       m, box_dim, planes, rot_sc, rot, loc, num_try, chosen, out_points, out_boxes);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
