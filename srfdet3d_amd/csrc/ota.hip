// ota.hip -- the dynamic-k OTA label assignment of training (OTAssignerSRFDet, ota_srfdet.py:18-327) for gfx950: every decoder stage
// and every sample of a step in ONE call, two launches, nothing read back inside the call.
//
// srfdet3d_amd/plugin/training.py restates the assigner op by op in torch (about 60 launches and five host synchronisations per stage and
// sample); tests/ota_ref.py is the text below in numpy.
//
// DEFINITION.  All arithmetic is f32, one rounding per operation, never an fma; a + b + c means (a + b) + c.  For stage s, sample b, with
// n = n_gt[b] live ground-truth boxes (columns g >= n are never read and never written), prediction row q = pred_boxes[s, b, p, 0..7] =
// [x, y, z, log w, log l, log h, sin, cos], ground truth t = gt_boxes[b, g] = [x, y, z, dx, dy, dz, yaw], class L = gt_labels[b, g]
// (clamped into [0, C)) and logit v = pred_logits[s, b, p, L]:
//   in box      the axis-aligned bounds of the eight corners boxes3d_to_corners3d(ry=True, bottom_center=False) gives for t -- which takes
//               exp() of the three sizes, as the reference does: half sizes hw = expf(dx) / 2, hl = expf(dy) / 2, hh = expf(dz) / 2, corners
//               (t.x + (sx hw cos + sy hl sin), t.y + (sx hw (-sin) + sy hl cos), t.z -+ hh) over the four sign pairs, cos / sin = cosf / sinf of
//               the yaw; in_box = lo < q.xyz < hi on all three axes, strict
//   in centre   r = center_radius * t.dxyz;  in_ctr = t.xyz - r < q.xyz < t.xyz + r on all three axes, strict
//   valid(p)    = OR over g < n of (in_box | in_ctr);   in_both(p, g) = in_box & in_ctr
//   focal cost  pr = 1 / (1 + expf(-v));  neg = (-logf((1 - pr) + eps)) * (1 - alpha) * pr^gamma;  pos = (-logf(pr + eps)) * alpha * (1 - pr)^gamma;
//               cls = (pos - neg) * w_cls;  x^gamma is x * x for gamma == 2 and powf otherwise;  1 - alpha is rounded once from float64
//   L1 cost     reg = (sum over k = 0..7 ascending of |q[k] - tn[k]|) * w_reg,  tn = [t.x, t.y, t.z, logf(dx), logf(dy), logf(dz), sinf(yaw), cosf(yaw)]
//   3-D IoU     bbox_overlaps_3d of (x, y, z, w = expf(q[3]), l = expf(q[4]), h = expf(q[5]), atan2f(q[6], q[7])) and t:
//               hgt = max(min(q.z + h, t.z + dz) - max(q.z, t.z), 0);  BEV sizes clamped at 1e-4;  u = srf_rotated_iou(BEV of q, BEV of t);
//               a1, a2 the clamped BEV areas;  inter = u * (a1 + a2) / (1 + u) * hgt;  vol = w * l * h + dx * dy * dz (sizes unclamped);
//               iou = inter / max(vol - inter, 1e-8)
//   cost        = ((cls + reg) + (-w_iou * iou)) + (in_both ? 0 : 100),  then + 10000 on every row that is not valid
// and on those two matrices (`_dynamic_k` as written in training.py, quirks included; NaN orders as +inf, -0 equals +0):
//   dynamic k   ks[g] = max(1, trunc(sum - 0.5 (num_heads - head_idx[s]))), sum = the min(topk, P) largest iou[:, g] added in descending order from 0
//   by rank     p matches g when fewer than ks[g] rows come before it in the ascending order of cost[:, g], lower index first on ties
//   multi       rows with more than one match keep only their arg-min column over ALL g < n (lower index on ties); these rows are the FIRST
//               multi mask
//   repair      for it = 0, 1, ...: stop when every column g < n has a match; when it == 32 set status = 1 and stop (the state stays as it is);
//               otherwise add 100000 to every cost of every matched row (an f32 add: it absorbs low bits), then every unmatched column takes the
//               arg-min row of its column (lower index on ties), then, if any row has more than one match, every row of the FIRST multi mask --
//               and no other -- is reset to its arg-min column on the updated costs
//   output      the rows with a match in ascending order in pred_idx[0..count), gt_idx = the first matched column of each; the slots from count
//               on hold -1.  n == 0: count = 0, status = 0.
// No float atomics and a fixed order everywhere: two calls give the same bytes.
//
// SHAPE.  cost / iou / match live in the caller's workspace g-major, (S, B, Gpad, P): everything the matching does many times walks a column
// (top-k, rank, arg-min, column count), and with the column contiguous a wave reads it in 256-byte runs; the walks over a row are one
// thread per row, so neighbouring lanes read neighbouring addresses there as well.
// srf_ota_cost_k: workgroups of 4 waves, one per (s, b, 64 rows); a lane keeps its prediction row in registers and wave w takes the columns
// w, w + 4, ...; `valid` is the OR of a lane's own columns and of the four waves through 1 KB of LDS, and the 10000 is added by the thread
// that wrote the cost.  At config 4 (S 6, B 2, P 900, 20-40 boxes) that is 180 workgroups and about ten pairs per thread.
// srf_ota_match_k: one workgroup of 16 waves per (s, b).  A wave per column: every pick is one walk over the column and one wave arg-min of
// (value, index) pairs; the pick after (v, i) is the smallest pair behind it in the total order, so no "taken" set is kept.  Row walks,
// the +100000 and the compaction are a thread per row.  Global memory written by one wave is read by another only across __syncthreads().
// The stage is launch- and latency-bound (1.4 M pairs per step): no LDS tiling of the matrices, which do not fit (5.5 MB).
#include "common.hpp"
#include "rotated_iou.hpp"

#include <limits.h>

#define SRF_OTA_MAX_P 4096      // s_multi, one byte per row
#define SRF_OTA_MAX_G 512       // s_col, one int per column
#define SRF_OTA_CAP 32          // iterations of the repair loop
#define SRF_OTA_COST_THREADS 256
#define SRF_OTA_MATCH_THREADS 1024

struct OtaCostArgs {
    const float *pred_boxes, *pred_logits, *gt_boxes;
    const int *gt_labels, *n_gt;
    int S, B, P, D, C, G;
    float w_cls, w_reg, w_iou, alpha, one_minus_alpha, gamma, eps, radius;
    float *cost, *iou;
};

struct OtaMatchArgs {
    float *cost;
    const float *iou;
    unsigned char *match;
    const int *n_gt, *head_idx;
    int S, B, P, G, topk, num_heads;
    int *count, *pred_idx, *gt_idx, *status;
};

__device__ __forceinline__ int srf_ota_live(const int *n_gt, int b, int G)
{
    const int n = n_gt[b];
    return n < 0 ? 0 : (n > G ? G : n);
}

__device__ __forceinline__ float srf_ota_pow(float x, float gamma) { return gamma == 2.0f ? x * x : powf(x, gamma); }

__global__ __launch_bounds__(SRF_OTA_COST_THREADS) void srf_ota_cost_k(OtaCostArgs a)
{
    __shared__ int s_any[SRF_OTA_COST_THREADS / 64][64];
    const int tiles = (a.P + 63) / 64;
    const int sb = blockIdx.x / tiles, tile = blockIdx.x - sb * tiles;
    const int b = sb % a.B;
    const int ng = srf_ota_live(a.n_gt, b, a.G);
    if (ng == 0) return;   // the whole workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = tile * 64 + lane;
    const bool live = p < a.P;
    const size_t base = (size_t)sb * a.G * a.P + (live ? p : 0);

    int any = 0;
    if (live) {
        const float *q = a.pred_boxes + ((size_t)sb * a.P + p) * a.D;
        const float *lg = a.pred_logits + ((size_t)sb * a.P + p) * a.C;
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = q[k];
        const float w = expf(r[3]), l = expf(r[4]), h = expf(r[5]);
        float bev1[5] = {r[0], r[1], fmaxf(w, 1e-4f), fmaxf(l, 1e-4f), atan2f(r[6], r[7])};
        const float a1 = bev1[2] * bev1[3], v1 = w * l * h, top1 = r[2] + h;

        for (int g = wave; g < ng; g += SRF_OTA_COST_THREADS / 64) {
            const float *t = a.gt_boxes + ((size_t)b * a.G + g) * 7;
            const float gx = t[0], gy = t[1], gz = t[2], dx = t[3], dy = t[4], dz = t[5], yaw = t[6];
            const float cy = cosf(yaw), sy = sinf(yaw);
            // the corners' bounds (the sizes go through exp(), as in the reference's call of boxes3d_to_corners3d)
            const float hw = expf(dx) / 2.0f, hl = expf(dy) / 2.0f, hh = expf(dz) / 2.0f;
            float lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xc = (c == 0 || c == 3) ? hw : -hw, yc = c >= 2 ? hl : -hl;
                const float X = gx + (xc * cy + yc * sy), Y = gy + (xc * (-sy) + yc * cy);
                lox = fminf(lox, X), hix = fmaxf(hix, X), loy = fminf(loy, Y), hiy = fmaxf(hiy, Y);
            }
            const float loz = fminf(gz + (-hh), gz + hh), hiz = fmaxf(gz + (-hh), gz + hh);
            const bool in_box = r[0] > lox && r[0] < hix && r[1] > loy && r[1] < hiy && r[2] > loz && r[2] < hiz;
            const float rx = a.radius * dx, ry = a.radius * dy, rz = a.radius * dz;
            const bool in_ctr = r[0] > gx - rx && r[0] < gx + rx && r[1] > gy - ry && r[1] < gy + ry && r[2] > gz - rz && r[2] < gz + rz;
            any |= (in_box || in_ctr) ? 1 : 0;

            int lab = a.gt_labels[(size_t)b * a.G + g];
            lab = lab < 0 ? 0 : (lab >= a.C ? a.C - 1 : lab);
            const float pr = 1.0f / (1.0f + expf(-lg[lab]));
            const float neg = (-logf((1.0f - pr) + a.eps)) * a.one_minus_alpha * srf_ota_pow(pr, a.gamma);
            const float pos = (-logf(pr + a.eps)) * a.alpha * srf_ota_pow(1.0f - pr, a.gamma);
            const float cls = (pos - neg) * a.w_cls;

            const float tn[8] = {gx, gy, gz, logf(dx), logf(dy), logf(dz), sy, cy};
            float l1 = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) l1 = l1 + fabsf(r[k] - tn[k]);
            const float reg = l1 * a.w_reg;

            float bev2[5] = {gx, gy, fmaxf(dx, 1e-4f), fmaxf(dy, 1e-4f), yaw};
            const float u = srf_rotated_iou(bev1, bev2);
            const float hgt = fmaxf(fminf(top1, gz + dz) - fmaxf(r[2], gz), 0.0f);
            const float a2 = bev2[2] * bev2[3];
            const float inter = u * (a1 + a2) / (1.0f + u) * hgt;
            const float v2 = dx * dy * dz;
            const float iou = inter / fmaxf((v1 + v2) - inter, 1e-8f);

            const float cost = ((cls + reg) + (-a.w_iou * iou)) + ((in_box && in_ctr) ? 0.0f : 100.0f);
            a.cost[base + (size_t)g * a.P] = cost;
            a.iou[base + (size_t)g * a.P] = iou;
        }
    }
    s_any[wave][lane] = any;
    __syncthreads();
    if (!live) return;
    int valid = 0;
#pragma unroll
    for (int w = 0; w < SRF_OTA_COST_THREADS / 64; ++w) valid |= s_any[w][lane];
    if (!valid)
        for (int g = wave; g < ng; g += SRF_OTA_COST_THREADS / 64) {   // this thread's own stores
            float *c = a.cost + base + (size_t)g * a.P;
            *c = *c + 10000.0f;
        }
}

// NaN orders as +inf
__device__ __forceinline__ float srf_ota_key(float v) { return v != v ? INFINITY : v; }

// (v, i) comes before (w, j): smaller value first, lower index on ties
__device__ __forceinline__ bool srf_ota_before(float v, int i, float w, int j) { return v < w || (v == w && i < j); }

// The first pair behind (pv, pi) in the ascending order of the column col[0..P) (values negated when `negate`: descending order of the
// column), over the wave; i == INT_MAX when there is none.  The same (v, i) in every lane.
__device__ __forceinline__ void srf_ota_next(const float *col, int P, bool negate, float pv, int pi, float &v, int &i)
{
    const int lane = threadIdx.x & 63;
    float bv = INFINITY;
    int bi = INT_MAX;
    for (int p = lane; p < P; p += 64) {
        float x = col[p];
        x = srf_ota_key(negate ? -x : x);
        if (srf_ota_before(pv, pi, x, p) && srf_ota_before(x, p, bv, bi)) {
            bv = x;
            bi = p;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (srf_ota_before(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    v = bv;
    i = bi;
}

// row p keeps only its arg-min column over g < ng (lower index on ties)
__device__ __forceinline__ void srf_ota_keep_best(const float *cost, unsigned char *match, int P, int ng, int p)
{
    float bv = srf_ota_key(cost[p]);
    int bg = 0;
    for (int g = 1; g < ng; ++g) {
        const float v = srf_ota_key(cost[(size_t)g * P + p]);
        if (v < bv) {
            bv = v;
            bg = g;
        }
    }
    for (int g = 0; g < ng; ++g) match[(size_t)g * P + p] = g == bg ? 1 : 0;
}

__device__ __forceinline__ int srf_ota_row_count(const unsigned char *match, int P, int ng, int p)
{
    int c = 0;
    for (int g = 0; g < ng; ++g) c += match[(size_t)g * P + p];
    return c;
}

// exclusive scan of one flag per thread over the workgroup (thread order) and the workgroup's total
__device__ __forceinline__ int srf_ota_scan(int v, int *s_w, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = srf_wave_inclusive_scan(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SRF_OTA_MATCH_THREADS / 64; ++w) {
        const int c = s_w[w];
        before += w < wave ? c : 0;
        tot += c;
    }
    total = tot;
    __syncthreads();
    return before + inc - v;
}

// cost and match are read and written by different waves of the workgroup across barriers: no __restrict__ on them
__global__ __launch_bounds__(SRF_OTA_MATCH_THREADS) void srf_ota_match_k(OtaMatchArgs a)
{
    constexpr int T = SRF_OTA_MATCH_THREADS, W = T / 64;
    __shared__ unsigned char s_multi[SRF_OTA_MAX_P];
    __shared__ int s_col[SRF_OTA_MAX_G];
    __shared__ int s_w[W];
    const int sb = blockIdx.x, s = sb / a.B, b = sb - s * a.B;
    const int P = a.P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = srf_ota_live(a.n_gt, b, a.G);
    float *cost = a.cost + (size_t)sb * a.G * P;
    const float *iou = a.iou + (size_t)sb * a.G * P;
    unsigned char *match = a.match + (size_t)sb * a.G * P;
    int *pidx = a.pred_idx + (size_t)sb * P, *gidx = a.gt_idx + (size_t)sb * P;

    if (ng == 0) {   // the whole workgroup
        for (int p = tid; p < P; p += T) pidx[p] = gidx[p] = -1;
        if (tid == 0) a.count[sb] = 0, a.status[sb] = 0;
        return;
    }
    for (int t = tid; t < ng * P; t += T) match[t] = 0;
    __syncthreads();

    // dynamic k and the matching by rank, a wave per column
    const float shift = 0.5f * (float)(a.num_heads - a.head_idx[s]);
    const int cand = a.topk < P ? a.topk : P;
    for (int g = wave; g < ng; g += W) {
        const float *ucol = iou + (size_t)g * P;
        float sum = 0.0f, pv = -INFINITY;
        int pi = -1;
        for (int k = 0; k < cand; ++k) {
            float v;
            int i;
            srf_ota_next(ucol, P, true, pv, pi, v, i);
            if (i == INT_MAX) break;
            sum = sum + (-v);
            pv = v, pi = i;
        }
        const float kf = sum - shift;
        const int ks = kf >= (float)P ? P : (kf >= 1.0f ? (int)kf : 1);
        const float *ccol = cost + (size_t)g * P;
        pv = -INFINITY, pi = -1;
        for (int k = 0; k < ks; ++k) {
            float v;
            int i;
            srf_ota_next(ccol, P, false, pv, pi, v, i);
            if (i == INT_MAX) break;
            if (lane == 0) match[(size_t)g * P + i] = 1;
            pv = v, pi = i;
        }
    }
    __syncthreads();

    // rows with more than one match keep their best column; they are the FIRST multi mask
    for (int p = tid; p < P; p += T) {
        const bool m = srf_ota_row_count(match, P, ng, p) > 1;
        s_multi[p] = m ? 1 : 0;
        if (m) srf_ota_keep_best(cost, match, P, ng, p);
    }
    __syncthreads();

    int status = 0;
    for (int it = 0;; ++it) {
        int open = 0;
        for (int g = wave; g < ng; g += W) {
            int c = 0;
            for (int p = lane; p < P; p += 64) c += match[(size_t)g * P + p];
            c = srf_wave_sum(c);
            if (lane == 0) s_col[g] = c;
            open |= c == 0 ? 1 : 0;
        }
        if (!__syncthreads_or(open)) break;
        if (it == SRF_OTA_CAP) {
            status = 1;
            break;
        }
        for (int p = tid; p < P; p += T)
            if (srf_ota_row_count(match, P, ng, p) > 0)
                for (int g = 0; g < ng; ++g) cost[(size_t)g * P + p] = cost[(size_t)g * P + p] + 100000.0f;
        __syncthreads();
        for (int g = wave; g < ng; g += W) {
            if (s_col[g] != 0) continue;
            float v;
            int i;
            srf_ota_next(cost + (size_t)g * P, P, false, -INFINITY, -1, v, i);
            if (lane == 0 && i != INT_MAX) match[(size_t)g * P + i] = 1;
        }
        __syncthreads();
        int more = 0;
        for (int p = tid; p < P; p += T) more |= srf_ota_row_count(match, P, ng, p) > 1 ? 1 : 0;
        if (__syncthreads_or(more))
            for (int p = tid; p < P; p += T)
                if (s_multi[p]) srf_ota_keep_best(cost, match, P, ng, p);
        __syncthreads();
    }

    // the matched rows in ascending order, each with its first matched column
    int carry = 0;
    for (int p0 = 0; p0 < P; p0 += T) {   // uniform trip count
        const int p = p0 + tid;
        int first = -1;
        if (p < P)
            for (int g = ng - 1; g >= 0; --g) first = match[(size_t)g * P + p] ? g : first;
        int tot;
        const int ex = srf_ota_scan(first >= 0 ? 1 : 0, s_w, tot);
        if (first >= 0) {
            pidx[carry + ex] = p;
            gidx[carry + ex] = first;
        }
        carry += tot;
    }
    for (int t = carry + tid; t < P; t += T) pidx[t] = gidx[t] = -1;
    if (tid == 0) a.count[sb] = carry, a.status[sb] = status;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
static bool srf_ota_fits(long long a, long long b, long long c, long long d) { return a * b * c * d < (1ll << 31) / 4; }

static int srf_ota_shape(int S, int B, int P, int Gpad)
{
    if (S <= 0 || B <= 0 || P <= 0 || Gpad <= 0) return SRF_EINVAL;
    return SRF_OK;
}

static int srf_ota_shape_limits(int S, int B, int P, int Gpad)
{
    if (P > SRF_OTA_MAX_P || Gpad > SRF_OTA_MAX_G || (long long)S * B > 65535 || !srf_ota_fits(S, B, P, Gpad)) return SRF_EUNSUPPORTED;
    return SRF_OK;
}

static size_t srf_ota_matrix(int S, int B, int P, int Gpad) { return (size_t)S * B * P * Gpad; }

extern "C" size_t srf_ota_match_workspace_bytes(int S, int B, int P, int Gpad)
{
    if (srf_ota_shape(S, B, P, Gpad) != SRF_OK || srf_ota_shape_limits(S, B, P, Gpad) != SRF_OK) return 0;
    return srf_align256(srf_ota_matrix(S, B, P, Gpad));
}

extern "C" size_t srf_ota_workspace_bytes(int S, int B, int P, int Gpad)
{
    if (srf_ota_shape(S, B, P, Gpad) != SRF_OK || srf_ota_shape_limits(S, B, P, Gpad) != SRF_OK) return 0;
    return 2 * srf_align256(srf_ota_matrix(S, B, P, Gpad) * sizeof(float)) + srf_ota_match_workspace_bytes(S, B, P, Gpad);
}

static int srf_ota_cost_check(const float *pred_boxes, const float *pred_logits, const float *gt_boxes, const int *gt_labels, const int *n_gt,
                              int S, int B, int P, int D, int C, int Gpad)
{
    if (srf_ota_shape(S, B, P, Gpad) != SRF_OK || D <= 0 || C <= 0) return SRF_EINVAL;
    if (!pred_boxes || !pred_logits || !gt_boxes || !gt_labels || !n_gt) return SRF_EINVAL;
    if (srf_ota_shape_limits(S, B, P, Gpad) != SRF_OK || (D != 8 && D != 10) || C > 64 || !srf_ota_fits(S, B, P, C)) return SRF_EUNSUPPORTED;
    return SRF_OK;
}

static void srf_ota_launch_cost(const float *pred_boxes, const float *pred_logits, const float *gt_boxes, const int *gt_labels, const int *n_gt,
                                int S, int B, int P, int D, int C, int Gpad, float w_cls, float w_reg, float w_iou, float alpha, float gamma,
                                float eps, float center_radius, float *cost, float *iou, hipStream_t st)
{
    OtaCostArgs a;
    a.pred_boxes = pred_boxes, a.pred_logits = pred_logits, a.gt_boxes = gt_boxes, a.gt_labels = gt_labels, a.n_gt = n_gt;
    a.S = S, a.B = B, a.P = P, a.D = D, a.C = C, a.G = Gpad;
    a.w_cls = w_cls, a.w_reg = w_reg, a.w_iou = w_iou, a.alpha = alpha, a.one_minus_alpha = (float)(1.0 - (double)alpha), a.gamma = gamma;
    a.eps = eps, a.radius = center_radius;
    a.cost = cost, a.iou = iou;
    hipLaunchKernelGGL(srf_ota_cost_k, dim3(S * B * ((P + 63) / 64)), dim3(SRF_OTA_COST_THREADS), 0, st, a);
}

static void srf_ota_launch_match(float *cost, const float *iou, unsigned char *match, const int *n_gt, const int *head_idx, int S, int B, int P,
                                 int Gpad, int topk, int num_heads, int *count, int *pred_idx, int *gt_idx, int *status, hipStream_t st)
{
    OtaMatchArgs a;
    a.cost = cost, a.iou = iou, a.match = match, a.n_gt = n_gt, a.head_idx = head_idx;
    a.S = S, a.B = B, a.P = P, a.G = Gpad, a.topk = topk, a.num_heads = num_heads;
    a.count = count, a.pred_idx = pred_idx, a.gt_idx = gt_idx, a.status = status;
    hipLaunchKernelGGL(srf_ota_match_k, dim3(S * B), dim3(SRF_OTA_MATCH_THREADS), 0, st, a);
}

extern "C" int srf_ota_cost(const float *pred_boxes, const float *pred_logits, const float *gt_boxes, const int *gt_labels, const int *n_gt, int S,
                            int B, int P, int D, int C, int Gpad, float w_cls, float w_reg, float w_iou, float alpha, float gamma, float eps,
                            float center_radius, float *cost, float *iou, srf_stream_t stream)
{
    const int rc = srf_ota_cost_check(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, S, B, P, D, C, Gpad);
    if (rc == SRF_EINVAL || !cost || !iou) return SRF_EINVAL;
    if (rc != SRF_OK) return rc;
    srf_ota_launch_cost(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, S, B, P, D, C, Gpad, w_cls, w_reg, w_iou, alpha, gamma, eps,
                        center_radius, cost, iou, (hipStream_t)stream);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

extern "C" int srf_ota_match(float *cost, const float *iou, const int *n_gt, const int *head_idx, int S, int B, int P, int Gpad,
                             int candidate_topk, int num_heads, int *count, int *pred_idx, int *gt_idx, int *status, void *workspace,
                             size_t workspace_bytes, srf_stream_t stream)
{
    if (srf_ota_shape(S, B, P, Gpad) != SRF_OK || candidate_topk <= 0) return SRF_EINVAL;
    if (!cost || !iou || !n_gt || !head_idx || !count || !pred_idx || !gt_idx || !status || !workspace) return SRF_EINVAL;
    if (srf_ota_shape_limits(S, B, P, Gpad) != SRF_OK) return SRF_EUNSUPPORTED;
    if (workspace_bytes < srf_ota_match_workspace_bytes(S, B, P, Gpad)) return SRF_EWORKSPACE;
    srf_ota_launch_match(cost, iou, (unsigned char *)workspace, n_gt, head_idx, S, B, P, Gpad, candidate_topk, num_heads, count, pred_idx, gt_idx,
                         status, (hipStream_t)stream);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}

extern "C" int srf_ota_assign(const float *pred_boxes, const float *pred_logits, const float *gt_boxes, const int *gt_labels, const int *n_gt,
                              const int *head_idx, int S, int B, int P, int D, int C, int Gpad, float w_cls, float w_reg, float w_iou, float alpha,
                              float gamma, float eps, float center_radius, int candidate_topk, int num_heads, int *count, int *pred_idx,
                              int *gt_idx, int *status, void *workspace, size_t workspace_bytes, srf_stream_t stream)
{
    const int rc = srf_ota_cost_check(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, S, B, P, D, C, Gpad);
    if (rc == SRF_EINVAL || candidate_topk <= 0) return SRF_EINVAL;
    if (!head_idx || !count || !pred_idx || !gt_idx || !status || !workspace) return SRF_EINVAL;
    if (rc != SRF_OK) return rc;
    if (workspace_bytes < srf_ota_workspace_bytes(S, B, P, Gpad)) return SRF_EWORKSPACE;
    const size_t mat = srf_align256(srf_ota_matrix(S, B, P, Gpad) * sizeof(float));
    float *cost = (float *)workspace, *iou = (float *)((char *)workspace + mat);
    unsigned char *match = (unsigned char *)workspace + 2 * mat;
    hipStream_t st = (hipStream_t)stream;
    srf_ota_launch_cost(pred_boxes, pred_logits, gt_boxes, gt_labels, n_gt, S, B, P, D, C, Gpad, w_cls, w_reg, w_iou, alpha, gamma, eps,
                        center_radius, cost, iou, st);
    srf_ota_launch_match(cost, iou, match, n_gt, head_idx, S, B, P, Gpad, candidate_topk, num_heads, count, pred_idx, gt_idx, status, st);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
