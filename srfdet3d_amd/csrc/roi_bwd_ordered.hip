// roi_bwd_ordered.hip -- srf_roi_extract_bwd_ordered: the gradient of the multi-level RoIAlign gather w.r.t. its feature maps with
// the adds of every map element in a FIXED order (gfx950).  srf_roi_extract_bwd (roi.hip) adds the same terms with float atomics, in
// whatever order they arrive; here two calls give the same bytes.  Training takes this entry under SRF_DETERMINISTIC=1.
//
// Definition (tests/roi_bwd_ordered_ref.py is the same text in numpy float32, operation by operation):
//   * A record is (RoI r, output row ph, column pw, sample iy, ix, tap t in 0..3); the taps are ordered (y_low, x_low), (y_low, x_high),
//     (y_high, x_low), (y_high, x_high).  Its slot is ((((r P + ph) P + pw) sr + iy) sr + ix) 4 + t, P = pooled: ascending slot is
//     ascending (r, ph, pw, iy, ix, t).
//   * Level, sample point, validity and the f32 weights are those of srf_roi_extract_bwd_k: the same __f*_rn sequence for the sample
//     point, the clamps of mmcv, ly = y - y_low, hy = 1 - ly (likewise x), w = hy hx, hy lx, ly hx, ly lx.
//   * A record with w == 0, with a sample that is NaN or outside [-1, H] x [-1, W], or with a batch id outside [0, N) contributes nothing.
//   * For every element (level, n, y, x, c) touched by at least one record:
//         acc = +0;  for the element's records in ascending slot:  acc = __fadd_rn(acc, __fmul_rn(w, __fmul_rn(gout[r][bin][c], 1.0f / (sr sr))))
//     and the element is STORED.  An element without a record is left as the caller passed it (the caller zero-fills).
//   The terms are the atomic kernel's own terms; only the order of the adds is fixed.
//
// Keys.  A record's key is level_base[level] + (n H + y) W + x with level_base the running sum of N H W over the levels; "no
// contribution" is the key T = the sum over all levels, which sorts last.  Keys are 30 bits wide: a call whose levels hold 2^30 pixels or
// more between them (and so any level that does on its own) is SRF_EUNSUPPORTED before any launch, as is R > 2^24 or more than 2^30
// records.  (Config 4's finest level is 12 x 232 x 400 = 1.1 M pixels, 21 bits.)
//
// Kernels, all on the caller's stream, nothing read back:
//   (a) srf_roi_ord_records_k  one thread per (RoI, sample): level, sample point and the four taps -> keys[slot], weights[slot].
//   (b) a stable LSD radix sort of (key, slot) by key, 8 bits a pass over the significant bits of T only (3 passes for config 4).  A pass
//       is: per-block digit counts (integer LDS atomics: a count does not depend on arrival order) -> exclusive scan of the (digit, block)
//       table (srf_device_scan) -> scatter, where a record's rank among its block's records of the same digit is taken in index order
//       (ballot match inside the wave, wave and round counts through LDS).  Stable, so equal keys stay in ascending slot.
//   (c) segment heads by comparing neighbouring keys, compacted by srf_device_scan; the same pass writes each sorted record's
//       (r, bin) and weight into the sort's free ping-pong buffers, so that (d) reads 8 contiguous bytes per record.
//   (d) srf_roi_ord_reduce_k  one wave per (destination pixel, 256 channels): lanes own four channels (one float4 on channels-last maps
//       with a channel-contiguous grad_out, four strided scalars otherwise); the segment's (source row, weight) pairs are read
//       wave-uniformly; the grad_out rows of four records are requested before the four dependent adds; plain stores.
// No float atomic anywhere.  (b)-(d) is a segmented fixed-order reduction over (key, source) pairs: the primitive a fixed-order
// srf_msda_bwd would reuse with key = value row.
#include "roi_frame.hpp"

#define ORD_TILE_ITEMS 16
#define ORD_TILE (256 * ORD_TILE_ITEMS)
#define ORD_KEY_BITS 30
#define ORD_MAX_R (1 << 24)
#define ORD_MAX_RECORDS (1LL << 30)
#define ORD_REDUCE_BLOCKS 2048

struct OrdGeom {
    unsigned base[SRF_MAX_LEVELS + 1];   // base[l] = sum of N H W of the levels below l; base[SRF_MAX_LEVELS] = T
};

// ----------------------------------------------------------------------------------------------------------------- (a) records
__global__ __launch_bounds__(256) void srf_roi_ord_records_k(RoiLevels L, OrdGeom Gm, const float *__restrict__ rois, int R, int pooled, int sr,
                                                            float finest_scale, unsigned *__restrict__ keys, float *__restrict__ wts)
{
    const int per_roi = pooled * pooled * sr * sr;
    const long long tidx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tidx >= (long long)R * per_roi) return;
    const int r = (int)(tidx / per_roi);
    int q = (int)(tidx - (long long)r * per_roi);
    const int ix = q % sr;
    q /= sr;
    const int iy = q % sr;
    q /= sr;
    const int pw = q % pooled, ph = q / pooled;
    const float *b = rois + (size_t)r * 5;
    const int lvl = srf_roi_level(b, L.num, finest_scale);
    const srf_featmap f = L.lv[lvl];
    const int n = (int)b[0];
    const bool valid_n = n >= 0 && n < f.N;
    // the sample point: the statements of srf_roi_extract_bwd_k
    const float x1 = __fsub_rn(__fmul_rn(b[1], f.spatial_scale), 0.5f), y1 = __fsub_rn(__fmul_rn(b[2], f.spatial_scale), 0.5f);
    const float x2 = __fsub_rn(__fmul_rn(b[3], f.spatial_scale), 0.5f), y2 = __fsub_rn(__fmul_rn(b[4], f.spatial_scale), 0.5f);
    const float bin_h = __fdiv_rn(__fsub_rn(y2, y1), (float)pooled), bin_w = __fdiv_rn(__fsub_rn(x2, x1), (float)pooled);
    float y = __fadd_rn(__fadd_rn(y1, __fmul_rn((float)ph, bin_h)), __fdiv_rn(__fmul_rn(__fadd_rn((float)iy, 0.5f), bin_h), (float)sr));
    float x = __fadd_rn(__fadd_rn(x1, __fmul_rn((float)pw, bin_w)), __fdiv_rn(__fmul_rn(__fadd_rn((float)ix, 0.5f), bin_w), (float)sr));
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned pix[4] = {0u, 0u, 0u, 0u};
    const int H = f.H, W = f.W;
    if (valid_n && !(y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) && (y == y) && (x == x)) {
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
        const float ly = __fsub_rn(y, (float)y_low), lx = __fsub_rn(x, (float)x_low);
        const float hy = __fsub_rn(1.0f, ly), hx = __fsub_rn(1.0f, lx);
        w[0] = __fmul_rn(hy, hx);
        w[1] = __fmul_rn(hy, lx);
        w[2] = __fmul_rn(ly, hx);
        w[3] = __fmul_rn(ly, lx);
        const unsigned row_lo = ((unsigned)n * H + y_low) * W, row_hi = ((unsigned)n * H + y_high) * W;
        pix[0] = row_lo + x_low;
        pix[1] = row_lo + x_high;
        pix[2] = row_hi + x_low;
        pix[3] = row_hi + x_high;
    }
    const unsigned T = Gm.base[SRF_MAX_LEVELS];
    uint4 k;
    k.x = w[0] != 0.f ? Gm.base[lvl] + pix[0] : T;
    k.y = w[1] != 0.f ? Gm.base[lvl] + pix[1] : T;
    k.z = w[2] != 0.f ? Gm.base[lvl] + pix[2] : T;
    k.w = w[3] != 0.f ? Gm.base[lvl] + pix[3] : T;
    reinterpret_cast<uint4 *>(keys)[tidx] = k;                      // slots 4 tidx .. 4 tidx + 3: the buffers are 256-byte aligned
    reinterpret_cast<float4 *>(wts)[tidx] = make_float4(w[0], w[1], w[2], w[3]);
}

// ----------------------------------------------------------------------------------------------------------------- (b) radix pass
// hist[d * nblk + block] = records of the block's tile whose digit is d
__global__ __launch_bounds__(256) void srf_roi_ord_hist_k(const unsigned *__restrict__ keys, int n, int shift, int nblk, int *__restrict__ hist)
{
    __shared__ int s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * ORD_TILE;
#pragma unroll
    for (int q = 0; q < ORD_TILE_ITEMS; ++q) {
        const long long i = base + q * 256 + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(keys[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}

struct OrdHistVal {
    const int *h;
    __device__ int operator()(int i) const { return h[i]; }
};
struct OrdHistOut {
    int *h;
    __device__ void operator()(int i, int, int prefix) const { h[i] = prefix; }
};

// offs[d * nblk + block] = first output position of the block's records of digit d.  in_vals == NULL: the value of record i is i.
__global__ __launch_bounds__(256) void srf_roi_ord_scatter_k(const unsigned *__restrict__ in_keys, const unsigned *__restrict__ in_vals, int n,
                                                            int shift, int nblk, const int *__restrict__ offs,
                                                            unsigned *__restrict__ out_keys, unsigned *__restrict__ out_vals)
{
    __shared__ int s_base[256];
    __shared__ int s_cnt[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = offs[(size_t)tid * nblk + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) s_cnt[w][tid] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * ORD_TILE;
    for (int q = 0; q < ORD_TILE_ITEMS; ++q) {   // block-uniform trip count
        const long long i = base + q * 256 + tid;
        const bool active = i < n;
        const unsigned key = active ? in_keys[i] : 0u;
        const unsigned val = active ? (in_vals ? in_vals[i] : (unsigned)i) : 0u;
        const unsigned d = (key >> shift) & 255u;
        // the lanes of this wave that hold the same digit
        unsigned long long m = __ballot(active);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = __ballot(active && bit);
            m &= bit ? bb : ~bb;
        }
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (active && rank == 0) s_cnt[wave][d] = __popcll(m);
        __syncthreads();
        if (active) {
            int pos = s_base[d] + rank;
#pragma unroll
            for (int w = 0; w < 3; ++w) pos += w < wave ? s_cnt[w][d] : 0;
            if (pos >= 0 && pos < n) {
                out_keys[pos] = key;
                out_vals[pos] = val;
            }
        }
        __syncthreads();
        s_base[tid] += s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
#pragma unroll
        for (int w = 0; w < 4; ++w) s_cnt[w][tid] = 0;
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------------------------------- (c) segments
struct OrdHeadVal {
    const unsigned *k;
    __device__ int operator()(int i) const { return (i == 0 || k[i] != k[i - 1]) ? 1 : 0; }
};
struct OrdHeadOut {
    const unsigned *slot;    // sorted
    const float *wts;        // by slot
    int *seg_start;
    unsigned *src;           // (r << 6) | bin of sorted record i
    float *w;                // its weight
    int per_bin, bins;       // 4 sr sr, pooled pooled
    unsigned n;              // records
    __device__ void operator()(int i, int v, int prefix) const
    {
        if (v) seg_start[prefix] = i;
        const unsigned s = min(slot[i], n - 1u);   // a slot is below n by construction; the clamp keeps every later read inside its buffer
        const unsigned rb = s / (unsigned)per_bin;
        const unsigned r = rb / (unsigned)bins;
        src[i] = (r << 6) | (rb - r * (unsigned)bins);
        w[i] = wts[s];
    }
};

// ----------------------------------------------------------------------------------------------------------------- (d) reduce
template <bool VEC>
__global__ __launch_bounds__(256) void srf_roi_ord_reduce_k(RoiLevels L, RoiGradLevels G, OrdGeom Gm, int C, int n, const int *__restrict__ nseg_p,
                                                           const int *__restrict__ seg_start, const unsigned *__restrict__ keys,
                                                           const unsigned *__restrict__ src, const float *__restrict__ wsrt, int sr,
                                                           const float *__restrict__ gout, long long so_r, long long so_c, long long so_b)
{
    const int lane = threadIdx.x & 63;
    const int nchunk = (C + 255) >> 8;
    const int nseg = *nseg_p;
    const long long items = (long long)nseg * nchunk;
    const long long stride = (long long)gridDim.x * 4;
    const float inv = 1.0f / (float)(sr * sr);
    const unsigned T = Gm.base[SRF_MAX_LEVELS];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // in a scalar register: what follows is wave-uniform
    for (long long item = (long long)blockIdx.x * 4 + wave; item < items; item += stride) {
        const int seg = (int)(item / nchunk), chunk = (int)(item - (long long)seg * nchunk);
        const int s0 = seg_start[seg];
        const int s1 = seg + 1 < nseg ? seg_start[seg + 1] : n;
        const unsigned key = keys[s0];
        if (key >= T) continue;   // the records that contribute nothing
        const int lvl = (key >= Gm.base[1]) + (key >= Gm.base[2]) + (key >= Gm.base[3]);
        const srf_featmap f = L.lv[lvl];
        unsigned p = key - Gm.base[lvl];
        const unsigned px = p % (unsigned)f.W;
        p /= (unsigned)f.W;
        const unsigned py = p % (unsigned)f.H, pn = p / (unsigned)f.H;
        float *dst = G.grad[lvl] + (long long)pn * f.stride_n + (long long)py * f.stride_h + (long long)px * f.stride_w;
        // lane -> channels c0 + u * cs, u = 0..3
        const int c0 = VEC ? chunk * 256 + lane * 4 : chunk * 256 + lane;
        const int cs = VEC ? 1 : 64;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = s0; j < s1; j += 4) {
            unsigned sj[4];
            float wj[4];
            float g[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {   // past the segment's end: its last record again, loaded and not added
                const int jj = min(j + u, s1 - 1);
                sj[u] = src[jj];
                wj[u] = wsrt[jj];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float *row = gout + (long long)(sj[u] >> 6) * so_r + (long long)(sj[u] & 63u) * so_b;
                if (VEC) {
                    const float4 v = c0 < C ? *reinterpret_cast<const float4 *>(row + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
                    g[u][0] = v.x;
                    g[u][1] = v.y;
                    g[u][2] = v.z;
                    g[u][3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[u][e] = c0 + e * cs < C ? row[(long long)(c0 + e * cs) * so_c] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = j + u < s1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sum = __fadd_rn(acc[e], __fmul_rn(wj[u], __fmul_rn(g[u][e], inv)));
                    acc[e] = live ? sum : acc[e];
                }
            }
        }
        if (VEC) {
            if (c0 < C) *reinterpret_cast<float4 *>(dst + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e * cs < C) dst[(long long)(c0 + e * cs) * f.stride_c] = acc[e];
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- host
namespace {
struct OrdLayout {
    long long n;                 // records
    int nblk;                    // radix tiles
    size_t keys[2], vals[2], wts, seg, hist, hist_part, head_part, nseg, total;
};

// 0 records when the sizes are outside the entry's limits
OrdLayout ord_layout(int R, int pooled, int sr)
{
    OrdLayout o = {};
    if (R <= 0 || pooled <= 0 || pooled > SRF_MAX_POOLED || sr <= 0 || sr > SRF_MAX_SR || pooled * sr * sr > 128 || R > ORD_MAX_R) return o;
    const long long n = (long long)R * pooled * pooled * sr * sr * 4;
    if (n > ORD_MAX_RECORDS) return o;
    o.n = n;
    o.nblk = srf_ceil_div(n, ORD_TILE);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += srf_align256(bytes);
        return here;
    };
    for (int i = 0; i < 2; ++i) {
        o.keys[i] = take((size_t)n * 4);
        o.vals[i] = take((size_t)n * 4);
    }
    o.wts = take((size_t)n * 4);
    o.seg = take((size_t)n * 4);
    o.hist = take((size_t)256 * o.nblk * 4);
    o.hist_part = take(((size_t)srf_scan_blocks(256LL * o.nblk) + 1) * 4);
    o.head_part = take(((size_t)srf_scan_blocks(n) + 1) * 4);
    o.nseg = take(4);
    o.total = at;
    return o;
}
}   // namespace

extern "C" size_t srf_roi_extract_bwd_ordered_workspace_bytes(int R, int pooled, int sampling_ratio)
{
    return ord_layout(R, pooled, sampling_ratio).total;
}

extern "C" int srf_roi_extract_bwd_ordered(const srf_featmap *levels, float *const *grad_levels, int num_levels, int C, const float *rois, int R,
                                           int pooled, int sampling_ratio, float finest_scale, const float *grad_out, int64_t out_stride_r,
                                           int64_t out_stride_c, int64_t out_stride_bin, void *workspace, size_t workspace_bytes,
                                           srf_stream_t stream)
{
    if (!levels || !grad_levels || num_levels <= 0 || num_levels > SRF_MAX_LEVELS || C <= 0 || R < 0 || pooled <= 0 ||
        pooled > SRF_MAX_POOLED || sampling_ratio <= 0 || sampling_ratio > SRF_MAX_SR || !(finest_scale > 0.0f))
        return SRF_EINVAL;
    if (pooled * sampling_ratio * sampling_ratio > 128) return SRF_EINVAL;
    if (R == 0) return SRF_OK;
    if (!rois || !grad_out) return SRF_EINVAL;
    RoiLevels L;
    RoiGradLevels G;
    OrdGeom Gm;
    L.num = num_levels;
    unsigned long long total = 0;
    bool vec = C % 4 == 0 && out_stride_c == 1 && out_stride_r % 4 == 0 && out_stride_bin % 4 == 0 && ((uintptr_t)grad_out & 15) == 0;
    for (int i = 0; i < SRF_MAX_LEVELS; ++i) {
        const int j = i < num_levels ? i : 0;
        if (!grad_levels[j] || levels[j].N <= 0 || levels[j].H <= 0 || levels[j].W <= 0) return SRF_EINVAL;
        L.lv[i] = levels[j];
        G.grad[i] = grad_levels[j];
        Gm.base[i] = (unsigned)total;
        if (i < num_levels) {
            total += (unsigned long long)levels[j].N * levels[j].H * levels[j].W;
            if (total >= (1ull << ORD_KEY_BITS)) return SRF_EUNSUPPORTED;
            vec = vec && levels[j].stride_c == 1 && levels[j].stride_n % 4 == 0 && levels[j].stride_h % 4 == 0 && levels[j].stride_w % 4 == 0 &&
                  ((uintptr_t)grad_levels[j] & 15) == 0;
        }
    }
    Gm.base[SRF_MAX_LEVELS] = (unsigned)total;
    for (int i = num_levels; i < SRF_MAX_LEVELS; ++i) Gm.base[i] = (unsigned)total;   // no key reaches an unused level
    const OrdLayout o = ord_layout(R, pooled, sampling_ratio);
    if (o.n == 0) return SRF_EUNSUPPORTED;
    if (!workspace) return SRF_EINVAL;
    if (workspace_bytes < o.total) return SRF_EWORKSPACE;
    if ((uintptr_t)workspace & 15) return SRF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int n = (int)o.n;
    unsigned *keys[2] = {(unsigned *)(ws + o.keys[0]), (unsigned *)(ws + o.keys[1])};
    unsigned *vals[2] = {(unsigned *)(ws + o.vals[0]), (unsigned *)(ws + o.vals[1])};
    float *wts = (float *)(ws + o.wts);
    int *seg = (int *)(ws + o.seg), *hist = (int *)(ws + o.hist), *nseg = (int *)(ws + o.nseg);

    hipLaunchKernelGGL(srf_roi_ord_records_k, dim3(srf_ceil_div(o.n / 4, 256)), dim3(256), 0, st, L, Gm, rois, R, pooled, sampling_ratio,
                       finest_scale, keys[0], wts);
    int bits = 1;
    while (bits < ORD_KEY_BITS && (total >> bits) != 0) ++bits;
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8, cur ^= 1) {
        hipLaunchKernelGGL(srf_roi_ord_hist_k, dim3(o.nblk), dim3(256), 0, st, keys[cur], n, shift, o.nblk, hist);
        int rc = srf_device_scan(256 * o.nblk, OrdHistVal{hist}, OrdHistOut{hist}, (int *)(ws + o.hist_part), (int *)nullptr, -1, st);
        if (rc != SRF_OK) return rc;
        hipLaunchKernelGGL(srf_roi_ord_scatter_k, dim3(o.nblk), dim3(256), 0, st, keys[cur], shift == 0 ? (const unsigned *)nullptr : vals[cur], n,
                           shift, o.nblk, hist, keys[cur ^ 1], vals[cur ^ 1]);
    }
    // sorted (key, slot) in buffers `cur`; the other pair is free: (r, bin) and weight of every sorted record
    const OrdHeadOut head = {vals[cur], wts, seg, keys[cur ^ 1], (float *)vals[cur ^ 1], 4 * sampling_ratio * sampling_ratio, pooled * pooled,
                             (unsigned)n};
    int rc = srf_device_scan(n, OrdHeadVal{keys[cur]}, head, (int *)(ws + o.head_part), nseg, -1, st);
    if (rc != SRF_OK) return rc;
    const long long most = (o.n * ((C + 255) / 256) + 3) / 4;
    const int blocks = (int)(most < ORD_REDUCE_BLOCKS ? most : ORD_REDUCE_BLOCKS);
    if (vec)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_roi_ord_reduce_k<true>), dim3(blocks), dim3(256), 0, st, L, G, Gm, C, n, nseg, seg, keys[cur],
                           keys[cur ^ 1], (const float *)vals[cur ^ 1], sampling_ratio, grad_out, (long long)out_stride_r,
                           (long long)out_stride_c, (long long)out_stride_bin);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(srf_roi_ord_reduce_k<false>), dim3(blocks), dim3(256), 0, st, L, G, Gm, C, n, nseg, seg, keys[cur],
                           keys[cur ^ 1], (const float *)vals[cur ^ 1], sampling_ratio, grad_out, (long long)out_stride_r,
                           (long long)out_stride_c, (long long)out_stride_bin);
    SRF_LAUNCH_CHECK();
    return SRF_OK;
}
