/*
 * srfdet3d.h -- C ABI of libsrfdet3d_hip.so, the MI355X (gfx950) implementation of the SRFDet3D hot path.
 *
 * The reference (gopi-erabati/SRFDet3D) has no native code and no FFI of its own: its Python reaches the
 * operators below through third-party CUDA wheels (mmcv-full 1.7.0, mmdet 2.28.2, mmdet3d 1.0.0rc6,
 * spconv).  Each entry point cites the reference call site whose operator it replaces; the Python binding a
 * maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions:
 *   - plain C types only; every pointer is a DEVICE pointer borrowed from the caller unless marked "host";
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised here;
 *   - the library never allocates, frees or retains memory: outputs and workspaces come from the caller,
 *     sized with the *_workspace_bytes / *_capacity helpers (host-side, pure functions);
 *   - data-dependent sizes (voxel count, active-site count) are written to a device int the caller reads
 *     back when it needs the value on the host;
 *   - return value: 0 on success, negative on error (srf_error_string); no exceptions, no exit();
 *   - re-entrant, no global mutable state.
 */
#ifndef SRFDET3D_H
#define SRFDET3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *srf_stream_t;

#define SRF_OK 0
#define SRF_EINVAL (-1)       /* bad argument (null pointer, non-positive size, unsupported shape) */
#define SRF_EWORKSPACE (-2)   /* workspace smaller than *_workspace_bytes() */
#define SRF_EUNSUPPORTED (-3) /* channel count / kernel size outside the compiled set */
#define SRF_EHIP_BASE (-1000) /* -(1000 + hipError_t) */

int srf_abi_version(void);
const char *srf_error_string(int code);
/* Number of HIP devices visible, or a negative error.  Used by the Python loader to fail loudly. */
int srf_device_count(void);

/* ---- bitmap-rank rulebooks -------------------------------------------------------------------------------------
 * The same indice-pair generation (spconv SubMConv3d / SparseConv3d, sparse_encoder_custom.py:73-107, :123-134, :182-201)
 * for active sets whose rows are kept sorted by (b, y, x, z): one occupancy bit per cell of the level's grid plus an
 * exclusive popcount prefix per 32-bit word give "active? which row?" without a hash table, and the prefix scan of a
 * strided conv's output bitmap emits the new active set already sorted (a canonical order: independent of scheduling).
 * cell = ((b*H + y)*W + x)*D + z.  shape = host {D,H,W}.  bitmap: srf_bitmap_words() uint32; prefix: as many ints.
 * Valid geometries are those of K4 below (the window must fit the padded grid: shape[d] + 2*pad[d] >= ksize[d]); the SubM entry
 * wants odd kernel extents besides (SRF_EUNSUPPORTED).
 * Overflow of a strided step (more outputs than out_capacity): nothing is written past out_capacity rows / nbr_stride columns,
 * *num_out is the TRUE count (not clamped: the caller compares it with its capacity), the output bitmap and prefix are complete, and
 * the rows [0, out_capacity) are the first rows of the sorted set.  A consumer that is given such a level with A = out_capacity
 * (in_rows = out_capacity) reads every site whose rank is >= that as absent (-1). */
size_t srf_bitmap_words(const int *shape, int batch);
/* pair_counts may be NULL (the counts are bookkeeping, no kernel needs them).  ints a pair_counts buffer of the
 * srf_bitmap_* entry points must hold otherwise: the K counts come first, the rest is scratch
 * (replicated counters: hundreds of workgroups adding to one address would serialise in L2) */
size_t srf_bitmap_pair_count_ints(void);
size_t srf_bitmap_workspace_bytes(size_t words);
/* marks `indices` (A x 4 (b,z,y,x), distinct; rows with b < 0 are padding and are skipped by every srf_bitmap_* entry
 * point and by srf_densify), ranks them; order[r] = original row of sorted row r and
 * sorted_indices[r] = its coordinate (both optional, pass NULL for rows that are already sorted) */
int srf_bitmap_build(const int *indices, int A, const int *shape, int batch, void *bitmap, int *prefix, int *order,
                     int *sorted_indices, void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* the same for a capacity-sized set with padding rows: the slots of `order` / `sorted_indices` past the live count are written as
 * 0 / (-1,-1,-1,-1) by the call itself (same launch as the bitmap clear), so the caller passes uninitialised buffers */
int srf_bitmap_build_padded(const int *indices, int A, const int *shape, int batch, void *bitmap, int *prefix, int *order,
                            int *sorted_indices, void *workspace, size_t workspace_bytes, srf_stream_t stream);
int srf_bitmap_rulebook_subm(const int *sorted_indices, int A, const int *shape, int batch, const int *ksize,
                             const void *bitmap, const int *prefix, int *nbr /* K x A */, int *pair_counts /* K */,
                             srf_stream_t stream);
/* phase 1 of a strided conv: bitmap + prefix of the OUTPUT level (sized for the output shape), the sorted output
 * coordinates (at most out_capacity rows are written; use srf_strided_max_outputs) and their number */
int srf_bitmap_strided_outputs(const int *indices, int A, const int *shape, int batch, const int *ksize, const int *stride,
                               const int *pad, void *out_bitmap, int *out_prefix, int *out_indices, int out_capacity,
                               int *num_out, void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* fixed-shape form: ALL out_capacity rows of out_indices are written, those past *num_out as (-1,-1,-1,-1) */
int srf_bitmap_strided_outputs_static(const int *indices, int A, const int *shape, int batch, const int *ksize, const int *stride,
                                      const int *pad, void *out_bitmap, int *out_prefix, int *out_indices, int out_capacity,
                                      int *num_out, void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* phase 2: nbr (K rows of nbr_stride ints) from the INPUT level's bitmap + prefix.  The number of outputs is read on
 * the device (num_out, as written by phase 1), so this launch need not wait for the host; max_out bounds the grid (the
 * out_capacity of phase 1).  Columns >= *num_out are left untouched, or set to -1 when fill_tail != 0 (static-shape
 * levels: rows >= *num_out are padding whose coordinates are -1 and which every kernel here skips).  in_rows = rows of
 * the input level's arrays: ranks beyond it (possible only after a capacity overflow upstream) become -1. */
int srf_bitmap_strided_pairs(const int *out_indices, const int *num_out, int max_out, const int *shape, int batch,
                             const int *ksize, const int *stride, const int *pad, const void *in_bitmap, const int *in_prefix,
                             int in_rows, int *nbr, int nbr_stride, int fill_tail, int *pair_counts, srf_stream_t stream);

/* SparseConvTensor.dense() + the (N, C, D, H, W) -> (N, C * D, H, W) view of sparse_encoder_custom.py:144-147 as ONE pass that writes
 * the BEV map channels-last (out: (B, H, W, C * D) floats, channel c * D + z): every pixel is written once, from the level's bitmap
 * (active cells: the feature row of their rank; others: zeros) -- no zero fill, no scatter, no NCHW -> NHWC transpose.
 * feats (A x C) sorted by (b, y, x, z); bitmap / prefix as built for this level; (C * D) % 4 == 0. */
int srf_densify_bev(const float *feats, int A, int C, const void *bitmap, const int *prefix, int B, int D, int H, int W, float *out,
                    srf_stream_t stream);

/* The encoder of the pillar configs (csrc/pillar.hip, whose header holds the exact definition of both).
 *
 * srf_pillar_vfe: PillarFeatureNetCustom with one PFNLayer, mode="max", in eval mode (pillar_encoder_custom.py:108-161, utils.py:63-146)
 * in one launch.  voxels (rows, P, nf) zero-padded, num (rows), coors4 (rows, 4) (b, z, y, x) as srf_hard_voxelize[_static] writes them;
 * rows_dev: device count of live rows, or NULL (all rows); voxel_size / offset: host[3] (x, y, z), offset = v / 2 + range_lo rounded to
 * f32; W (Cout, K) row-major, K = nf + 3 * cluster_center + 3 * voxel_center; scale / shift (Cout): the folded eval BatchNorm;
 * out (rows, Cout).  Padding rows (r >= *rows_dev, b < 0 or num <= 0) are written as zeros.  Deterministic.
 * Limits (SRF_EUNSUPPORTED): Cout % 64 == 0 and Cout <= 256, 3 <= nf <= 8, P <= 64, voxels and out below 2^31 bytes.  Null pointers and
 * non-positive sizes: SRF_EINVAL.  Both are checked before any HIP call; rows == 0 is SRF_OK with no launch.
 *
 * srf_pillar_scatter_nhwc: PointPillarsScatter with the canvas channels-last: out (B, H, W, C) is zero-filled, then row r of feats
 * (rows, C), C % 4 == 0, is copied to pixel (b, y, x) of coors4[r] (z is ignored) in 16-byte stores; feats and out 16-byte aligned.
 * Rows with b < 0 or r >= *rows_dev (rows_dev may be NULL) are skipped, as srf_densify skips them.  The coordinates are distinct by
 * construction (one pillar per occupied cell).  A bit copy.  Limits: feats and out below 2^31 bytes. */
int srf_pillar_vfe(const float *voxels, const int *num, const int *coors4, const int *rows_dev, int rows, int P, int nf,
                   const float *voxel_size /*host[3]*/, const float *offset /*host[3]*/, int cluster_center, int voxel_center, int legacy,
                   const float *W, const float *scale, const float *shift, int Cout, float *out, srf_stream_t stream);
int srf_pillar_scatter_nhwc(const float *feats, const int *coors4, const int *rows_dev, int rows, int C, int B, int H, int W, float *out,
                            srf_stream_t stream);

/* The encoder of the dynamic-voxelization configs (csrc/dvfe.hip, whose header holds the exact definition).
 *
 * srf_dvfe_fwd: DynamicVFECustom.forward in eval mode (voxel_encoder.py:162-240, utils.py:8-45) with with_cluster_center,
 * with_centroid_aware_vox, mode="max", no distance feature and no fusion layer, in two launches behind srf_voxel_unique.
 * points (n, nf); point2voxel, order, offsets, counts, num_voxels as srf_voxel_unique writes them; voxel_coors (>= rows, 4) (b, z, y, x) its
 * sorted out_coors; voxel_size / offset: host[3] (x, y, z), offset = v / 2 + range_lo rounded to f32; voxel_center: append xyz - centre.
 * Position encoder: W1 (d, 3), W2 (d, d) row-major, scale1 / shift1 / scale2 / shift2 (d) the folded eval BatchNorms.  Layers: Wa
 * (C0, nf + d + 3 * voxel_center), scale_a / shift_a (C0); C1 > 0: Wb (C1, 2 * C0), scale_b / shift_b (C1); C1 == 0: one layer, Wb and
 * its vectors unused (may be NULL).  out (rows, C1 > 0 ? C1 : C0); rows at or past min(*num_voxels, rows) are written as zeros; points with
 * point2voxel < 0 (or past that count) touch nothing.  Nothing is read back; deterministic.
 * workspace: srf_dvfe_workspace_bytes(n, C0) bytes (the per-point output of layer 0, the only per-point intermediate in memory).
 * Checked before any HIP call, in this order: negative n / rows or non-positive nf, d, C0 (negative C1): SRF_EINVAL; n == 0 or rows == 0:
 * SRF_OK, no launch; null pointers: SRF_EINVAL; limits (3 <= nf <= 8, d in {16, 32, 64}, C0 and C1 <= 16, points, the workspace and out below
 * 2^31 bytes): SRF_EUNSUPPORTED; workspace too small: SRF_EWORKSPACE. */
size_t srf_dvfe_workspace_bytes(int n, int C0);
int srf_dvfe_fwd(const float *points, int n, int nf, const int *point2voxel, const int *order, const int *offsets, const int *counts,
                 const int *num_voxels, const int *voxel_coors, int rows, const float *voxel_size /*host[3]*/,
                 const float *offset /*host[3]*/, int voxel_center, const float *W1, const float *scale1, const float *shift1,
                 const float *W2, const float *scale2, const float *shift2, int d, const float *Wa, const float *scale_a,
                 const float *shift_a, int C0, const float *Wb, const float *scale_b, const float *shift_b, int C1, float *out,
                 void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * f-4  the step before the path: the CPU transforms of the reference's test pipeline between the decoded
 * sensor data and SRFDet.forward (configs/nus/srfdet_voxel_nusc_LC.py:253-283), on the device.
 *
 * srf_points_filter: PointsRangeFilter (mmdet3d points.in_range_3d: x > x_min && y > y_min && z > z_min &&
 * x < x_max && y < y_max && z < z_max) and, when close_radius > 0, the remove_close of
 * LoadPointsFromMultiSweeps (points with |x| < r && |y| < r dropped).  pc_range: host[6] or NULL (no range
 * test).  The kept points are copied in their original order to out_points (room for n rows); out_index
 * (may be NULL) receives their source rows; *num_out (device int) their count.
 * workspace: srf_points_filter_workspace_bytes(n).
 *
 * srf_image_prepare: V decoded views (V, H, W, 3) uint8 -> (V, 3, Hp, Wp) float32 = NormalizeMultiviewImage
 * ((x - mean) * (1 / std) per channel in float32, after a BGR<->RGB swap when to_rgb != 0) + PadMultiViewImage
 * (zeros below / right of the image; Hp >= H, Wp >= W, Wp % 4 == 0; the caller rounds up to size_divisor) of
 * mmdet3d_plugin/datasets/pipelines/transform_3d.py:7-93 + the HWC -> CHW transpose and stack of
 * DefaultFormatBundle3D.  mean / std: host[3].
 * ------------------------------------------------------------------------------------------------------- */
size_t srf_points_filter_workspace_bytes(int n);
int srf_points_filter(const float *points, int n, int nf, const float *pc_range /*host[6] or NULL*/,
                      float close_radius, float *out_points, int *out_index, int *num_out, void *workspace,
                      srf_stream_t stream);
int srf_image_prepare(const unsigned char *images, int V, int H, int W, const float *mean /*host[3]*/,
                      const float *std /*host[3]*/, int to_rgb, int Hp, int Wp, float *out, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * f-5  train-time augmentation: the 3-D transforms of the reference's train pipelines (GlobalRotScaleTrans,
 * RandomFlip3D, PointsRangeFilter, ObjectRangeFilter, ObjectNameFilter; mmdet3d 1.0.0rc6 LiDARPoints /
 * LiDARInstance3DBoxes semantics, e.g. configs/nus/srfdet_voxel_nusc_L.py train_pipeline) and GridMask
 * (mmdet3d_plugin/models/utils/grid_mask.py:72-128, applied at srfdet.py:189-190).
 * Random draws and sin / cos / arctan2 stay with the caller (host, float32); the device does correctly rounded
 * + - * / floor in the reference's order only.
 *
 * steps: bitmask, applied in this order; a clear bit skips the step (it is not applied as an identity):
 *   1 rotate     xyz <- xyz @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] (products rounded one by one, summed left to
 *                right, zero terms kept)
 *   2 scale      xyz *= scale
 *   4 translate  xyz += t
 *   8 h-flip     y = -y
 *  16 v-flip     x = -x
 * aug: host[7] = sin, cos, yaw_add, scale, tx, ty, tz (may be NULL when steps == 0).
 *
 * srf_points_augment: points (n, nf >= 3); the steps on channels 0-2, channels >= 3 copied unchanged; then, when
 * pc_range (host[6]) is given, the PointsRangeFilter test of srf_points_filter (strict inequalities).  The kept
 * points are written in their original order to out_points (room for n rows); out_index (may be NULL) receives
 * their source rows; *num_out (device int) their count.  workspace: srf_points_augment_workspace_bytes(n).
 *
 * srf_boxes_augment: boxes (n, box_dim = 7 | 9) [x, y, z, dx, dy, dz, yaw (, vx, vy)] with int64 labels (n):
 *   rotate     centre as above, yaw += yaw_add, [vx, vy] @ rot_mat_T[:2, :2];
 *   scale      columns 0-5 and 7- *= scale;
 *   translate  columns 0-2 += t;
 *   h-flip     y, vy negated, yaw = -yaw;
 *   v-flip     x, vx negated, yaw = -yaw + float32(pi);
 * then ObjectRangeFilter when bev_range (host[4] = xmin, ymin, xmax, ymax) is given (kept iff x > xmin && y > ymin &&
 * x < xmax && y < ymax, then yaw <- yaw - floor(yaw / P + 0.5) * P with P = float32(2 pi)), and ObjectNameFilter when
 * num_classes > 0 (kept iff 0 <= label < num_classes).  Kept boxes and labels are compacted in their original order
 * (out_boxes room for n rows, out_labels n); out_index (may be NULL) receives their source rows; *num_out (device
 * int) their count.  workspace: srf_boxes_augment_workspace_bytes(n).
 *
 * srf_grid_mask: out = in * mask over `planes` planes of H x W float32 (out of place; in is not changed).  With
 * hh = int(1.5 H), row y is in a stripe iff use_h && q = y + (hh - H) / 2 - st_h satisfies q >= 0, q / d < hh / d and
 * q % d < l (columns alike with W, st_w, use_w).  mode 1: mask = row or column in a stripe; mode 0: its negation.
 * A multiplication, so -0.0 and NaN come out as the reference's `x * mask`.  2 <= d, 1 <= l < d, 0 <= st_h, st_w < d.
 * ------------------------------------------------------------------------------------------------------- */
size_t srf_points_augment_workspace_bytes(int n);
int srf_points_augment(const float *points, int n, int nf, int steps, const float *aug /*host[7]*/,
                       const float *pc_range /*host[6] or NULL*/, float *out_points, int *out_index, int *num_out,
                       void *workspace, srf_stream_t stream);
size_t srf_boxes_augment_workspace_bytes(int n);
int srf_boxes_augment(const float *boxes, const long long *labels, int n, int box_dim, int steps,
                      const float *aug /*host[7]*/, const float *bev_range /*host[4] or NULL*/, int num_classes,
                      float *out_boxes, long long *out_labels, int *out_index, int *num_out, void *workspace,
                      srf_stream_t stream);
int srf_grid_mask(const float *in, int planes, int H, int W, int d, int l, int st_h, int st_w, int use_h, int use_w,
                  int mode, float *out, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * f-6  GT-database sampling and per-object noise of the LiDAR-only train pipelines (mmdet3d 1.0.0rc6 ObjectSample /
 * DataBaseSampler and ObjectNoise / noise_per_object_v3_, e.g. configs/kitti/srfdet_voxel_kitti_L.py train_pipeline).
 * The caller draws every random number and computes the box geometry on the host in float32: BEV corners (4 x [x, y],
 * clockwise as center_to_corner_box2d) and surface planes (6 x [a, b, c, d] as surface_equ_3d of corner_to_surfaces_3d).
 * The device does correctly rounded float32 + - * and compares in the reference's order, and float64 + where the
 * reference adds float64 noise.
 *
 * srf_points_in_boxes: out_box[i] = the first box b (box_mask[b] != 0 when box_mask is given) with
 * ((x a + y b) + z c) + d < 0 for all six planes of b, else -1; points (n, nf >= 3), planes (m, 6, 4).  num_outside
 * (device int, may be NULL) receives the count of -1s.  m <= 512, else SRF_EUNSUPPORTED.
 *
 * srf_box_collision_matrix: out[i * K + j] = box_collision_test(boxes[i], qboxes[j]) (uint8): the axis-aligned hulls
 * overlap (strictly) and either two edges cross or all corners of one box lie strictly inside the other.
 *
 * srf_box_collision_accept: the greedy rejection of DataBaseSampler.sample_all.  fixed (n_fixed, 4, 2) = the GT boxes'
 * corners, cand (n_cand, 4, 2) the candidates' grouped by class, class c = [class_offsets[c], class_offsets[c + 1])
 * (device int[num_classes + 1]), classes in sampling order.  Candidate i is rejected iff it collides (as `boxes`) with a
 * fixed box, an accepted candidate of an earlier class, or a not-rejected candidate of its own class other than itself,
 * the later ones included; accept[i] = 1 / 0.  One workgroup; n_fixed + n_cand <= 2048, else SRF_EUNSUPPORTED.
 *
 * srf_object_sample_merge: out rows [0, s) = sampled (s, nf) with columns 0-2 + the centre (obj_centres (k, 3)) of
 * their object o (rows [obj_offsets[o], obj_offsets[o + 1]); obj_offsets device int[k + 1], obj_offsets[0] = 0), then
 * the points (n, nf) with point_box[i] < 0 (srf_points_in_boxes of the accepted boxes) in their order; *num_out
 * (device int) = s + their count.  out has room for s + n rows.  workspace: srf_object_sample_merge_workspace_bytes.
 *
 * srf_object_noise: m boxes (m, box_dim = 7 | 9), num_try tries each: rot_sc (m, num_try, 2) = float32 sin, cos of
 * the float64 angles rot (m, num_try), loc (m, num_try, 3) float64 translations; corners (m, 4, 2) and planes
 * (m, 6, 4) of the unmoved boxes.  Box i (in order) takes its first try whose moved BEV corners (float32 rotation about
 * its centre, then float32(float64 corner + (float64 centre + loc))) collide with no other box's current corners;
 * chosen[i] = that try or -1.  Then every point inside a box (the first one by index, original planes) becomes
 * float32(float64(rotate(p - centre) + centre) + loc) (a box with chosen -1 uses angle 0 and loc 0), the others are
 * copied; out_boxes: xyz = float32(float64 xyz + loc), yaw = float32(float64 yaw + rot).  m <= 512, else
 * SRF_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------------------- */
int srf_points_in_boxes(const float *points, int n, int nf, const float *planes, int m, const int *box_mask, int *out_box,
                        int *num_outside, srf_stream_t stream);
int srf_box_collision_matrix(const float *boxes, int N, const float *qboxes, int K, unsigned char *out, srf_stream_t stream);
int srf_box_collision_accept(const float *fixed, int n_fixed, const float *cand, int n_cand, const int *class_offsets,
                             int num_classes, int *accept, srf_stream_t stream);
size_t srf_object_sample_merge_workspace_bytes(int n, int s);
int srf_object_sample_merge(const float *points, int n, int nf, const int *point_box, const float *sampled, int s,
                            const int *obj_offsets, const float *obj_centres, int k, float *out, int *num_out, void *workspace,
                            srf_stream_t stream);
int srf_object_noise(const float *points, int n, int nf, const float *boxes, int m, int box_dim, const float *corners,
                     const float *planes, const float *rot_sc, const double *rot, const double *loc, int num_try,
                     float *out_points, float *out_boxes, int *chosen, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K2  dynamic voxelization.
 * Replaces mmcv.ops.Voxelization(max_num_points=-1).forward as called from SRFDet.voxelize,
 * mmdet3d_plugin/models/detectors/srfdet.py:233-247.
 * coors: (n,3) int32 rows (z,y,x), (-1,-1,-1) for points outside the range.  grid = (gx,gy,gz).
 * ------------------------------------------------------------------------------------------------------- */
int srf_dynamic_voxelize(const float *points, int n, int nf, const float *voxel_size /*host[3]*/,
                         const float *pc_range /*host[6]*/, const int *grid /*host[3] x,y,z*/, int *coors,
                         srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K1  hard voxelization (+ a3 HardSimpleVFE mean, fused).
 * Replaces mmcv.ops.Voxelization(max_num_points>0, deterministic=True).forward as called from
 * SRFDet.voxelize, srfdet.py:218-232 (module built at srfdet.py:58), and the HardSimpleVFE of
 * configs/nus/srfdet_voxel_nusc_L.py:40.
 * Outputs in first-seen voxel order: voxels (rows x max_points x nf, unused slots zero), coors (rows x 3,
 * z,y,x), num (rows), voxel_num (1 int).  rows = min(n, max_voxels) must be allocated; only the first
 * *voxel_num rows are written.  mean (rows x mean_features) may be NULL.
 * ------------------------------------------------------------------------------------------------------- */
size_t srf_hard_voxelize_workspace_bytes(int n, int max_points);
int srf_hard_voxelize(const float *points, int n, int nf, const float *voxel_size /*host[3]*/,
                      const float *pc_range /*host[6]*/, const int *grid /*host[3]*/, int max_points, int max_voxels,
                      float *voxels, int *coors, int *num, int *voxel_num, float *mean, int mean_features,
                      void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* The fixed-shape form of K1 for a frame replayed from a hipGraph (one sample, n >= 1): ALL rows = min(n, max_voxels) rows of every
 * output are written -- rows >= *voxel_num are padding: zeros, num 0, coordinates -1 -- and the coordinates are (rows x 4)
 * (batch_index, z, y, x), the layout SparseEncoderCustom takes (the F.pad of srfdet.py:228-229 folded in). */
int srf_hard_voxelize_static(const float *points, int n, int nf, const float *voxel_size /*host[3]*/,
                             const float *pc_range /*host[6]*/, const int *grid /*host[3]*/, int max_points, int max_voxels,
                             float *voxels, int *coors4, int *num, int *voxel_num, float *mean, int mean_features, int batch_index,
                             void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K3  DynamicScatter, split in its two halves so that a caller can reuse the point->voxel map.
 * Replaces mmcv.ops.DynamicScatter.forward as called from
 * mmdet3d_plugin/models/voxel_encoders/voxel_encoder.py:189 (mean) and :232 (max), and the dense canvas of
 * map_voxel_center_to_point (:118-158).
 * srf_voxel_unique: coors (n,4) int32 (b,z,y,x).  A row is kept only if it names a cell of the grid: 0 <= b < batch,
 *   0 <= z < D, 0 <= y < H, 0 <= x < W.  Every other row is dropped -- a row with a negative entry (the -1 rows of K2),
 *   and equally a row with b >= batch or a coordinate at or over its extent: it is never filed under another cell and
 *   never reaches past the batch*D*H*W cells.  Outputs, all
 *   caller-allocated with n rows: out_coors (n x 4, first *num_voxels rows valid, sorted lexicographically),
 *   point2voxel (n; -1 for dropped points), counts (n; points per voxel), offsets (n; start of each voxel's
 *   list in `order`), order (n; point indices grouped by voxel, ascending within a voxel; the entries past the
 *   number of kept points are not written), num_voxels (1 int).
 * srf_scatter_reduce: out (rows x C); the first min(rows, *num_voxels) rows are written, any further rows are left as
 *   they were; mode 0 = mean (sum in point order / count), 1 = max (v > acc ? v : acc from -inf: a NaN is never taken).
 * ------------------------------------------------------------------------------------------------------- */
size_t srf_voxel_unique_workspace_bytes(int n, const int *grid_zyx /*host[3] D,H,W*/, int batch);
int srf_voxel_unique(const int *coors, int n, const int *grid_zyx /*host[3]*/, int batch, int *out_coors,
                     int *point2voxel, int *counts, int *offsets, int *order, int *num_voxels, void *workspace,
                     size_t workspace_bytes, srf_stream_t stream);
int srf_scatter_reduce(const float *feats, const int *order, const int *offsets, const int *counts,
                       const int *num_voxels, int rows, int C, int mode, float *out, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K4  sparse-conv rulebooks.
 * Replaces spconv's indice-pair generation behind SparseConvTensor / SubMConv3d / SparseConv3d as used by
 * SparseEncoderCustom, mmdet3d_plugin/models/middle_encoders/sparse_encoder_custom.py:123-134 (layers built
 * at :73-107, :182-201).
 * A coordinate table maps (b,z,y,x) -> row.  The rulebook is output-stationary:
 * nbr[k * nbr_stride + o] = input row feeding output row o through kernel offset k, or -1;
 * k = (kz*KH + ky)*KW + kx.  pair_counts[k] = number of valid pairs of offset k.
 * Strided convs number their output rows in first-seen order over (input row, k) ascending.
 * Geometry (every entry point here and in the bitmap section): extents >= 1, pad >= 0, K <= 27, fewer than 2^32 - 1 cells in the
 * input and in the output grid, and the window fits the padded grid, shape[d] + 2*pad[d] >= ksize[d], in every dimension;
 * out_shape[d] = floor((shape[d] + 2*pad[d] - ksize[d]) / stride[d]) + 1.  Anything else is SRF_EINVAL -- a window larger than
 * the padded grid too, whatever the stride.  Every refusal is decided on the host before anything is enqueued.
 * Preconditions the library cannot check: rows distinct and inside the grid.
 * ------------------------------------------------------------------------------------------------------- */
int srf_coord_table_capacity(int max_rows); /* smallest power of two >= max(1024, 2*max_rows) */
size_t srf_coord_table_bytes(int capacity);
int srf_coord_table_build(const int *indices /* A x 4 */, int A, const int *shape /*host[3] D,H,W*/, int batch,
                          void *table, int capacity, srf_stream_t stream);
int srf_rulebook_subm(const int *indices, int A, const int *shape /*host[3]*/, const int *ksize /*host[3]*/,
                      const void *table, int capacity, int *nbr /* K x A */, int *pair_counts /* K */,
                      srf_stream_t stream);
/* bound on the outputs of a strided conv: A * prod(ceil(k/s)), clipped to the output volume */
int srf_strided_max_outputs(int A, int batch, const int *shape, const int *ksize, const int *stride, const int *pad);
size_t srf_rulebook_strided_workspace_bytes(int A, const int *ksize /*host[3]*/, int out_capacity);
/* phase 1: discover and number the outputs; builds the coordinate table of the output level */
int srf_rulebook_strided_outputs(const int *indices, int A, const int *shape, int batch, const int *ksize,
                                 const int *stride, const int *pad, int *out_indices /* max_out x 4 */,
                                 int *num_out /* 1 int */, void *out_table, int out_capacity, void *workspace,
                                 size_t workspace_bytes, srf_stream_t stream);
/* phase 2: fill nbr (K x num_out_host, caller-allocated after reading num_out) from the same workspace */
int srf_rulebook_strided_pairs(int A, const int *ksize, const void *out_table, int out_capacity,
                               const void *workspace, int num_out_host, int *nbr, int *pair_counts,
                               srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K5  sparse convolution forward with fused eval-BatchNorm / residual / ReLU epilogue.
 * Replaces spconv SubMConv3d/SparseConv3d.forward (+ the BN1d and ReLU modules chained by mmdet3d's
 * make_sparse_convmodule / SparseBasicBlock) on the path sparse_encoder_custom.py:125-134.
 * out[o] = sum_k W[k]^T in[nbr[k][o]] accumulated as an f32 fma chain (k ascending, c ascending);
 * then y = fma(x, alpha, beta) if alpha, y += residual[o] if residual, y = max(y,0) if relu (each step one rounded f32 operation:
 * srf_spconv_epilogue, csrc/spconv_frame.hpp, shared by every entry point below).
 * W: (K, Cin, Cout) row-major.  Supported Cout: 16 (any Cin <= 512) and 32, 64, 128 (Cin a multiple of 4).
 * rows_dev (may be NULL): device int; output rows >= *rows_dev are padding of a static-shape level and are skipped
 * (their tiles return at once), so a hipGraph can launch the layer at its capacity without paying for it.
 * ------------------------------------------------------------------------------------------------------- */
int srf_spconv_fwd(const float *in, int A_in, int Cin, const float *W, int K, const int *nbr, int nbr_stride,
                   int A_out, int Cout, const float *alpha, const float *beta, const float *residual, int relu,
                   float *out, const int *rows_dev, srf_stream_t stream);

/* Gradients of the sparse convolution, for the configurations that train the LiDAR branch (the reference does so in every
 * L-only config: tools/train.py:221-234 freezes it only under `freeze_lidar_components`); they stand where spconv's
 * indice_conv_backward runs.
 * srf_spconv_transpose_rulebook: nbrT (K x A_in) with nbrT[k][i] = o <=> nbr[k][o] = i, -1 elsewhere.
 * srf_spconv_bwd_data: d_in[i] = sum_k W[k] d_out[nbrT[k][i]]; W_T is (K, Cout, Cin) row-major (each offset's matrix
 *   transposed).  It is srf_spconv_fwd with the roles swapped, so Cin must be one of its output widths (16, 32, 64, 128).
 *   A submanifold layer may pass nbrT = its own nbr with W_T's offsets reversed (the rulebook is symmetric).
 * srf_spconv_bwd_weight: d_W[k][ci][co] = sum_o in[nbr[k][o]][ci] d_out[o][co], (K, Cin, Cout); Cin, Cout <= 128.  Row
 *   ranges are combined with float atomics: reproducible to rounding, not bitwise (srf_spconv_bwd_weight_ordered below is). */
int srf_spconv_transpose_rulebook(const int *nbr, int nbr_stride, int K, int A_out, int *nbrT, int A_in, srf_stream_t stream);
int srf_spconv_bwd_data(const float *grad_out, int A_out, int Cout, const float *W_T, int K, const int *nbrT, int nbrT_stride,
                        int A_in, int Cin, float *grad_in, srf_stream_t stream);
int srf_spconv_bwd_weight(const float *in, int A_in, int Cin, const float *grad_out, int A_out, int Cout, const int *nbr,
                          int nbr_stride, int K, float *grad_W, srf_stream_t stream);

/* srf_spconv_bwd_weight in a fixed order: two calls give the same bytes.  The output rows are cut into ranges j = 0, 1, ... of 2048
 * rows; the kernel of srf_spconv_bwd_weight (the same K loop) STORES the (Cin, Cout) partial of (offset k, range j), zeros
 * included, to workspace[j][k][ci][co], and a second kernel writes d_W[k][ci][co] = the __fadd_rn sum of the partials for
 * j = 0, 1, ... in ascending order, starting from range 0's value (a single range is stored straight into grad_W).  Limits, codes
 * and check order of srf_spconv_bwd_weight, then: a NULL workspace with work to do SRF_EINVAL, a workspace smaller than
 * srf_spconv_bwd_weight_ordered_workspace_bytes SRF_EWORKSPACE.  A_out == 0 or A_in == 0 gives zeros.  The size is 0 for
 * non-positive arguments and outside the limits. */
size_t srf_spconv_bwd_weight_ordered_workspace_bytes(int A_out, int Cin, int Cout, int K);
int srf_spconv_bwd_weight_ordered(const float *in, int A_in, int Cin, const float *grad_out, int A_out, int Cout, const int *nbr,
                                  int nbr_stride, int K, float *grad_W, void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* Fast path of K5 for constant weights: re-lay W once (srf_spconv_pack_weights -> packed, of
 * srf_spconv_packed_weight_bytes bytes) into the operand layout of the kernel, then call srf_spconv_fwd_packed with
 * the same remaining arguments.  Results are bit-identical to srf_spconv_fwd.  The shapes (K, Cin, Cout) with a packed form, with the
 * bf16 form below and with a row plan are ONE table: srf_spconv_shape, csrc/spconv_frame.hpp.
 * srf_spconv_packed_weight_bytes returns 0 for every other shape (no packed form: use srf_spconv_fwd); there
 * srf_spconv_pack_weights and srf_spconv_fwd_packed return SRF_EUNSUPPORTED.  srf_spconv_fwd_packed also returns
 * SRF_EUNSUPPORTED for an input of 2 GiB or more (A_in * Cin * 4 >= 2^31) or with no rows (A_in == 0). */
size_t srf_spconv_packed_weight_bytes(int K, int Cin, int Cout);
int srf_spconv_pack_weights(const float *W, int K, int Cin, int Cout, float *packed, srf_stream_t stream);
int srf_spconv_fwd_packed(const float *in, int A_in, int Cin, const float *W_packed, int K, const int *nbr,
                          int nbr_stride, int A_out, int Cout, const float *alpha, const float *beta,
                          const float *residual, int relu, float *out, const int *rows_dev, const int *tiles,
                          srf_stream_t stream);

/* Work-balanced row ranges of a rulebook for srf_spconv_fwd_packed (optional, `tiles` may be NULL there): the output
 * rows are cut into srf_spconv_tiles_count(A_out) consecutive ranges of equal cost (a row costs its pairs +
 * srf_spconv_tiles_row_cost(); range t = the rows whose exclusive cost prefix lies in [t*P/T, (t+1)*P/T)),
 * tiles[t]..tiles[t+1], so that the workgroups of the 64- / 128-channel kernels (one range each) finish together
 * although the neighbour count per row varies over the sweep.  Built once per rulebook -- the SubM layers of a level share one (sparse_encoder_custom.py:125-134) --
 * from nbr alone; A_out / nbr_stride / rows_dev as in srf_spconv_fwd, and the same A_out must be passed to both calls.
 * workspace: srf_spconv_tiles_workspace_bytes(A_out) bytes; tiles: srf_spconv_tiles_count(A_out) + 1 ints. */
int srf_spconv_tiles_count(int A_out);
int srf_spconv_tiles_row_cost(void);
size_t srf_spconv_tiles_workspace_bytes(int A_out);
int srf_spconv_tiles_build(const int *nbr, int nbr_stride, int K, int A_out, const int *rows_dev, void *workspace,
                           int *tiles, srf_stream_t stream);
/* Row order for the 32-output-channel layers of srf_spconv_fwd_packed (optional; passed as its `tiles` argument for the shapes of
 * plan kind 2): rows with the same set of kernel offsets side by side, so that a wave, which multiplies every offset any of
 * its 32 rows has, skips more of them.  plan: srf_spconv_order_ints(A_out, K) ints = [order: A_pad][sorted rulebook: K x A_pad], A_pad =
 * A_out rounded up to 1024; order[pos] = the row at position pos (-1: padding).  One launch, no workspace; rows_dev as for the
 * convolution.  Outputs are bit-identical with and without a plan (every row is its own fma chain).  No reference counterpart. */
size_t srf_spconv_order_ints(int A_out, int K);
int srf_spconv_order_build(const int *nbr, int nbr_stride, int K, int A_out, const int *rows_dev, int *plan, srf_stream_t stream);
/* Which plan srf_spconv_fwd_packed takes as `tiles` for a layer shape (the table's third column; a host call): 0 none, 1 the row
 * ranges of srf_spconv_tiles_build, 2 the row order of srf_spconv_order_build. */
int srf_spconv_plan_kind(int K, int Cin, int Cout);

/* K5 with bf16 products (opt-in, inference; no reference counterpart beyond its fp16 option): f32 tensors, every input value and every
 * weight rounded to bf16 once (round to nearest even), exact products on the bf16 MFMA, f32 accumulation in a fixed order, the epilogue
 * of srf_spconv_fwd in f32 on the f32 accumulator (alpha, beta and the residual are not rounded), f32 stored.  Defined exactly by
 * tests/spconv_bf16_ref.py.  The bits of an output row depend on its own pairs, the operands and the epilogue alone (not on A_out,
 * *rows_dev, `tiles` or the rows beside it); two launches give the same bits.  Non-finite weights are outside the domain.
 * The shapes (K, Cin, Cout) with this form are the ones srf_spconv_fwd_packed runs on its 64- / 128-channel kernel in the encoders
 * (the table's bf16 column).  srf_spconv_bf16_packed_weight_bytes returns 0 for every other shape; there srf_spconv_bf16_pack_weights and srf_spconv_fwd_bf16
 * return SRF_EUNSUPPORTED.  srf_spconv_bf16_pack_weights rounds W (K, Cin, Cout) and lays it out for the kernel.  srf_spconv_fwd_bf16
 * takes the arguments of srf_spconv_fwd_packed with the same meanings and the same codes in the same order, all decided before any
 * HIP call: bad arguments SRF_EINVAL; another shape SRF_EUNSUPPORTED; A_out == 0 SRF_OK with nothing launched; null pointers
 * SRF_EINVAL; A_in == 0 or an input of 2 GiB or more SRF_EUNSUPPORTED.  `tiles` may be NULL; the kernel takes no row plan and ignores
 * it.  Rows at or past *rows_dev are not written. */
size_t srf_spconv_bf16_packed_weight_bytes(int K, int Cin, int Cout);
int srf_spconv_bf16_pack_weights(const float *W, int K, int Cin, int Cout, void *packed, srf_stream_t stream);
int srf_spconv_fwd_bf16(const float *in, int A_in, int Cin, const void *W_packed, int K, const int *nbr, int nbr_stride, int A_out,
                        int Cout, const float *alpha, const float *beta, const float *residual, int relu, float *out,
                        const int *rows_dev, const int *tiles, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K6  SparseConvTensor.dense() (+ the view to (B, C*D, H, W), which is a no-op on this layout).
 * Replaces sparse_encoder_custom.py:135-138.  out: (B, C, D, H, W) contiguous; zero_fill != 0 clears it first.
 * ------------------------------------------------------------------------------------------------------- */
int srf_densify(const float *feats, const int *indices, int A, int C, int B, int D, int H, int W, float *out,
                int zero_fill, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K7  RoIAlign(avg, aligned) behind mmdet SingleRoIExtractor.
 * Replaces pooler(feats[:4], rois) at mmdet3d_plugin/models/sparse_heads/srfdet_head.py:1685, :2548, :2626
 * (config configs/nus/srfdet_voxel_nusc_LC.py:169-178).
 * Feature maps are described by element strides so that NCHW and channels-last tensors both work.
 * out element (r, c, bin) is written at out[r*out_stride_r + c*out_stride_c + bin*out_stride_bin];
 * accumulate != 0 adds into out instead of overwriting it (camera sum, srfdet_head.py:2561).
 * ------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *data;
    int N, H, W;
    int64_t stride_n, stride_c, stride_h, stride_w; /* in elements */
    float spatial_scale;                            /* 1 / featmap stride */
} srf_featmap;

int srf_roi_extract(const srf_featmap *levels /*host[num_levels]*/, int num_levels, int C, const float *rois /* R x 5 */,
                    int R, int pooled, int sampling_ratio, float finest_scale, float *out, int64_t out_stride_r,
                    int64_t out_stride_c, int64_t out_stride_bin, int accumulate, int *levels_out /* R or NULL */,
                    srf_stream_t stream);
/* srf_roi_extract_sum: output row r (R rows) = the sum over s = 0 .. n_sum - 1, added in that order, of the gathers of the RoIs
 * rois[s * R + r] (n_sum * R RoIs, group-major): the per-camera image RoIs of a proposal summed over the cameras
 * (srfdet_head.py:2543-2562: pooler over all n_cam * R RoIs, then .sum over the camera axis) in one launch, without the
 * (n_cam * R, S, C) intermediate.  Same sampling arithmetic as srf_roi_extract; out is addressed through the three strides, so it may
 * be a channel slice of the fused (R, S, 2 C) operand of `output_fused_proj` (:2255-2329). */
int srf_roi_extract_sum(const srf_featmap *levels /*host[num_levels]*/, int num_levels, int C, const float *rois /* (n_sum R) x 5 */,
                        int R, int n_sum, int pooled, int sampling_ratio, float finest_scale, float *out, int64_t out_stride_r,
                        int64_t out_stride_c, int64_t out_stride_bin, srf_stream_t stream);


/* Backward of srf_roi_extract with respect to the feature maps (training of the image branch; RoIs carry no
 * gradient, as in mmcv's roi_align_backward).  grad_levels[i] has the layout of levels[i] and must be zeroed by
 * the caller; grad_out has the strides given.  Every tap is added with a float atomic: the bits depend on the order in which
 * the adds arrive (srf_roi_extract_bwd_ordered below fixes the order). */
int srf_roi_extract_bwd(const srf_featmap *levels /*host*/, float *const *grad_levels /*host array of device ptrs*/,
                        int num_levels, int C, const float *rois, int R, int pooled, int sampling_ratio,
                        float finest_scale, const float *grad_out, int64_t out_stride_r, int64_t out_stride_c,
                        int64_t out_stride_bin, srf_stream_t stream);

/* srf_roi_extract_bwd with the adds of every map element in a fixed order and no float atomic: two calls give the same bytes
 * (csrc/roi_bwd_ordered.hip; tests/roi_bwd_ordered_ref.py is the definition in numpy float32).
 *   A record is (RoI r, output row ph, column pw, sample iy, ix, tap t in 0..3), the taps ordered (y_low, x_low), (y_low, x_high),
 *   (y_high, x_low), (y_high, x_high).  Level, sample point, validity rules and the f32 weights are those of srf_roi_extract_bwd
 *   (the same __f*_rn sequence; hy = 1 - ly; w = hy * hx and the other three likewise).  A record with w == 0, a sample that is
 *   NaN or out of range, or a batch id outside [0, N) contributes nothing.  For every element (level, n, y, x, c) touched by at
 *   least one record:  acc = +0; for the element's records in ascending (r, ph, pw, iy, ix, t):
 *       acc = __fadd_rn(acc, __fmul_rn(w, __fmul_rn(grad_out[r][bin][c], 1.0f / (sr * sr))))
 *   and the element is STORED, not added.  Elements without a record are left as the caller passed them (the caller zero-fills).
 * Arguments, codes and check order of srf_roi_extract_bwd (a level with H <= 0 or W <= 0 is SRF_EINVAL too), then, before any
 * launch: the levels' N H W summing to 2^30 or more (record keys are 30 bits: level base + flat pixel), R > 2^24 or more than 2^30
 * records (R pooled^2 sr^2 4): SRF_EUNSUPPORTED; a NULL workspace SRF_EINVAL; one smaller than
 * srf_roi_extract_bwd_ordered_workspace_bytes SRF_EWORKSPACE; one that is not 16-byte aligned SRF_EUNSUPPORTED.  R == 0 is SRF_OK with
 * nothing launched.  The workspace size is a worst case computed on the host from (R, pooled, sampling_ratio) alone -- 24 bytes per
 * record and the scan tables -- and 0 for non-positive arguments and outside the limits. */
size_t srf_roi_extract_bwd_ordered_workspace_bytes(int R, int pooled, int sampling_ratio);
int srf_roi_extract_bwd_ordered(const srf_featmap *levels /*host*/, float *const *grad_levels /*host array of device ptrs*/,
                                int num_levels, int C, const float *rois, int R, int pooled, int sampling_ratio, float finest_scale,
                                const float *grad_out, int64_t out_stride_r, int64_t out_stride_c, int64_t out_stride_bin,
                                void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a11-a13  proposal box -> RoI geometry, fused.
 * Replaces the torch op chains of points_feats_sampling_bboxes_roi (srfdet_head.py:1638-1683 / :2579-2624)
 * and img_feats_sampling_bboxes_roi (:2435-2528), including boxes3d_to_corners3d
 * (mmdet3d_plugin/core/bbox/util.py:84-176).
 * boxes: (B, P, box_dim >= 8).  mutate_centres != 0 overwrites boxes[..., :3] with metres in place, as
 * srfdet_head.py:1646 does.  rois_bev: (B*P, 5).  rois_img: (n_cam*B*P, 5), cam-major, batch id b + cam*B
 * (the reference's indexing, :2520-2528); lidar2img: (B, n_cam, 4, 4) row-major.  Either output may be NULL.
 * ------------------------------------------------------------------------------------------------------- */
int srf_box_rois(float *boxes, int B, int P, int box_dim, const float *pc_range /*host[6]*/,
                 const float *voxel_size /*host[3]*/, int mutate_centres, float *rois_bev, const float *lidar2img,
                 int n_cam, float *rois_img, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * a14-a17  dense arithmetic of a decoder stage (SingleSRFDetHeadLiDAR.forward / SingleSRFDetHead.forward,
 * srfdet_head.py:1484-1525 == :2281-2322; DynamicConv :2633-2693; fused projection :2255-2264).
 *
 * srf_linear: Y (M x N, row stride ldy) = chain(X (M x K, ldx) . W^T (W is N x K, ldw) + bias) where chain is
 *   [LayerNorm(ln1, eps1)] -> [ReLU if relu1] -> [+ residual (M x N, ldr)] -> [LayerNorm(ln2, eps2)] -> [ReLU if relu2];
 *   null pointers skip a step.  Replaces nn.Linear + nn.LayerNorm + ReLU (+ the residual adds) call chains, e.g.
 *   out_layer -> norm3 -> ReLU -> (+prop) -> norm2 (srfdet_head.py:2689-2691, :1502-1503).  K % 4 == 0; K >= 2048 is
 *   split over K and needs the workspace (srf_linear_workspace_bytes), as does any row step with N > 128.  The row steps
 *   (LayerNorm, residual, relu2) need N <= 1024, else SRF_EUNSUPPORTED; bias and relu1 alone take any N, split over K or not.
 * srf_self_attention: qkv (P x 3E) = [q | k | v] rows after in_proj -> out (P x E), heads H, head dim E/H in {16, 32};
 *   replaces the attention core of nn.MultiheadAttention(batch 1) at srfdet_head.py:1489.
 * srf_dynconv_mid: feats (R x S x C) bin-major RoI features, params (R x 2*C*D) from dynamic_layer ->
 *   relu(LN_C(relu(LN_D(feats W1)) W2)) (R x S x C); srfdet_head.py:2671-2686.  (C, D) in {(128,32), (256,64)}, S <= 64.
 * srf_apply_deltas: srfdet_head.py:1534-1625; deltas (R x Dd) on boxes (R x Dd) [centres in metres, log sizes, ...] -> out (R x Dd):
 *   clip((d / w * exp(b_size) + b_ctr - lo) / ext, 0, 1) | log(exp(min(d / w, scale_clamp)) * exp(b_size)) | the deltas from column 6 on,
 *   copied.  weights6 / pc_range are host arrays of 6 floats; ext = pc_range[3 + i] - pc_range[i], formed in float32.  Checked in this
 *   order: R < 0, Dd < 8 (no upper limit), a NULL weights6 or pc_range: SRF_EINVAL; R == 0: SRF_OK; a NULL deltas, boxes or out: SRF_EINVAL.
 * ------------------------------------------------------------------------------------------------------- */
size_t srf_linear_workspace_bytes(int M, int N, int K);
int srf_linear(const float *X, int M, int K, int ldx, const float *W, int N, int ldw, const float *bias,
               const float *ln1_g, const float *ln1_b, float eps1, int relu1, const float *residual, int ldr,
               const float *ln2_g, const float *ln2_b, float eps2, int relu2, float *Y, int ldy, void *workspace,
               size_t workspace_bytes, srf_stream_t stream);
int srf_self_attention(const float *qkv, int P, int E, int H, float *out, srf_stream_t stream);
/* the same for B samples of P proposals each (rows sample-major): one launch instead of the per-sample loop of a batched head */
int srf_self_attention_batched(const float *qkv, int B, int P, int E, int H, float *out, srf_stream_t stream);
int srf_dynconv_mid(const float *feats, const float *params, int R, int S, int C, int D, const float *g1,
                    const float *b1, float eps1, const float *g2, const float *b2, float eps2, float *out,
                    srf_stream_t stream);
/* srf_channel_affine: y[n][c][:] = x[n][c][:] * scale + shift (+ residual[n][c][:]), optionally clamped at 0, in one
 * pass.  per_sample == 0: scale/shift are [C] -- eval-mode BatchNorm2d (+ ReLU) after the dense convolutions of
 * SECONDCustom / FPN / VoVNet (second_custom.py:41-63, vovnet.py:116-153).  per_sample == 1: scale/shift are [N*C] -- the
 * eSE channel gate, with the OSA block's identity input as `residual` (vovnet.py:165-177, :225-228).  shift and
 * residual may be NULL.  x, y: NCHW f32 with plane size HW and their own batch strides (in floats), so y may be a
 * channel slice of a wider tensor; y == x is allowed; residual is contiguous (N, C, HW). */
int srf_channel_affine(const float *x, int N, int C, int HW, long long x_batch_stride, const float *scale,
                       const float *shift, int per_sample, const float *residual, int relu, float *y,
                       long long y_batch_stride, srf_stream_t stream);

/* srf_upsample_add: out = lateral + nearest_upsample(top), the top-down step of mmdet's FPN (`laterals[i-1] +=
 * F.interpolate(laterals[i], size=laterals[i-1].shape[2:], mode='nearest')`; the necks of configs/nus/srfdet_voxel_nusc_LC.py)
 * in one pass.  lateral, out: (NC, H, W) f32 contiguous (out == lateral allowed), top: (NC, Ht, Wt); source index
 * floor(dst * Ht / H) as F.interpolate.  W % 4 == 0, else SRF_EUNSUPPORTED. */
int srf_upsample_add(const float *lateral, const float *top, int NC, int H, int W, int Ht, int Wt, float *out,
                     srf_stream_t stream);

/* srf_dwconv3x3s2: depthwise 3x3 convolution, stride 2, padding 1 (w: (C, 9), no bias) followed by y = y * scale[c] +
 * shift[c] (eval BatchNorm2d; either may be NULL) and an optional ReLU: the stair of the dynamic proposal generator,
 * ConvModule(C, C, 3, stride=2, padding=1, groups=C, norm BN2d) built at srfdet_head.py:265-320 and run at :525-536.
 * x: (N, C, H, W) f32 contiguous -> y: (N, C, (H - 1) / 2 + 1, (W - 1) / 2 + 1). */
int srf_dwconv3x3s2(const float *x, int N, int C, int H, int W, const float *w, const float *scale, const float *shift,
                    int relu, float *y, srf_stream_t stream);

/* srf_nchw_to_nhwc: y[n][p][c] = x[n][c][p] (p = h * W + w): the channels-last copy of a feature level that
 * srf_roi_extract gathers from (the reference feeds NCHW levels to mmcv RoIAlign, srfdet_head.py:1685 / :2548; this
 * library's gather wants one contiguous C-run per tap).  HW % 4 == 0, else SRF_EUNSUPPORTED. */
int srf_nchw_to_nhwc(const float *x, int N, int C, int HW, float *y, srf_stream_t stream);

/* srf_ese_gate: gate[n][c] = relu6(sum_k W[c][k] * mean[n][k] + bias[c] + 3) / 6 -- the channel gate of VoVNet's eSE
 * module (mmdet3d_plugin/models/backbones/vovnet.py, eSEModule: Hsigmoid(fc(avg_pool(x)))) on the (N, C) global averages;
 * W: (C, C) row-major = the 1x1 conv weight, bias (C) or NULL.  N <= 8, C % 4 == 0. */
int srf_ese_gate(const float *mean, int N, int C, const float *W, const float *bias, float *gate, srf_stream_t stream);

/* srf_maxpool3s2_ceil: nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True) on (NC, H, W) f32 -> (NC, Ho, Wo),
 * Ho = ceil((H - 3) / 2) + 1 (the last window must start inside the input), likewise Wo: the stage pooling of the
 * VoVNet image backbone (mmdet3d_plugin/models/backbones/vovnet.py, `_make_layer` of every stage but the first). */
int srf_maxpool3s2_ceil(const float *x, int NC, int H, int W, float *y, srf_stream_t stream);

/* srf_conv1x1: 1x1 convolution over the channel concatenation of n_src (<= 8) NCHW f32 tensors of the same N and
 * H*W, followed by y = y * scale[co] + shift[co] (scale may be NULL: bias only; both NULL: none) and an optional ReLU --
 * the `concat` layer of VoVNet's OSA blocks (vovnet.py:180-230: torch.cat + conv1x1 + BN + ReLU) without the
 * concatenated tensor, and the FPN lateral convolutions.  srcs / src_channels are HOST arrays (device pointers,
 * channel counts, each a multiple of 32); W_packed comes from srf_conv1x1_pack_weights(W (Cout x K row-major, K = sum
 * of the channel counts in concat order)); Cout % 128 == 0 and HW % 4 == 0, else SRF_EUNSUPPORTED.  out: (N, Cout, HW). */
size_t srf_conv1x1_packed_weight_bytes(int Cout, int K);
int srf_conv1x1_pack_weights(const float *W, int Cout, int K, float *packed, srf_stream_t stream);
int srf_conv1x1(const float *const *srcs, const int *src_channels, int n_src, int N, int HW, const float *W_packed, int Cout,
                const float *scale, const float *shift, int relu, float *out, srf_stream_t stream);

/* ---- channels-last (NHWC) dense convolutions on the f32 MFMA (csrc/conv.hip) --------------------------------------
 * Activations are (N, H, W, ld) f32, `ld` floats per pixel >= the channels used: x / y point at the first channel of
 * the slice a layer reads / writes inside its buffer, so the OSA concatenation of VoVNet (vovnet.py:222) is a set
 * of slices of one buffer and never a copy.
 *
 * srf_wino3x3: Conv2d(Cin, Cout, 3, stride 1, padding 1, bias folded into shift) as Winograd F(2x2, 3x3), followed by
 * y = y * scale[co] + shift[co] (either may be NULL) and an optional ReLU: the 3x3 layers of VoVNet's OSA blocks
 * (vovnet.py:116-133, :180-230), the image FPN outputs, `img_convs` (srfdet_head.py:404-416), SECONDCustom
 * (second_custom.py:41-63) and the BEV FPN.  U_packed comes from srf_wino3x3_pack_weights(W (Cout, Cin, 3, 3)).
 * Cin % 8 == 0, x 16-byte aligned, x_ld % 4 == 0, 4 H W x_ld < 2^30, else SRF_EUNSUPPORTED. */
size_t srf_wino3x3_packed_weight_bytes(int Cout, int Cin);
int srf_wino3x3_pack_weights(const float *W, int Cout, int Cin, float *packed, srf_stream_t stream);
int srf_wino3x3(const float *x, int N, int H, int W, int Cin, long long x_ld, const float *U_packed, int Cout,
                const float *scale, const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);

/* srf_wino43: the same layer as srf_wino3x3 as Winograd F(4x4, 3x3) (csrc/wino43.hip): 36 products per 16 outputs instead of
 * 16 per 4, i.e. direct FLOPs / 4 on the MFMA.  Two kernels per call: the input transform V = B^T d B of every 6 x 6 patch into
 * `workspace` (srf_wino43_workspace_bytes), then the 36 batched products with the output transform, scale / shift / ReLU as the
 * epilogue.  U_packed comes from srf_wino43_pack_weights(W (Cout, Cin, 3, 3)) (U = G g G^T computed in double, rounded once).
 * Replaces the same reference call sites as srf_wino3x3 (vovnet.py:116-133, :180-216; srfdet_head.py:404-416;
 * second_custom.py:41-63).  f32 result within ~2e-5 of the map's maximum of the direct convolution (Cin <= 1024).
 * Cin % 8 == 0, Cout % 4 == 0, x / y / scale / shift 16-byte aligned, x_ld % 4 == 0, y_ld % 4 == 0, else SRF_EUNSUPPORTED. */
size_t srf_wino43_packed_weight_bytes(int Cout, int Cin);
int srf_wino43_pack_weights(const float *W, int Cout, int Cin, float *packed, srf_stream_t stream);
size_t srf_wino43_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int srf_wino43(const float *x, int N, int H, int W, int Cin, long long x_ld, const float *U_packed, int Cout, const float *scale,
               const float *shift, int relu, float *y, long long y_ld, void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* The two kernels of srf_wino43 as separate calls, for callers that time them apart (bench.py's roofline: the transform is
 * HBM-bound, the multiply MFMA-bound) or order other work between them.  Same arguments and limits; SRF_EUNSUPPORTED when the
 * layer's transformed input exceeds one workspace slab (srf_wino43 then runs it in several). */
int srf_wino43_transform(const float *x, int N, int H, int W, int Cin, long long x_ld, int Cout, void *workspace, size_t workspace_bytes,
                         srf_stream_t stream);
int srf_wino43_multiply(const void *workspace, size_t workspace_bytes, int N, int H, int W, int Cin, const float *U_packed, int Cout,
                        const float *scale, const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);

/* srf_conv1x1_nhwc: Conv2d(K, Cout, 1) on channels-last activations = the GEMM y[p][co] = sum_k x[p][k] W[co][k] over
 * M = N * H * W pixels, then y = y * scale[co] + shift[co] (either may be NULL) and an optional ReLU: the `concat` layer of
 * VoVNet's OSA blocks read straight from the block's concat buffer (vovnet.py:222-223) and the FPN lateral convolutions.
 * W_packed comes from srf_conv1x1_nhwc_pack_weights(W (Cout, K) row-major).  K % 32 == 0, x 16-byte aligned, x_ld % 4 == 0,
 * else SRF_EUNSUPPORTED. */
size_t srf_conv1x1_nhwc_packed_weight_bytes(int Cout, int K);
int srf_conv1x1_nhwc_pack_weights(const float *W, int Cout, int K, float *packed, srf_stream_t stream);
int srf_conv1x1_nhwc(const float *x, long long M, int K, long long x_ld, const float *W_packed, int Cout, const float *scale,
                     const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);
/* srf_conv1x1_nhwc_direct*: the same three operations (plain, _topdown, _pooled) on a GEMM kernel whose operands go L2 ->
 * registers without LDS staging or barriers (csrc/gemm_direct.hip; 128 x 128 tiles only: meant for launches of >= ~1000 tiles,
 * where it runs at 122-135 TFLOP/s against 110-117 for srf_conv1x1_nhwc).  W_packed comes from
 * srf_conv1x1_nhwc_direct_pack_weights (a different operand order than srf_conv1x1_nhwc_pack_weights).  Same arguments, limits
 * and -- output for output -- the same fma chain, i.e. identical bits in y; the pooled mean adds its block sums in a different
 * (fixed) order.  Workspace of the pooled form: srf_conv1x1_nhwc_pooled_workspace_bytes. */
size_t srf_conv1x1_nhwc_direct_packed_weight_bytes(int Cout, int K);
int srf_conv1x1_nhwc_direct_pack_weights(const float *W, int Cout, int K, float *packed, srf_stream_t stream);
int srf_conv1x1_nhwc_direct(const float *x, long long M, int K, long long x_ld, const float *W_packed, int Cout, const float *scale,
                            const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_direct_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const float *W_packed, int Cout,
                                    const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt, long long top_ld,
                                    float *y, long long y_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_direct_pooled(const float *x, int N, long long HW, int K, long long x_ld, const float *W_packed, int Cout,
                                   const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean, void *workspace,
                                   size_t workspace_bytes, srf_stream_t stream);
/* srf_conv1x1_nhwc_split*: the same three operations as an f32 GEMM computed on the bf16 MFMA (csrc/gemm_split.hip).  Every f32
 * operand is the exact sum of three bf16 values (x = xh + xm + xl); of the nine exact partial products of a b the six of relative
 * magnitude >= 2^-16 are accumulated in f32 on v_mfma_f32_32x32x16_bf16, the three dropped ones are together below 2^-23 |a b| (one
 * f32 rounding of the product).  Error against float64 = that of the f32 fma chain (measured 2.0-2.8e-7 of sum |a b| against 1.7-3.0e-7);
 * NOT bit-identical to srf_conv1x1_nhwc (another summation order), deterministic.  189-199 TFLOP/s f32-equivalent where the f32 MFMA
 * kernels reach 122-135.  W_packed (bf16 planes, 6 bytes per weight) comes from srf_conv1x1_nhwc_split_pack_weights; x stays f32 and
 * is split while it is staged.  Same arguments and limits as the _direct forms; workspace of the pooled form:
 * srf_conv1x1_nhwc_pooled_workspace_bytes. */
size_t srf_conv1x1_nhwc_split_packed_weight_bytes(int Cout, int K);
int srf_conv1x1_nhwc_split_pack_weights(const float *W, int Cout, int K, void *packed, srf_stream_t stream);
int srf_conv1x1_nhwc_split(const float *x, long long M, int K, long long x_ld, const void *W_packed, int Cout, const float *scale,
                           const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_split_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const void *W_packed, int Cout,
                                   const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt, long long top_ld,
                                   float *y, long long y_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_split_pooled(const float *x, int N, long long HW, int K, long long x_ld, const void *W_packed, int Cout,
                                  const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean,
                                  void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* srf_conv_gemm_nhwc_split: srf_conv_gemm_nhwc (Conv2d with stride / padding as an implicit-im2col GEMM: VoVNet stem_3, SECONDCustom's
 * stride-2 layers, the BEV FPN extras) on the split GEMM kernel.  W_packed = srf_conv1x1_nhwc_split_pack_weights of the weight reordered
 * to (Cout, kh * kw * Cin), tap index slowest.  Cin % 32 == 0, the input below 2 GB, else SRF_EUNSUPPORTED. */
int srf_conv_gemm_nhwc_split(const float *x, int N, int H, int W, int Cin, long long x_ld, const void *W_packed, int Cout, int kh, int kw,
                             int stride, int pad, const float *scale, const float *shift, int relu, float *y, long long y_ld,
                             srf_stream_t stream);
/* srf_conv1x1_nhwc_bf16* / srf_conv_gemm_nhwc_bf16: the same four operations with ONE bf16 product per f32 product
 * (csrc/gemm_bf16.hip) -- the opt-in reduced-precision mode of the image branch, never taken by default.  Tensors stay f32.  Each
 * activation and each weight is rounded to bf16 once (round to nearest even, as v_cvt_pk_bf16_f32 and torch.Tensor.bfloat16()), the
 * products (exact in f32) are accumulated in f32 on v_mfma_f32_32x32x16_bf16, and the epilogue of the split forms (scale / shift /
 * ReLU, the top-down add, the column means of the stored outputs) is applied to the f32 accumulator: y = epilogue(sum bf16(x) bf16(w))
 * up to f32 accumulation error (<= 6e-7 of sum |a b|), <= (2^-7 + 2^-16 + 6e-7) sum |a b| from the unrounded product.  Deterministic.
 * +-inf / NaN and values that round to infinity (|v| > 0x1.FEp127) give what IEEE arithmetic gives on the rounded operands; operands
 * whose rounding is a bf16 subnormal may be flushed: an absolute error of at most 2^-126 |partner| per such term.  W_packed (one bf16
 * plane in the kernel's image order, K padded to a multiple of 64: 2 bytes per weight) comes from srf_conv1x1_nhwc_bf16_pack_weights;
 * for the conv form of the weight reordered to (Cout, kh * kw * Cin), tap index slowest.  Same arguments, limits and error codes as
 * the _split forms; workspace of the pooled form: srf_conv1x1_nhwc_pooled_workspace_bytes. */
size_t srf_conv1x1_nhwc_bf16_packed_weight_bytes(int Cout, int K);
int srf_conv1x1_nhwc_bf16_pack_weights(const float *W, int Cout, int K, void *packed, srf_stream_t stream);
int srf_conv1x1_nhwc_bf16(const float *x, long long M, int K, long long x_ld, const void *W_packed, int Cout, const float *scale,
                          const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_bf16_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const void *W_packed, int Cout,
                                  const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt, long long top_ld,
                                  float *y, long long y_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_bf16_pooled(const float *x, int N, long long HW, int K, long long x_ld, const void *W_packed, int Cout,
                                 const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean,
                                 void *workspace, size_t workspace_bytes, srf_stream_t stream);
int srf_conv_gemm_nhwc_bf16(const float *x, int N, int H, int W, int Cin, long long x_ld, const void *W_packed, int Cout, int kh, int kw,
                            int stride, int pad, const float *scale, const float *shift, int relu, float *y, long long y_ld,
                            srf_stream_t stream);



/* srf_conv_wgrad_nhwc (training, config 4): the WEIGHT gradient of a stride-1 Conv2d on channels-last tensors,
 *   dW[co][ci][ky][kx] = sum over (n, y, x) of g[n][y][x][co] * x[n][y + ky - pad][x + kx - pad][ci],
 * ksize 1 (padding 0) or 3 (padding 1) -- what torch.autograd computes through aten::convolution_backward for the trainable layers of
 * tools/train.py:220-234 (VoVNet stages 4-5, vovnet.py:354-374; the image FPN; the head's img_convs, srfdet_head.py:404-416), there on
 * MIOpen's float-atomic split-K kernels.  Here: an f32 GEMM over the pixels on the bf16 MFMA through the exact three-way split of both
 * operands (csrc/wgrad.hip), the pixel ranges added in a fixed order: deterministic.  g: (N, H, W, g_ld) with Cout channels, x:
 * (N, H, W, x_ld) with Cin channels, dW: (Cout, Cin, ksize, ksize) contiguous; workspace: srf_conv_wgrad_workspace_bytes bytes.
 * Cin % 4 == Cout % 4 == 0, W >= 32, tensors below 2 GB, 16-byte aligned bases, g_ld % 4 == x_ld % 4 == 0; else SRF_EUNSUPPORTED. */
size_t srf_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ksize);
int srf_conv_wgrad_nhwc(const float *g, long long g_ld, const float *x, long long x_ld, int N, int H, int W, int Cin, int Cout, int ksize,
                        void *workspace, size_t workspace_bytes, float *dW, srf_stream_t stream);

/* srf_conv_wgrad_nhwc_bf16 (training, the opt-in bf16-product mode): the same weight gradient on ONE bf16 product per f32 product,
 *   dW[co][ci][ky][kx] = sum over p of bf16(g[p][co]) * bf16(x[p + tap][ci]),
 * each operand rounded once to nearest even, products exact in f32, f32 accumulation, pixels outside the image zero, the pixel ranges
 * added in a fixed order: deterministic (csrc/wgrad_bf16.hip; reduced precision, the caller's explicit choice).  Arguments as
 * srf_conv_wgrad_nhwc; workspace: srf_conv_wgrad_bf16_workspace_bytes bytes (partial sums and the bf16 planes of both operands; 0 for
 * sizes the entry point refuses), 16-byte aligned.  Any map width.  Checked in this order, before any HIP call: non-positive sizes, a
 * pitch below the channel count, null pointers: SRF_EINVAL; ksize other than 1 or 3, Cin % 4, Cout % 4, g_ld % 4, x_ld % 4, a base or
 * workspace that is not 16-byte aligned, a tensor of 2 GB or more: SRF_EUNSUPPORTED; workspace too small: SRF_EWORKSPACE. */
size_t srf_conv_wgrad_bf16_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ksize);
int srf_conv_wgrad_nhwc_bf16(const float *g, long long g_ld, const float *x, long long x_ld, int N, int H, int W, int Cin, int Cout,
                             int ksize, void *workspace, size_t workspace_bytes, float *dW, srf_stream_t stream);

/* srf_conv1x1_nhwc_topdown: an FPN lateral convolution with the top-down step in its epilogue (mmdet FPN.forward:
 * `laterals[i - 1] += F.interpolate(laterals[i], size=..., mode="nearest")`, necks of configs/nus/srfdet_voxel_nusc_LC.py:55-64
 * and :67-76): y[n][py][px][co] = act(conv) + top[n][floor(py Ht / H)][floor(px Wt / W)][co].  x rows are the pixels of an
 * (N, H, W) map; top is an (N, Ht, Wt, >= Cout) channels-last slice with top_ld floats per pixel.  Same bits as
 * srf_conv1x1_nhwc followed by srf_nhwc_upsample_add. */
int srf_conv1x1_nhwc_topdown(const float *x, int N, int H, int W, int K, long long x_ld, const float *W_packed, int Cout,
                             const float *scale, const float *shift, int relu, const float *top, int Ht, int Wt, long long top_ld,
                             float *y, long long y_ld, srf_stream_t stream);
/* srf_conv1x1_nhwc_residual / _direct_residual / _split_residual: conv3 of a ResNet bottleneck with the block's identity in the
 * epilogue (mmdet Bottleneck.forward: `relu(bn3(conv3(out)) + identity)`), one entry per f32-accurate family:
 *   y[p][co] = act(fl(fma(acc, scale[co], shift[co])) + res[p][co]),   act = the family's fmaxf ReLU (relu != 0) or nothing,
 * i.e. the add comes BEFORE the ReLU (the _topdown forms add after it).  res: an (M, res_ld) row-major operand on the rows of y,
 * res_ld >= Cout (SRF_EINVAL), res_ld % 4 == 0 and res 16-byte aligned (SRF_EUNSUPPORTED), not overlapping y (not checked).  res is read
 * through a 32-bit buffer descriptor over the rows of one tile: res_ld * rows * 4 must stay below 2^31 bytes, rows = 256 for
 * srf_conv1x1_nhwc_residual and 128 for the other two, else SRF_EUNSUPPORTED.  Otherwise the arguments, limits, codes and check order of
 * the plain forms; the residual checks follow the plain ones of their class.  Same bits as the plain form without ReLU followed by one
 * f32 add and the ReLU.  There is no bf16-product residual form. */
int srf_conv1x1_nhwc_residual(const float *x, long long M, int K, long long x_ld, const float *W_packed, int Cout, const float *scale,
                              const float *shift, int relu, float *y, long long y_ld, const float *res, long long res_ld,
                              srf_stream_t stream);
int srf_conv1x1_nhwc_direct_residual(const float *x, long long M, int K, long long x_ld, const float *W_packed, int Cout,
                                     const float *scale, const float *shift, int relu, float *y, long long y_ld, const float *res,
                                     long long res_ld, srf_stream_t stream);
int srf_conv1x1_nhwc_split_residual(const float *x, long long M, int K, long long x_ld, const void *W_packed, int Cout,
                                    const float *scale, const float *shift, int relu, float *y, long long y_ld, const float *res,
                                    long long res_ld, srf_stream_t stream);
/* srf_conv1x1_nhwc_pooled: the same convolution on N images of HW pixels (rows n HW .. (n + 1) HW - 1), which also returns
 * mean[n][co] = the mean over the image's pixels of the stored outputs: VoVNet's eSE average pool (reference
 * mmdet3d_plugin/models/backbones/vovnet.py:165-177 eSEModule.avg_pool on the output of vovnet.py:223 `concat`) without a
 * second pass over the map.  Deterministic (per-block sums added in a fixed order).  workspace: _workspace_bytes(N, HW, Cout). */
size_t srf_conv1x1_nhwc_pooled_workspace_bytes(int N, long long HW, int Cout);
int srf_conv1x1_nhwc_pooled(const float *x, int N, long long HW, int K, long long x_ld, const float *W_packed, int Cout,
                            const float *scale, const float *shift, int relu, float *y, long long y_ld, float *mean, void *workspace,
                            size_t workspace_bytes, srf_stream_t stream);

/* srf_conv_gemm_nhwc: Conv2d(Cin, Cout, (kh, kw), stride, padding) on channels-last activations as the GEMM of
 * srf_conv1x1_nhwc with an implicit im2col (rows = output pixels, k = (tap, input channel)): the stride-2 3x3 layers of the
 * path (VoVNet stem_3, vovnet.py stem; the first layer of SECONDCustom's later blocks, second_custom.py:41-52; the extra levels
 * of the BEV FPN) -- deterministic k-ordered fma chains where MIOpen's channels-last choice is an atomic split-K kernel.
 * W_packed = srf_conv1x1_nhwc_pack_weights(W reordered to (Cout, kh * kw * Cin), tap slowest).  Cin % 32 == 0, the input
 * tensor below 2 GiB.  y: (N, Ho, Wo, y_ld), Ho = floor((H + 2 pad - kh) / stride) + 1; any kh, kw, stride > 0 and pad >= 0 (kh != kw,
 * pad >= k and stride > k included).  A kernel larger than the padded map (H + 2 pad < kh or W + 2 pad < kw) has no output pixel and
 * is SRF_EINVAL whatever the stride, here and in srf_conv_gemm_nhwc_split / srf_conv_gemm_nhwc_bf16.
 * srf_stem_conv_nchw: Conv2d(Cin <= 4, 64, 3, stride 2, padding 1) + scale / shift + ReLU from NCHW images to channels-last
 * (VoVNet stem_1 on the 6 camera views); Wt is the (64, Cin, 3, 3) weight. */
int srf_conv_gemm_nhwc(const float *x, int N, int H, int W, int Cin, long long x_ld, const float *W_packed, int Cout, int kh,
                       int kw, int stride, int pad, const float *scale, const float *shift, int relu, float *y, long long y_ld,
                       srf_stream_t stream);
int srf_stem_conv_nchw(const float *x, int N, int Cin, int H, int W, const float *Wt, int Cout, const float *scale,
                       const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);
/* srf_stem_conv7_nchw: Conv2d(Cin <= 4, 64, 7, stride 2, padding 3) + scale / shift + ReLU from contiguous NCHW images to a
 * channels-last slice (N, Ho, Wo, y_ld), Ho = (H - 1) / 2 + 1 (mmdet ResNet conv1 / bn1 / relu); Wt is the (64, Cin, 7, 7) weight.
 * Arguments, codes and refusal order of srf_stem_conv_nchw; every output is one k-ordered fma chain (k = ci 49 + ky 7 + kx). */
int srf_stem_conv7_nchw(const float *x, int N, int Cin, int H, int W, const float *Wt, int Cout, const float *scale,
                        const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);

/* srf_dcnv2_nhwc (csrc/dcn.hip): modulated deformable convolution (DCNv2) forward on channels-last activations -- mmcv's
 * `modulated_deform_conv2d` under `ModulatedDeformConv2dPack`, the 3x3 convolution of the bottlenecks of stages 3 and 4 of
 * the ResNet-101 image backbone of configs/others/srfdet_dvoxel_waymo_LC.py:68-69 (mmdet ResNet(dcn=dict(type='DCNv2'))):
 *   y[n][oy][ox][co] = act(scale[co] * sum_{tap, ci} W[co][ci][tap] * m(n, oy, ox, g(ci), tap) * bilinear(x[n][.][.][ci], py, px)
 *                          + shift[co]),
 *   py = oy * stride - pad + ky * dilation + dy(n, oy, ox, g, tap),  px likewise with dx,
 * bilinear sampling with zero padding (a corner outside the map contributes 0; continuous in the offsets), as
 * srfdet3d_amd/compat/dcn.py defines it.  The srf_conv_gemm_nhwc GEMM with a gathered A operand: W_packed is the same packed
 * weight (srf_conv1x1_nhwc_pack_weights of W reordered to (Cout, kh * kw * Cin), tap slowest); scale / shift (either may be
 * NULL; a bias is folded into shift by the caller) and relu as there.  x: (N, H, W, x_ld) with Cin channels, y: (N, Ho, Wo,
 * y_ld) with Cout channels, Ho = (H + 2 pad - dilation (kh - 1) - 1) / stride + 1.
 * offset: (N, Ho, Wo, offset_ld) with 2 kh kw G channels, channel (g kh kw + tap) 2 = dy and + 1 = dx; mask: (N, Ho, Wo, mask_ld)
 * with kh kw G channels, channel g kh kw + tap.  Both may point into one (N, Ho, Wo, 3 kh kw G) buffer, the raw `conv_offset`
 * output in mmcv's channel order (mask = offset + 2 kh kw G, the same pitch).  mask_is_logit != 0: the kernel applies the
 * sigmoid; 0: the mask is used as given.  Deterministic: fixed summation order, no atomics.
 * SRF_EUNSUPPORTED (before any launch): groups != 1, Cin % deform_groups != 0, (Cin / deform_groups) % 32 != 0, H < 2 or
 * W < 2, the input tensor of 2 GiB or more, x not 16-byte aligned, x_ld % 4 != 0. */
int srf_dcnv2_nhwc(const float *x, int N, int H, int W, int Cin, long long x_ld, const float *offset, long long offset_ld,
                   const float *mask, long long mask_ld, int mask_is_logit, const float *W_packed, int Cout, int kh, int kw,
                   int stride, int pad, int dilation, int groups, int deform_groups, const float *scale, const float *shift,
                   int relu, float *y, long long y_ld, srf_stream_t stream);

/* srf_msda_fwd (csrc/msda.hip): multi-scale deformable attention, forward -- the sampling core of mmcv's
 * `MultiScaleDeformableAttention` (Zhu et al., "Deformable DETR", eq. 3) under the two layers of `encoder_lidar`
 * (srfdet_head.py:241-263, :657-758, `with_lidar_encoder=True`).  mmcv is not part of the reference tree: this text is the definition.
 *   value:  (B S, value_ld) rows of heads * head_dim channels [head][d], S = sum_l H_l W_l, the L levels of a batch element one after
 *           the other in the order of `shapes`, row h W_l + w inside a level: a flattened channels-last pyramid.
 *   shapes: host[L][2] = (H_l, W_l); a level starts at the prefix sum of the products.
 *   ref:    (B Q, L, 2) contiguous, normalised (x, y) per query and level.
 *   offs:   (B Q, offs_ld) rows of (heads, L, P, 2) = (dx, dy) in pixels of level l;  logits: (B Q, logits_ld) rows of (heads, L, P), raw.
 *           Both may point into one row buffer of width 3 heads L P (offsets first, the same pitch): the output of ONE GEMM.
 *   out:    (B Q, out_ld) rows of heads * head_dim channels.
 *   a[q,h,:,:]  = softmax over the L P logits of (q, h)   (float32, max-subtracted)
 *   px = ref_x W_l + dx - 0.5,  py = ref_y H_l + dy - 0.5  (grid_sample's align_corners=False)
 *   out[q,h,:]  = sum_{l,p} a[q,h,l,p] * bilinear(value_l[b, ., ., h, :], py, px)
 * A corner outside the map contributes 0.  A sample whose position is not inside (-1, H_l) x (-1, W_l) contributes 0 as a whole; the
 * comparisons are false for NaN and +-inf, so such offsets contribute 0 too.  This is the rule of mmcv's CUDA operator and NOT
 * grid_sample's, which lets a NaN position through; on finite positions the two agree.  Non-finite logits propagate as a float32
 * softmax propagates them.  Deterministic: the sum runs over l, then p, then the corners (y0 x0), (y0 x1), (y1 x0), (y1 x1) as one
 * fma chain; no atomics.  Forward only.
 * SRF_EINVAL: a negative B or Q, L, P, heads or head_dim <= 0, no shapes, a level with H or W <= 0, a pitch below its row's width, a null
 * tensor with B Q > 0.  SRF_EUNSUPPORTED (before any launch): head_dim not 16 or 32, L > 4, P > 4, a tensor of 2 GiB or more, a pitch
 * that is no multiple of 4 floats, a base that is not 16-byte aligned.  B Q == 0 is nothing to do (SRF_OK). */
int srf_msda_fwd(const float *value, long long value_ld, int B, const int *shapes /*host[L][2]*/, int L, const float *ref,
                 const float *offs, long long offs_ld, const float *logits, long long logits_ld, int Q, int heads, int head_dim, int P,
                 float *out, long long out_ld, srf_stream_t stream);

/* srf_msda_bwd (csrc/msda_bwd.hip): the gradient of srf_msda_fwd, as that definition is written.  value, shapes, ref, offs, logits, Q,
 * heads, head_dim, P: the forward's inputs, same layouts and pitches (offs and logits may share one row buffer).
 *   grad_out:    (B Q, grad_out_ld) rows of heads * head_dim channels, the cotangent of `out`.
 *   grad_value:  (B S, grad_value_ld), the layout of `value`.  The entry point ADDS into it: the caller zeroes it.
 *   grad_offs:   (B Q, grad_offs_ld) rows of (heads, L, P, 2);  grad_logits: (B Q, grad_logits_ld) rows of (heads, L, P).  Both may point
 *                into one row buffer, as the forward's inputs do.
 * Each of the three outputs may be NULL: that gradient is skipped (its pitch is ignored) and the others do not change by a bit.
 * With g = grad_out[q,h,:], a the softmax, px, py the forward's position, (x0, y0) = floor, lx = px - x0, ly = py - y0 and the
 * corners v00 = value_l[y0][x0], v01 = [y0][x0+1], v10 = [y0+1][x0], v11 = [y0+1][x0+1] (0 outside the map):
 *   t[l,p]              = <g, (1-ly)(1-lx) v00 + (1-ly) lx v01 + ly (1-lx) v10 + ly lx v11>
 *   grad_logits[l,p]    = a[l,p] (t[l,p] - sum_j a[j] t[j])
 *   grad_offs[l,p].x    = a[l,p] <g, (1-ly)(v01 - v00) + ly (v11 - v10)>
 *   grad_offs[l,p].y    = a[l,p] <g, (1-lx)(v10 - v00) + lx (v11 - v01)>            (offsets are in pixels: no W or H factor)
 *   grad_value[corner] += a[l,p] w_corner g                                         (corners inside the map only)
 * A sample whose position is not inside (-1, H_l) x (-1, W_l) -- NaN and +-inf positions included -- has t = 0, a zero offset
 * gradient and adds nothing.  A position on an integer takes its floor cell.  This is the rule of mmcv's CUDA operator and NOT the
 * derivative grid_sample's backward takes at positions exactly on an integer or on the box edge; everywhere else the two agree.  There
 * is no gradient for `ref`.  Non-finite logits propagate as float32 arithmetic propagates them (not pinned).
 * Determinism: grad_offs and grad_logits are computed in a fixed order (the sum over a head's channels is a fixed cross-lane butterfly,
 * the sum over j runs in sample order): two launches give the same bits.  grad_value is a data-dependent scatter of no-return float32
 * atomic adds: its bits depend on the order in which the adds arrive, as for srf_roi_extract_bwd.
 * Return codes and their order are srf_msda_fwd's, with grad_out and every non-NULL output held to the same rules (a pitch below the
 * row's width: SRF_EINVAL; 2 GiB or more, a pitch % 4, a base that is not 16-byte aligned: SRF_EUNSUPPORTED); a NULL input with work to
 * do: SRF_EINVAL.  B Q == 0, or all three outputs NULL, is nothing to do (SRF_OK, no launch).  All checks run before any HIP call. */
int srf_msda_bwd(const float *value, long long value_ld, int B, const int *shapes /*host[L][2]*/, int L, const float *ref,
                 const float *offs, long long offs_ld, const float *logits, long long logits_ld, int Q, int heads, int head_dim, int P,
                 const float *grad_out, long long grad_out_ld, float *grad_value, long long grad_value_ld, float *grad_offs,
                 long long grad_offs_ld, float *grad_logits, long long grad_logits_ld, srf_stream_t stream);

/* ---- streaming layers of the channels-last camera branch (csrc/nhwc.hip); all take (N, H, W, ld) channel slices, C % 4 == 0,
 * 16-byte aligned pointers, ld % 4 == 0 ---------------------------------------------------------------------------------
 * Defined exactly by tests/nhwc_ref.py.  Checks, in this order: sizes (negative count, C <= 0, map extent < 1, ld < C: SRF_EINVAL);
 * the empty batch (N, M or B == 0: SRF_OK, nothing read or written, except that srf_nhwc_affine_relu_bwd* zero `sums`; SRF_OK
 * also where HW == 0, which srf_nhwc_colmean / _colsum_prod refuse for N > 0); null pointers (SRF_EINVAL); C % 4, ld % 4, pointer
 * alignment -- the workspace of srf_nhwc_colmean / _colsum_prod included -- and range limits (SRF_EUNSUPPORTED); workspace size
 * (SRF_EWORKSPACE).
 * Non-finite values: ReLU and the pooling maximum are fmaxf, which drops a NaN operand: relu(NaN) = 0 in srf_nhwc_affine and
 * srf_nhwc_dwconv3x3s2*, and a pooling window holding a NaN returns the maximum of its other values, the taps past the bottom /
 * right edge counting as -inf values: nine NaN give NaN, a clipped window of NaN gives -inf (torch returns NaN in both places).  +-inf, and NaN where no fmaxf follows, propagate as IEEE arithmetic has them.  In srf_nhwc_affine_relu_bwd* a NaN
 * in y masks the gradient to 0, and a masked gy (NaN included) reaches neither gz nor the sums.
 * srf_nhwc_affine: y = x * scale[(per_sample & 1 ? n : 0)][c] + shift[(per_sample & 2 ? n : 0)][c] (+ residual), optional ReLU; scale / shift / residual
 *   may be NULL; in place allowed: eval BatchNorm2d + ReLU behind a library convolution, and the eSE gate multiply + OSA
 *   identity add of VoVNet (vovnet.py:165-177, :225-228).  HW = pixels per sample (0: nothing to do).  One f32 rounding per
 *   step (multiply, add shift, add residual); r_ld is ignored when residual is NULL.
 * srf_nhwc_colmean: mean[n][c] over the HW pixels (AdaptiveAvgPool2d(1) of the eSE module), deterministic two-level sum;
 *   C <= 1024.
 * srf_nhwc_maxpool3s2_ceil: MaxPool2d(3, stride 2, ceil_mode=True) (the VoVNet stage pooling) -> (N, Ho, Wo, C); Ho, Wo as
 *   torch's for H, W >= 2; H == 1 or W == 1, which torch refuses, gives the one clipped window (Ho = 1 / Wo = 1).
 * srf_nhwc_upsample_add: y = lat + nearest-upsampled top (the FPN top-down step; F.interpolate 'nearest' index rule).
 * srf_nhwc_dwconv3x3s2: depthwise Conv2d(C, C, 3, stride 2, padding 1, groups=C) + scale / shift (+ ReLU): the stair of the
 *   proposal generator on the camera levels (srfdet_head.py:265-320, :525-536); w is (C, 3, 3). */
int srf_nhwc_affine(const float *x, long long x_ld, int N, long long HW, int C, const float *scale, int per_sample,
                    const float *shift, const float *residual, long long r_ld, int relu, float *y, long long y_ld,
                    srf_stream_t stream);
size_t srf_nhwc_colmean_workspace_bytes(int N, int C);
int srf_nhwc_colmean(const float *x, long long x_ld, int N, long long HW, int C, float *mean, void *workspace,
                     size_t workspace_bytes, srf_stream_t stream);
/* out[n][c] = sum over the pixels of a[n][p][c] * b[n][p][c] (training: the pixel sum behind the gradient of the eSE gate, vovnet.py:165-177);
 * deterministic; workspace: srf_nhwc_colmean_workspace_bytes(N, C). */
int srf_nhwc_colsum_prod(const float *a, long long a_ld, const float *b, long long b_ld, int N, long long HW, int C, float *out /*N x C*/,
                         void *workspace, size_t workspace_bytes, srf_stream_t stream);
int srf_nhwc_maxpool3s2_ceil(const float *x, long long x_ld, int N, int H, int W, int C, float *y, long long y_ld,
                             srf_stream_t stream);
/* srf_nhwc_maxpool3s2_pad1: MaxPool2d(3, stride 2, padding 1), floor mode (the pool behind a ResNet stem) -> (N, Ho, Wo, C),
 *   Ho = (H - 1) / 2 + 1; the padding is -inf.  Arguments, codes and NaN rule of srf_nhwc_maxpool3s2_ceil. */
int srf_nhwc_maxpool3s2_pad1(const float *x, long long x_ld, int N, int H, int W, int C, float *y, long long y_ld,
                             srf_stream_t stream);
int srf_nhwc_upsample_add(const float *lat, long long l_ld, const float *top, long long t_ld, int N, int H, int W, int Ht, int Wt,
                          int C, float *y, long long y_ld, srf_stream_t stream);
int srf_nhwc_dwconv3x3s2(const float *x, long long x_ld, int N, int H, int W, int C, const float *w, const float *scale,
                         const float *shift, int relu, float *y, long long y_ld, srf_stream_t stream);
/* The proposal generator (srfdet_head.py:496-561) without its ~35 small torch launches:
 * srf_nhwc_dwconv3x3s2_cat: one step of the stair (:525-536), x = cat([level, conv(x)], 1): the convolution writes `y` and the
 *   pyramid level `side` (N, Ho, Wo, Cs) is copied to `side_out`, both slices of one concat buffer (row stride y_ld).
 * srf_nhwc_pool_sum: out[b][yo * Wo + xo] = sum over the n_cam images of sample b and the C channels of x at the `nearest`
 *   source pixel of (yo, xo) (F.interpolate to (Ho, Wo) + the camera sum + the channel sum, :537 / :548-552; Ho = H, Wo = W,
 *   n_cam = 1 for the BEV pyramid); out rows have out_ld >= Ho * Wo floats, the tail zero-filled (K padding of fc1).
 * srf_dpg_mix: softmax over the E experts of the logits wl (B, E * P) (with wi: of (wl + wi) / 2), the expert-weighted sums of
 *   the proposal boxes (E * P, D) and features (E * P, C), and the sigmoid of the box centres (:957) -> boxes (B, P, D),
 *   feats (B, P, C).  The logits are expert-major: expert e of proposal p of sample b is wl[(b * E + e) * P + p]; a logit of -inf gives
 *   that expert the weight 0 (every expert of a (b, p) at -inf is not defined).  Checked in this order: B < 0, E outside 1..16,
 *   P <= 0, D < 3, C <= 0: SRF_EINVAL; B == 0: SRF_OK; a NULL wl, boxes_w, feats_w, boxes or feats: SRF_EINVAL (wi may be NULL). */
int srf_nhwc_dwconv3x3s2_cat(const float *x, long long x_ld, int N, int H, int W, int C, const float *w, const float *scale,
                             const float *shift, int relu, float *y, long long y_ld, const float *side, long long side_ld, int Cs,
                             float *side_out, srf_stream_t stream);
/* Training (config 4, tools/train.py:220-234): the backward pass of y = relu(z * s[c] + t[c]) -- a convolution's eval-mode BatchNorm
 * (norm_eval=True, vovnet.py:371) + ReLU, which the forward pass runs as the convolution's epilogue -- over channels-last (M x C)
 * tensors in one pass: gz = (relu ? gy * [y > 0] : gy) * s, sums[0..C) = sum_p gu, sums[C..2C) = sum_p gu * y (gu = the masked gy);
 * deterministic (per-block partials added in block order).  C % 4 == 0, C <= 1024. */
size_t srf_nhwc_affine_relu_bwd_workspace_bytes(long long M, int C);
int srf_nhwc_affine_relu_bwd(const float *gy, long long gy_ld, const float *y, long long y_ld, long long M, int C, const float *scale /*or NULL*/,
                             int relu, float *gz, long long gz_ld, float *sums /*2 C*/, void *workspace, size_t workspace_bytes,
                             srf_stream_t stream);
/* ... with a second gradient of the same output, gy2 (M x C, row stride gy2_ld; NULL: none): gy + gy2 takes the place of gy (one rounding,
 * the add autograd makes as a pass of its own when an output has two consumers -- an OSA layer feeds the next layer AND the block's
 * concat convolution, vovnet.py:208-230). */
int srf_nhwc_affine_relu_bwd2(const float *gy, long long gy_ld, const float *gy2 /*or NULL*/, long long gy2_ld, const float *y, long long y_ld,
                              long long M, int C, const float *scale /*or NULL*/, int relu, float *gz, long long gz_ld, float *sums /*2 C*/,
                              void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* The per-channel arithmetic around an eval-mode BatchNorm2d under training (norm_eval=True, vovnet.py:371; tools/train.py:220-234), C values:
 * srf_bn_eval_fold: out[0..C) = s = gamma / sqrt(var + eps), out[C..2C) = t0 = beta - mean s, out[2C..3C) = inv = 1 / sqrt(var + eps);
 * srf_bn_eval_grads: from sums = srf_nhwc_affine_relu_bwd's [sum gu, sum gu y] and fold = srf_bn_eval_fold's output:
 *   out[0..C) = d gamma = ((s != 0 ? (sum gu y - t0 sum gu) / s : 0) - mean sum gu) inv,  out[C..2C) = d beta = sum gu. */
int srf_bn_eval_fold(const float *gamma, const float *beta, const float *mean, const float *var, float eps, int C, float *out /*3 C*/,
                     srf_stream_t stream);
int srf_bn_eval_grads(const float *sums /*2 C*/, const float *fold /*3 C*/, const float *mean, int C, float *out /*2 C*/, srf_stream_t stream);
int srf_nhwc_pool_sum(const float *x, long long x_ld, int B, int n_cam, int H, int W, int C, int Ho, int Wo, float *out, int out_ld,
                      srf_stream_t stream);
int srf_dpg_mix(const float *wl, const float *wi /*or NULL*/, int B, int E, int P, const float *boxes_w, int D, const float *feats_w,
                int C, float *boxes, float *feats, srf_stream_t stream);

/* srf_stage_tail: the row-local remainder of a stage in one launch (srfdet_head.py:1506-1520): FFN + residual + norm3,
 * classification tower + class_logits, regression tower + bboxes_delta + apply_deltas.  obj_in (R x C) is norm2's
 * output; outputs obj_out (R x C), logits (R x ncls), pred (R x Dd).  cls_/reg_ arrays are HOST arrays of n_cls / n_reg
 * device pointers (weights (C x C), LayerNorm gamma/beta) and host eps values; boxes_m (R x Dd) are the boxes of srf_apply_deltas,
 * weights6 / pc_range / scale_clamp its geometry.
 * Limits, checked in this order: R >= 0, C == 128, F in {128, 256, 384, 512}, 0 <= n_cls, n_reg <= 4, 1 <= ncls <= 32, 8 <= Dd <= 32, else
 * SRF_EUNSUPPORTED; R == 0: SRF_OK, no pointer is touched; a NULL among obj_in, w1, b1, w2, b2, n3_g, n3_b, wl, bl, wd, bd, boxes_m,
 * weights6, pc_range, obj_out, logits, pred: SRF_EINVAL (the tower arrays are read for the first n_cls / n_reg entries only); a workspace
 * shorter than srf_stage_tail_workspace_bytes: SRF_EWORKSPACE, nothing written.  plugin/heads.py::_tail_fusable restates the limits.
 * workspace (srf_stage_tail_workspace_bytes(R, C, F), may be NULL): with it the FFN runs as its own launch, one workgroup per
 * (32 rows, 128 hidden units), and the tail adds the slices in a fixed order (deterministic; the sum of F / 128 partial chains
 * instead of one chain over F, i.e. equal to the in-line FFN to rounding, not bit for bit); without it everything is one launch. */
size_t srf_stage_tail_workspace_bytes(int R, int C, int F);
int srf_stage_tail(const float *obj_in, int R, int C, int F, const float *w1, const float *b1, const float *w2,
                   const float *b2, const float *n3_g, const float *n3_b, float n3_eps, int n_cls,
                   const float *const *cls_w, const float *const *cls_g, const float *const *cls_b, const float *cls_eps,
                   int n_reg, const float *const *reg_w, const float *const *reg_g, const float *const *reg_b,
                   const float *reg_eps, const float *wl, const float *bl, int ncls, const float *wd, const float *bd,
                   int Dd, const float *boxes_m, const float *weights6, const float *pc_range, float scale_clamp,
                   float *obj_out, float *logits, float *pred, void *workspace, size_t workspace_bytes, srf_stream_t stream);
int srf_apply_deltas(const float *deltas, const float *boxes, int R, int Dd, const float *weights6 /*host[6]*/,
                     const float *pc_range /*host[6]*/, float scale_clamp, float *out, srf_stream_t stream);
/* srf_decode_boxes: the tensors the reference hands to box3d_multiclass_nms (srfdet_head.py:1246-1271, after the
 * centres-to-metres step that ends `forward`, :1002-1006) from the last stage's outputs in one launch: logits (R, ncls) ->
 * scores = sigmoid; pred (R, Dd) [centres normalised to pc_range, log sizes, sin, cos, (vx, vy)] -> boxes (R, Dd - 1)
 * [x, y, bottom-centre z in metres, w, l, h, yaw, (vx, vy)]. */
int srf_decode_boxes(const float *logits, const float *pred, int R, int ncls, int Dd, const float *pc_range /*host[6]*/,
                     float *scores, float *boxes, srf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * K8  rotated BEV NMS.
 * Replaces mmcv nms_rotated behind mmdet3d box3d_multiclass_nms, called at srfdet_head.py:1288-1293.
 * boxes: (n,5) [cx, cy, w, h, angle(rad)] already sorted by descending score; keep[i] = 1 if box i survives
 * greedy suppression at IoU > iou_threshold.  n <= 4096, else SRF_EUNSUPPORTED.  The IoU is K9's: within 1e-5 of the exact
 * IoU of the two float32 boxes, also for (nearly) identical boxes, boxes that share edges or corners, the same rectangle
 * written with yaw + pi or as (h, w, yaw + pi/2), thin boxes, yaw outside [-pi, pi] and centres kilometres from the origin; a
 * box with w * h < 1e-14 has IoU 0 with every box.
 * ------------------------------------------------------------------------------------------------------- */
/* K9 pairwise rotated BEV IoU (n x m), boxes (cx, cy, w, h, angle): mmcv box_iou_rotated under mmdet3d
 * BboxOverlaps3D, used by OTAssignerSRFDet (mmdet3d_plugin/core/bbox/assigners/ota_srfdet.py:148-150).
 * iou[i * m + j] is within 1e-5 of the exact IoU of boxes_a[i] and boxes_b[j] and a continuous function of the ten numbers
 * (no in/out or parallel-edge decision: the intersection area is a boundary integral in boxes_a[i]'s frame, csrc/nms.hip);
 * 0 when either box has w * h < 1e-14. */
/* srf_host_pack: the one vector a frame's host side reads back -- packed detections a (na floats), [survivors, candidates] b (nb ints),
 * live row counts of the sparse levels c (nc ints) -> out (na + nb + nc floats; the integers are < 2^24, exact).  One launch. */
int srf_host_pack(const float *a, int na, const int *b, int nb, const int *c, int nc, float *out, srf_stream_t stream);
int srf_box_iou_rotated(const float *boxes_a, int n, const float *boxes_b, int m, float *iou, srf_stream_t stream);

/* The dynamic-k OTA label assignment of training (OTAssignerSRFDet, ota_srfdet.py:18-327) for all S decoder stages and B samples of a step
 * (csrc/ota.hip, whose header holds the exact definition; tests/ota_ref.py is the same text in numpy).
 *
 * srf_ota_assign: pred_boxes (S, B, P, D) normalised boxes, columns 0..7 are read; pred_logits (S, B, P, C); gt_boxes (B, Gpad, 7) gravity
 * centre [x, y, z, dx, dy, dz, yaw], padded; gt_labels (B, Gpad) int32 (clamped into [0, C)); n_gt (B) int32 live boxes per sample (clamped
 * into [0, Gpad]; the padding is never read); head_idx (S) int32; the weights of FocalLossCost / BBox3DL1Cost / IoU3DCost, the focal
 * alpha / gamma / eps, center_radius, candidate_topk and num_heads of the assigner.  Fixed-shape outputs, nothing is read back: count (S, B)
 * matched predictions; pred_idx (S, B, P) their indices ascending in the first count slots; gt_idx (S, B, P) the matched ground truth of each
 * (the first matched column); the other slots hold -1; status (S, B) 0, or 1 when the repair loop reached its cap of 32 iterations.
 * Two launches (cost, match), no float atomics: two calls give the same bytes.  workspace: srf_ota_workspace_bytes(S, B, P, Gpad).
 *
 * srf_ota_cost / srf_ota_match are the two stages on the caller's own matrices, g-major: cost and iou (S, B, Gpad, P) f32, columns
 * g >= n_gt[b] untouched.  srf_ota_match adds 100000 to rows of `cost` in place when it has to repair; its workspace holds the match bytes:
 * srf_ota_match_workspace_bytes(S, B, P, Gpad).
 *
 * Checked before any HIP call, in this order: non-positive S, B, P, Gpad, D, C or candidate_topk: SRF_EINVAL; null pointers: SRF_EINVAL;
 * limits (P <= 4096: a byte of LDS per row; Gpad <= 512: an int of LDS per column; S * B <= 65535; D in {8, 10}; C <= 64; S * B * P * Gpad
 * and S * B * P * C floats below 2^31 bytes): SRF_EUNSUPPORTED; workspace too small: SRF_EWORKSPACE.  The workspace sizes are 0 outside
 * the limits. */
size_t srf_ota_workspace_bytes(int S, int B, int P, int Gpad);
size_t srf_ota_match_workspace_bytes(int S, int B, int P, int Gpad);
int srf_ota_cost(const float *pred_boxes, const float *pred_logits, const float *gt_boxes, const int *gt_labels, const int *n_gt, int S, int B,
                 int P, int D, int C, int Gpad, float w_cls, float w_reg, float w_iou, float alpha, float gamma, float eps, float center_radius,
                 float *cost, float *iou, srf_stream_t stream);
int srf_ota_match(float *cost, const float *iou, const int *n_gt, const int *head_idx, int S, int B, int P, int Gpad, int candidate_topk,
                  int num_heads, int *count, int *pred_idx, int *gt_idx, int *status, void *workspace, size_t workspace_bytes,
                  srf_stream_t stream);
int srf_ota_assign(const float *pred_boxes, const float *pred_logits, const float *gt_boxes, const int *gt_labels, const int *n_gt,
                   const int *head_idx, int S, int B, int P, int D, int C, int Gpad, float w_cls, float w_reg, float w_iou, float alpha,
                   float gamma, float eps, float center_radius, int candidate_topk, int num_heads, int *count, int *pred_idx, int *gt_idx,
                   int *status, void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* The losses of the decoder's deep supervision on the assignment srf_ota_assign made: sigmoid focal loss and weighted L1 loss (FocalLoss /
 * L1Loss, reduction "sum") of all S decoder stages and B samples of a step, values and gradients in one pass (csrc/setloss.hip, whose header
 * holds the exact definition; tests/set_loss_ref.py is the same text in numpy).
 *
 * pred_logits (S, B, P, C); pred_boxes (S, B, P, D) normalised boxes; count (S, B), pred_idx / gt_idx (S, B, P) as srf_ota_assign writes
 * them (count is clamped into [0, P]; a slot whose pred_idx is outside [0, P) or whose gt_idx is outside [0, Gpad) is skipped); gt_boxes
 * (B, Gpad, Dg) gravity centre [x, y, z, dx, dy, dz, yaw, (vx, vy)], padded; gt_labels (B, Gpad) int32, a label outside [0, C) is
 * background; code_weights (Dw) on the device; num (S, 2) on the HOST: the divisor of the class loss and of the box loss of each stage;
 * alpha / gamma / w_cls = loss_weight of the focal loss, w_box = loss_weight of the L1 loss.
 * Outputs, every element written: loss (S, 2) = [class loss, box loss] per stage after nan_to_num; grad_logits (S, B, P, C) and grad_boxes
 * (S, B, P, D) = the derivatives of loss[s, 0] and loss[s, 1] by the stage's own predictions.  A stage whose loss value is not finite
 * gets the nan_to_num value and all-zero gradients for that loss.
 * Two launches per 64 stages (element pass with per-workgroup float64 partial sums, fixed-order reduction), no float atomics: two calls
 * give the same bytes.  workspace: srf_set_loss_workspace_bytes(S, B, P, C, D).
 *
 * Checked before any HIP call, in this order: non-positive S, B, P, C, D, Dw, Gpad or Dg, or a num[s][k] that is <= 0 or not finite:
 * SRF_EINVAL; null pointers: SRF_EINVAL; limits (P <= 4096; Gpad <= 512; S * B <= 65535; C <= 64; (D, Dw, Dg) one of (8, 8, 7), (10, 8, 7),
 * (10, 8, 9), (10, 10, 9); gamma >= 1 and finite; alpha in [0, 1]; every tensor below 2^31 bytes): SRF_EUNSUPPORTED; workspace too small:
 * SRF_EWORKSPACE.  The workspace size is 0 outside the limits. */
size_t srf_set_loss_workspace_bytes(int S, int B, int P, int C, int D);
int srf_set_loss(const float *pred_logits, const float *pred_boxes, const int *count, const int *pred_idx, const int *gt_idx,
                 const float *gt_boxes, const int *gt_labels, const float *code_weights, const float *num, int S, int B, int P, int C, int D,
                 int Dw, int Gpad, int Dg, float alpha, float gamma, float w_cls, float w_box, float *loss, float *grad_logits,
                 float *grad_boxes, void *workspace, size_t workspace_bytes, srf_stream_t stream);

size_t srf_nms_rotated_workspace_bytes(int n);
int srf_nms_rotated(const float *boxes, int n, float iou_threshold, int *keep, void *workspace, size_t workspace_bytes,
                    srf_stream_t stream);
/* the same over the first *n_dev (device int, <= n) boxes only; keep[i] = 0 for the rest.  A fixed-shape form for
 * hipGraph replay: n is the capacity, the number of candidates above the score threshold is decided on the device. */
int srf_nms_rotated_counted(const float *boxes_xywhr, int n, const int *n_dev, float iou_threshold, int *keep,
                            void *workspace, size_t workspace_bytes, srf_stream_t stream);
/* class-aware: cls (n, int64) -- a box only suppresses boxes of its own class, i.e. the per-class loop of mmdet3d
 * box3d_multiclass_nms (mmdet3d/core/post_processing/box3d_nms.py as called at srfdet_head.py:1276-1293) in one pass on the
 * boxes' own coordinates (no class offsets added to x).  n_dev may be NULL (all n boxes are candidates). */
int srf_nms_rotated_classes(const float *boxes_xywhr, const long long *cls, int n, const int *n_dev, float iou_threshold,
                            int *keep, void *workspace, size_t workspace_bytes, srf_stream_t stream);

/* The fixed-shape multi-class selection around srf_nms_rotated_classes: the static form of mmdet3d box3d_multiclass_nms as
 * called at srfdet_head.py:1276-1293, without a host read-back (hipGraph replay).
 * srf_nms_select: boxes (n, D >= 7) [x, y, z, w, l, h, yaw, ...], scores (n, C) -> the L best (box, class) pairs above
 * score_thr in descending score: cand (L, D), top_s (L), cls (L, int64), bev (L, 5) = [x, y, w, l, yaw] (with cls the
 * operands of srf_nms_rotated_classes), *m (device int) = number of pairs above the threshold -- if it exceeds L the caller redoes the frame on the dynamic
 * path.  n * C <= 16384, L <= n * C.
 * srf_nms_finish: keep (L) from srf_nms_rotated_classes -> survivors first, class-major, descending score inside a class
 * (the order of the reference's per-class loop): out_boxes (L, D), out_scores (L), out_labels (L, int64), *kept. */
int srf_nms_select(const float *boxes, const float *scores, int n, int C, int D, float score_thr, int L, float *cand,
                   float *top_s, long long *cls, float *bev, int *m, srf_stream_t stream);
int srf_nms_finish(const float *cand, const float *top_s, const long long *cls, const int *keep, int L, int D,
                   float *out_boxes, float *out_scores, long long *out_labels, int *kept,
                   float *packed /* (L, D+2) rows [box, score, label] for one D2H copy, or NULL */,
                   const int *m /* srf_nms_select's count */, int *counts /* [kept, m] or NULL */, srf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRFDET3D_H */
