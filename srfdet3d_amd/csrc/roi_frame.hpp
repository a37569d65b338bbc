// roi_frame.hpp -- what the RoI kernels of roi.hip and roi_bwd_ordered.hip share: the limits of the C ABI, the level table a launch
// carries, and the float32 rule that maps a RoI to its level (mmdet SingleRoIExtractor.map_roi_levels, op by op).
#pragma once
#include "common.hpp"

#define SRF_MAX_LEVELS 4
#define SRF_MAX_POOLED 8
#define SRF_MAX_SR 4

struct RoiLevels {
    srf_featmap lv[SRF_MAX_LEVELS];
    int num;
};

struct RoiGradLevels {
    float *grad[SRF_MAX_LEVELS];
};

__device__ __forceinline__ int srf_roi_level(const float *b, int num_levels, float finest_scale)
{
    float area = __fmul_rn(__fsub_rn(b[3], b[1]), __fsub_rn(b[4], b[2]));
    float scale = sqrtf(area);
    float t = floorf(log2f(__fadd_rn(__fdiv_rn(scale, finest_scale), 1e-6f)));
    if (!(t == t)) return 0;
    return t < 0.0f ? 0 : (t > (float)(num_levels - 1) ? num_levels - 1 : (int)t);
}
