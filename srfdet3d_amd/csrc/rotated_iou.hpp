// rotated_iou.hpp -- the rotated BEV IoU of two (cx, cy, w, h, angle[rad]) boxes as one device function, shared by the NMS
// (nms.hip) and the OTA label assignment (ota.hip).  The method and its error bound are described at the top of nms.hip;
// tests/test_gpu_rotated_iou.py pins its bits.
#pragma once
#include "common.hpp"

__device__ __forceinline__ float srf_clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// mean of clamp(y, -h, h) over a segment along which y runs linearly from y0 to y1: the integrand is piecewise linear with
// kinks where y crosses -h and +h, so the trapezoid rule on the nodes {0, the two crossings clamped onto the segment, 1} is
// exact, and an ill-conditioned crossing (y0 ~ y1) only moves a node along a stretch where the integrand is flat to O(y1 - y0)
__device__ __forceinline__ float srf_clamped_mean(float y0, float y1, float h)
{
    const float dy = y1 - y0;
    const float inv = fabsf(dy) > 1e-30f ? 1.0f / dy : 0.0f;
    const float u = srf_clampf((-h - y0) * inv, 0.0f, 1.0f), v = srf_clampf((h - y0) * inv, 0.0f, 1.0f);
    const float lo = fminf(u, v), hi = fmaxf(u, v);
    const float g0 = srf_clampf(y0, -h, h), gl = srf_clampf(y0 + lo * dy, -h, h), gh = srf_clampf(y0 + hi * dy, -h, h),
                g1 = srf_clampf(y1, -h, h);
    return 0.5f * (lo * (g0 + gl) + (hi - lo) * (gl + gh) + (1.0f - hi) * (gh + g1));
}

// one edge (x0, y0) -> (x1, y1) of the other box: the integral of clamp(y, -hy, hy) dx over the part of the edge inside the
// slab |x| <= hx.  x is monotone along the edge, so that part runs from clamp(x0) to clamp(x1).
__device__ __forceinline__ float srf_edge_term(float x0, float y0, float x1, float y1, float hx, float hy)
{
    const float dx = x1 - x0, dy = y1 - y0;
    const float c0 = srf_clampf(x0, -hx, hx), c1 = srf_clampf(x1, -hx, hx);
    const float inv = fabsf(dx) > 1e-30f ? 1.0f / dx : 0.0f;
    const float ta = srf_clampf((c0 - x0) * inv, 0.0f, 1.0f), tb = srf_clampf((c1 - x0) * inv, 0.0f, 1.0f);
    return (c1 - c0) * srf_clamped_mean(y0 + ta * dy, y0 + tb * dy, hy);
}

__device__ float srf_rotated_iou(const float *a, const float *b)
{
    const float area1 = a[2] * a[3], area2 = b[2] * b[3];
    if (area1 < 1e-14f || area2 < 1e-14f) return 0.0f;
    // b in a's frame: the differences of nearby centres and angles are exact in float32 however far the pair is from the origin
    const float ca = cosf(a[4]), sa = sinf(a[4]);
    const float dx = b[0] - a[0], dy = b[1] - a[1];
    const float ox = ca * dx + sa * dy, oy = ca * dy - sa * dx;
    // the angle between them as dt + de exactly (two-sum): for yaws of several radians the rounding of the difference alone,
    // 5e-7 rad at |dt| > 8, would move the far corners of a 12 m box by 3e-6 m
    const float dt = b[4] - a[4];
    const float bv = dt - b[4], av = dt - bv;
    const float de = (b[4] - av) + (-a[4] - bv);
    const float cd = cosf(dt), sd = sinf(dt);
    const float c = (cd - de * sd) * 0.5f, s = (sd + de * cd) * 0.5f;
    const float ux = c * b[2], uy = s * b[2], vx = -s * b[3], vy = c * b[3];  // b's half axes
    const float x0 = ox - ux - vx, y0 = oy - uy - vy, x1 = ox + ux - vx, y1 = oy + uy - vy;
    const float x2 = ox + ux + vx, y2 = oy + uy + vy, x3 = ox - ux + vx, y3 = oy - uy + vy;
    const float hx = a[2] * 0.5f, hy = a[3] * 0.5f;
    // area(Q and R) = | closed integral over Q's boundary of 1[|x| <= hx] clamp(y, -hy, hy) dx |  (Green's theorem; R's own
    // sides inside Q are vertical cuts with dx = 0)
    const float sum = srf_edge_term(x0, y0, x1, y1, hx, hy) + srf_edge_term(x1, y1, x2, y2, hx, hy) +
                      srf_edge_term(x2, y2, x3, y3, hx, hy) + srf_edge_term(x3, y3, x0, y0, hx, hy);
    const float inter = fminf(fabsf(sum), fminf(area1, area2));
    return inter / (area1 + area2 - inter);
}
