// mc_proj_plan.hpp — the arithmetic of the projected boxes shared by the host and the device
// (get_top_images.py:204-237, get_bbox_by_projection): one world point into one camera, the box
// accumulator of one request, its status, and the draw clamp of draw_red_bbox (:262-272).
// Everything is float64 exactly as written: the three camera coordinates are ((r0*x + r1*y) + r2*z) + t,
// each product and sum rounded on its own, u = fx * (x / z) + cx in three rounded operations; no
// product feeds an addition through a fused multiply-add (contraction is off for this file, and
// the library is built with -ffp-contract=off).  Compiles as plain C++ (scripts/proj_plan_check.cpp)
// and inside the kernels.
#pragma once

#include <climits>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_PROJ_HD __host__ __device__ inline
#else
#define MC_PROJ_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mc {

constexpr int kProjOk = 0;       // status of a request
constexpr int kProjBehind = 1;   // no point with z > 0 (the reference returns None at :215-216)
constexpr int kProjOutside = 2;  // no point in the image (:228-229)
constexpr int kProjMaxTop = 16;  // requests of one object a workgroup serves at once; the largest top_k
constexpr int kProjChunk = 4096; // points of an object one workgroup takes per turn
constexpr int kProjMaxSide = 1 << 30;

constexpr int kProjBehindPoint = 0, kProjFrontPoint = 1, kProjInsidePoint = 2;  // proj_point's result

// One point through world_to_cam (row-major 4 x 4; the last row is not read: no division by w) and
// (fx, fy, cx, cy).  z > 0 strictly, a NaN z is behind.  The rounded pixel is tested in floating
// point (-0.0 is pixel 0; NaN, +-inf and values int cannot hold are outside) and converted after.
MC_PROJ_HD int proj_point(const double *m, const double *k, double x, double y, double z, int width, int height, int *px,
                          int *py)
{
    const double zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    if (!(zc > 0.0)) return kProjBehindPoint;
    const double xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const double yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const double qx = xc / zc, qy = yc / zc;
    const double sx = k[0] * qx, sy = k[1] * qy;
    const double u = sx + k[2], v = sy + k[3];
    const double ru = rint(u), rv = rint(v);  // round half to even (np.round)
    if (!(ru >= 0.0 && ru < static_cast<double>(width) && rv >= 0.0 && rv < static_cast<double>(height)))
        return kProjFrontPoint;
    *px = static_cast<int>(ru);
    *py = static_cast<int>(rv);
    return kProjInsidePoint;
}

// The accumulator of one request: pixel bounds of the in-bounds points, their count, and whether any
// point was in front of the camera.  Merging two of them is order-independent.
struct ProjAcc {
    int x0, y0, x1, y1, inside, front;
};

MC_PROJ_HD void proj_acc_init(ProjAcc *a)
{
    a->x0 = a->y0 = INT_MAX;
    a->x1 = a->y1 = INT_MIN;
    a->inside = a->front = 0;
}

MC_PROJ_HD void proj_acc_add(ProjAcc *a, int kind, int px, int py)
{
    if (kind == kProjBehindPoint) return;
    a->front = 1;
    if (kind != kProjInsidePoint) return;
    a->x0 = px < a->x0 ? px : a->x0;
    a->y0 = py < a->y0 ? py : a->y0;
    a->x1 = px > a->x1 ? px : a->x1;
    a->y1 = py > a->y1 ? py : a->y1;
    a->inside++;
}

// status and (min px, min py, max px, max py) of a finished accumulator; the box of a request without one is 0
MC_PROJ_HD int proj_acc_box(const ProjAcc *a, int32_t box[4])
{
    const bool ok = a->front && a->inside > 0;
    box[0] = ok ? a->x0 : 0, box[1] = ok ? a->y0 : 0, box[2] = ok ? a->x1 : 0, box[3] = ok ? a->y1 : 0;
    return !a->front ? kProjBehind : (a->inside > 0 ? kProjOk : kProjOutside);
}

// draw_red_bbox (:266-272): the corners it hands to cv2.rectangle, each clamped into
// [margin, side - 1 - margin] with margin = thickness // 2 (max outside min: a frame smaller than
// the margins gives min > max, as in the reference)
MC_PROJ_HD void proj_draw_clamp(const int32_t box[4], int width, int height, int thickness, int32_t out[4])
{
    const int margin = thickness / 2;
    for (int i = 0; i < 4; i++) {
        const int hi = ((i & 1) ? height : width) - 1 - margin;
        const int v = box[i] < hi ? box[i] : hi;
        out[i] = margin > v ? margin : v;
    }
}

}  // namespace mc
