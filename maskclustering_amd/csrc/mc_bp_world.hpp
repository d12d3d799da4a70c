// mc_bp_world.hpp — S1 voxels: a mask pixel's world point (Open3D create_from_depth_image + transform, in
// double, no FMA but div_rn's own; oracle/s1_oracle.c (a1), (u1)).
// Plain C++17 without a HIP include, usable from host and device: the voxel kernels (mc_bp_voxel.inl)
// compute every pixel's point with these functions, and scripts/bp_world_check.cpp checks them on the CPU
// (tests/test_bp_world_cpu.py).  Build with -ffp-contract=off: every operation is rounded where it stands.
//  * div_rn(a, b, rb) is a / b rounded to nearest from rb = RN(1 / b) (Markstein: q0 = RN(a rb),
//    r = a - b q0 is exact by FMA, and RN(q0 + r rb) is the correctly rounded quotient for normal operands
//    whose quotient neither overflows nor underflows): a multiply and two FMAs, the same bits as a / b
//    (tests/test_div_rn_cpu.py checks the identity on operands of the ranges here).
//  * bp_world is the general form: camera point (x, y, z), the four rows of the pose, the homogeneous
//    divide by row 3's value w unless w == 1.  The compiler turns that choice into a per-pixel select, so
//    the three IEEE divisions and row 3 are computed for every pixel and thrown away for a rigid pose.
//  * bp_world_affine is the same without row 3 and without the divide; bp_world_lin is bp_world_affine
//    without the translation column.
//  * bp_pose_affine(K, T, trunc) says when bp_world_affine returns bp_world's bits for every pixel the
//    kernels can see.  It holds iff
//        T[12] == 0, T[13] == 0, T[14] == 0 (either sign), T[15] == 1,
//        |T[i]| <= 2^64 for i < 12,  2^-64 <= |fx|, |fy| <= 2^64,  |cx|, |cy| <= 2^64,  trunc <= 2^128
//    (every comparison false for a NaN, so a NaN anywhere rejects).
//    Proof.  A listed pixel has integer 0 <= u, v < 2^31 and a float depth 0 < d < trunc (k_bp_count), so
//    0 < z <= 2^128.  |u - cx| <= 2^65, |(u - cx) z| <= 2^193; rb = RN(1 / fx) has |rb| <= 2^64, so in
//    div_rn |q0| <= 2^257, |b q0| <= 2^321, |r| <= 2^322, and |x| <= 2^258 + 2^386: finite, and so is y.  With
//    finite x, y, z the products T[12] x, T[13] y, T[14] z are zeros of either sign, their sums are
//    zeros, and a zero plus 1 is exactly 1: w == 1, the general form takes its `unit` branch and returns
//    r[0], r[1], r[2], which are the expressions bp_world_affine evaluates, in the same order.  (The two
//    forms' rows 0-2 are the same operations on the same operands whatever the predicate says: NaNs included.)
//  * The minimum over a slot's pixels (the voxel grid's origin) may be taken over bp_world_lin's values
//    and the translation added once: under the predicate every s = bp_world_lin value is finite
//    (|s| <= 3 * 2^64 * 2^387), t = T[4 c + 3] is finite, and s <= s' implies RN(s + t) <= RN(s' + t)
//    (rounding is monotone), so min_i RN(s_i + t) = RN(min_i s_i + t): the same double.  (Signed zeros:
//    the minimum may differ in a zero's sign only; the kernels subtract half a voxel from it first thing,
//    which gives the same double for either zero.)
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define MC_BW_HD __host__ __device__ __forceinline__
#else
#define MC_BW_HD inline
#endif

namespace mc {

MC_BW_HD double div_rn(double a, double b, double rb)
{
    const double q0 = a * rb;
    const double r = fma(-b, q0, a);
    return fma(r, rb, q0);
}

// the per-frame reciprocals of bp_world's divisors: rk[0] = RN(1 / fx), rk[1] = RN(1 / fy)
MC_BW_HD void bp_recip(const double *K, double rk[2])
{
    rk[0] = 1.0 / K[0];
    rk[1] = 1.0 / K[1];
}

// the camera point of pixel (u, v) at depth d
MC_BW_HD void bp_camera(const double *K, int u, int v, float d, const double *rk, double &x, double &y, double &z)
{
    z = static_cast<double>(d);
    x = div_rn((static_cast<double>(u) - K[2]) * z, K[0], rk[0]);
    y = div_rn((static_cast<double>(v) - K[3]) * z, K[1], rk[1]);
}

// any pose
MC_BW_HD void bp_world(const double *K, const double *T, int u, int v, float d, double &ox, double &oy, double &oz,
                       const double *rk)
{
    double x, y, z;
    bp_camera(K, u, v, d, rk, x, y, z);
    double r[4];
    for (int k = 0; k < 4; k++) r[k] = (((T[4 * k] * x) + (T[4 * k + 1] * y)) + (T[4 * k + 2] * z)) + T[4 * k + 3];
    // the homogeneous divide is the identity when w == 1 (a select per pixel: both sides are computed)
    const bool unit = r[3] == 1.0;
    ox = unit ? r[0] : r[0] / r[3];
    oy = unit ? r[1] : r[1] / r[3];
    oz = unit ? r[2] : r[2] / r[3];
}

// rows 0-2 without the translation column
MC_BW_HD void bp_world_lin(const double *K, const double *T, int u, int v, float d, double &ox, double &oy, double &oz,
                           const double *rk)
{
    double x, y, z;
    bp_camera(K, u, v, d, rk, x, y, z);
    ox = ((T[0] * x) + (T[1] * y)) + (T[2] * z);
    oy = ((T[4] * x) + (T[5] * y)) + (T[6] * z);
    oz = ((T[8] * x) + (T[9] * y)) + (T[10] * z);
}

// a pose for which bp_pose_affine holds: no row 3, no divide
MC_BW_HD void bp_world_affine(const double *K, const double *T, int u, int v, float d, double &ox, double &oy,
                              double &oz, const double *rk)
{
    bp_world_lin(K, T, u, v, d, ox, oy, oz, rk);
    ox = ox + T[3];
    oy = oy + T[7];
    oz = oz + T[11];
}

MC_BW_HD bool bp_pose_affine(const double *K, const double *T, double trunc)
{
    constexpr double kBig = 0x1p64, kSmall = 0x1p-64;
    bool ok = T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0 && trunc <= 0x1p128;
    for (int i = 0; i < 12; i++) ok = ok && fabs(T[i]) <= kBig;
    for (int i = 0; i < 4; i++) ok = ok && fabs(K[i]) <= kBig;
    return ok && fabs(K[0]) >= kSmall && fabs(K[1]) >= kSmall;
}

template <bool kAffine>
MC_BW_HD void bp_world_as(const double *K, const double *T, int u, int v, float d, double &ox, double &oy, double &oz,
                          const double *rk)
{
    if (kAffine) bp_world_affine(K, T, u, v, d, ox, oy, oz, rk);
    else bp_world(K, T, u, v, d, ox, oy, oz, rk);
}

}  // namespace mc
