// cc_pose_math.h — the odometry pose interpolation of the KITTI loader (kitti_loader.cpp:297-328), one text for host and gfx950 device
// (include/cc_poses.h).
//
// interpolate() restates cc_kitti.hip's host `interpolate` operation for operation: lower_bound, the raw sample at and beyond both ends,
// Eigen's matrix -> quaternion conversion, slerp and toRotationMatrix in their evaluation order, the translation's lerp. The one
// difference: slerp's acos and its three sin do not come from a libm (glibc picks FMA or non-FMA variants per CPU, OCML is a third
// implementation) but from acos01 / sin_q1 below, which use IEEE + - * / sqrt only. Compiled with -ffp-contract=off nothing is fused, so
// the host half and the device half of a .hip file compute the same bits, on any host.
//
// The two functions cover what slerp asks of them and no more: acos01 on [0, 1) (abs_d < 1 - eps), sin_q1 on [0, pi/2] (theta, and
// theta scaled by f and 1 - f in [0, 1]). The polynomial coefficients are this project's own (tools/pose_math_coeffs.py derives and
// prints them: interpolation at Chebyshev nodes with mpmath, rounded to double; the approximation error of each kernel is below 2^-57
// relative, 1/16 of a rounding). Nothing here is taken from a libm.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CCP_HD __host__ __device__ inline
#else
#define CCP_HD static inline
#endif

namespace ccp
{

constexpr double PIO2_HI = 0x1.921fb54442d18p+0; // pi/2 rounded
constexpr double PIO2_LO = 0x1.1a62633145c07p-54; // pi/2 - PIO2_HI
constexpr double PIO4 = 0x1.921fb54442d18p-1;

// asin x = x + x z A(z), z = x^2 in [0, 1/4]
CCP_HD double asin_tail(double z)
{
    const double a0 = 0x1.5555555555555p-3, a1 = 0x1.3333333333388p-4, a2 = 0x1.6db6db6dac1e0p-5, a3 = 0x1.f1c71c7a52ba3p-6,
                 a4 = 0x1.6e8ba123e494cp-6, a5 = 0x1.1c4efce23019fp-6, a6 = 0x1.c990ad3d8fdcap-7, a7 = 0x1.7b027ee1dd585p-7,
                 a8 = 0x1.3b49de7121487p-7, a9 = 0x1.31622469ce5adp-7, a10 = 0x1.8f193743418ffp-9, a11 = 0x1.406192d124629p-6,
                 a12 = -0x1.3b416bb7d9257p-6, a13 = 0x1.e529c6fce9bb4p-6;
    return z * (a0 + z * (a1 + z * (a2 + z * (a3 + z * (a4 + z * (a5 + z * (a6 + z * (a7 + z * (a8 + z * (a9 + z * (a10 + z * (a11 +
           z * (a12 + z * a13)))))))))))));
}

// acos on [0, 1). Below 1/2: pi/2 - asin x, with pi/2 in two parts. From 1/2: 2 asin(sqrt z), z = (1 - x) / 2 (1 - x is exact there);
// sqrt z is taken as df + c, df its upper half (df * df is exact) and c = (z - df^2) / (s + df), so the rounding of the square root
// does not reach the result.
CCP_HD double acos01(double x)
{
    if (x < 0.5)
    {
        const double r = asin_tail(x * x);
        return PIO2_HI - (x - (PIO2_LO - x * r));
    }
    const double z = (1.0 - x) * 0.5;
    const double s = __builtin_sqrt(z);
    const double r = asin_tail(z);
    const double df = __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, s) & 0xFFFFFFFF00000000ull);
    const double c = (z - df * df) / (s + df);
    return 2.0 * (df + (s * r + c));
}

// sin on [0, pi/2]. Up to pi/4: x + x z S(z). Above: cos y, y = pi/2 - x as y + yl (PIO2_HI - x is exact there),
// cos y = 1 - z/2 + z^2 C(z) summed from its large end with the rounding of 1 - z/2 put back, and - y yl for the low part of y.
CCP_HD double sin_q1(double x)
{
    if (x <= PIO4)
    {
        const double s0 = -0x1.5555555555555p-3, s1 = 0x1.1111111111110p-7, s2 = -0x1.a01a01a01990ap-13, s3 = 0x1.71de3a545b148p-19,
                     s4 = -0x1.ae6454093c147p-26, s5 = 0x1.61217781a8ccdp-33, s6 = -0x1.ab13654fd392ap-41;
        const double z = x * x;
        return x + x * (z * (s0 + z * (s1 + z * (s2 + z * (s3 + z * (s4 + z * (s5 + z * s6)))))));
    }
    const double c0 = 0x1.5555555555555p-5, c1 = -0x1.6c16c16c16955p-10, c2 = 0x1.a01a019f4a826p-16, c3 = -0x1.27e4fa1272706p-22,
                 c4 = 0x1.1eeb634b132cdp-29, c5 = -0x1.907999e6897e2p-37;
    const double t = PIO2_HI - x;
    const double y = t + PIO2_LO;
    const double yl = (t - y) + PIO2_LO;
    const double z = y * y;
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double p = z * (z * (c0 + z * (c1 + z * (c2 + z * (c3 + z * (c4 + z * c5))))));
    return w + (((1.0 - w) - hz) + (p - y * yl));
}

// ---- the pose arithmetic of cc_kitti.hip, same evaluation order ----------------------------------------------------------------------
// 3x4 row-major [R|t]

struct Quat
{
    double c[4]; // x, y, z, w (Eigen's coefficient order)
};

CCP_HD Quat quat_from_rotation(const double* m) // QuaternionBase::operator=(MatrixBase) for 3x3 (Eigen/src/Geometry/Quaternion.h)
{
    Quat q;
    double t = (m[0] + m[5]) + m[10];
    if (t > 0.0)
    {
        t = __builtin_sqrt(t + 1.0);
        q.c[3] = 0.5 * t;
        t = 0.5 / t;
        q.c[0] = (m[9] - m[6]) * t;
        q.c[1] = (m[2] - m[8]) * t;
        q.c[2] = (m[4] - m[1]) * t;
    }
    else
    {
        int i = 0;
        if (m[5] > m[0])
            i = 1;
        if (m[10] > m[i * 5])
            i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = __builtin_sqrt(m[i * 5] - m[j * 5] - m[k * 5] + 1.0);
        q.c[i] = 0.5 * t;
        t = 0.5 / t;
        q.c[3] = (m[k * 4 + j] - m[j * 4 + k]) * t;
        q.c[j] = (m[j * 4 + i] + m[i * 4 + j]) * t;
        q.c[k] = (m[k * 4 + i] + m[i * 4 + k]) * t;
    }
    return q;
}

CCP_HD Quat quat_slerp(const Quat& a, double t, const Quat& b) // QuaternionBase::slerp
{
    const double one = 1.0 - 2.220446049250313e-16;
    // 4-coefficient dot product as two 2-wide packets: (x x' + z z') + (y y' + w w')
    const double d = (a.c[0] * b.c[0] + a.c[2] * b.c[2]) + (a.c[1] * b.c[1] + a.c[3] * b.c[3]);
    const double abs_d = __builtin_fabs(d);
    double scale0, scale1;
    if (abs_d >= one)
    {
        scale0 = 1.0 - t;
        scale1 = t;
    }
    else
    {
        const double theta = acos01(abs_d);
        const double sin_theta = sin_q1(theta);
        scale0 = sin_q1((1.0 - t) * theta) / sin_theta;
        scale1 = sin_q1(t * theta) / sin_theta;
    }
    if (d < 0.0)
        scale1 = -scale1;
    Quat q;
    for (int i = 0; i < 4; i++)
        q.c[i] = scale0 * a.c[i] + scale1 * b.c[i];
    return q;
}

CCP_HD void quat_to_rotation(const Quat& q, double* out) // QuaternionBase::toRotationMatrix
{
    const double x = q.c[0], y = q.c[1], z = q.c[2], w = q.c[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    out[0] = 1.0 - (tyy + tzz);
    out[1] = txy - twz;
    out[2] = txz + twy;
    out[4] = txy + twz;
    out[5] = 1.0 - (txx + tzz);
    out[6] = tyz - twx;
    out[8] = txz - twy;
    out[9] = tyz + twx;
    out[10] = 1.0 - (txx + tyy);
}

// std::lower_bound: the first index whose stamp is not below `stamp`, n when there is none
CCP_HD int64_t lower_bound(int64_t n, const uint64_t* stamps, uint64_t stamp)
{
    int64_t lo = 0, len = n;
    while (len > 0)
    {
        const int64_t half = len >> 1;
        if (stamps[lo + half] < stamp)
        {
            lo += half + 1;
            len -= half + 1;
        }
        else
            len = half;
    }
    return lo;
}

// n >= 1 samples with non-decreasing stamps. Equal neighbours never meet the division: lower_bound returns the first of them, whose
// predecessor is strictly earlier.
CCP_HD void interpolate(int64_t n, const uint64_t* stamps, const double* poses, uint64_t stamp, double out[12])
{
    const int64_t ia = lower_bound(n, stamps, stamp);
    if (ia == n || ia == 0)
    {
        const double* raw = poses + (ia == n ? n - 1 : 0) * 12;
        for (int i = 0; i < 12; i++)
            out[i] = raw[i];
        return;
    }
    const double* pb = poses + (ia - 1) * 12;
    const double* pa = poses + ia * 12;
    const double f = static_cast<double>(stamp - stamps[ia - 1]) / static_cast<double>(stamps[ia] - stamps[ia - 1]);
    const Quat q = quat_slerp(quat_from_rotation(pb), f, quat_from_rotation(pa));
    quat_to_rotation(q, out);
    for (int i = 0; i < 3; i++)
        out[i * 4 + 3] = (1 - f) * pb[i * 4 + 3] + f * pa[i * 4 + 3];
}

// stamp of firing c of an n-firing sweep (cc_kitti_firing_stamps_and_poses), n >= 2
CCP_HD uint64_t sweep_stamp(uint64_t start, uint64_t end, int c, int n)
{
    const double elapsed_ratio = static_cast<double>(c) / (n - 1);
    const double elapsed_time = static_cast<double>(end - start) * elapsed_ratio;
    return start + static_cast<uint64_t>(elapsed_time);
}

} // namespace ccp
