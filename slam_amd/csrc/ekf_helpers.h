// What the device EKF (ekf.cpp) and the EKF ensemble (ekf_ens.cpp) evaluate alike: the angle wrap, the observation model and the
// 2x2 inverse of the gates, operation by operation as the host's.  Private to the including unit.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ inline float ekf_trig_offset(float ang) {  // core.cpp:460-477
    const double pi = 3.14159265358979323846;
    if (((double) ang < -2 * pi) || ((double) ang > 2 * pi)) {
        const int n = (int) floor((double) ang / (2 * pi));
        ang = (float) ((double) ang - n * (2 * pi));
    }
    if ((double) ang > pi) ang = (float) ((double) ang - (2 * pi));
    if ((double) ang < -pi) ang = (float) ((double) ang + (2 * pi));
    return ang;
}

// EkfSlam::observe_model: H restricted to its five non-zero columns {0, 1, 2, fpos, fpos + 1}
__device__ inline void ekf_observe_model(const float *__restrict__ x, int idf, bool want_zp, float zp[2], float H5[10]) {
#pragma clang fp contract(off)
    const int fpos = 3 + idf * 2;
    const float dx = x[fpos] - x[0], dy = x[fpos + 1] - x[1];
    const float d2 = dx * dx + dy * dy;
    const float d = sqrtf(d2);
    const float xd = dx / d, yd = dy / d, xd2 = dx / d2, yd2 = dy / d2;
    zp[0] = d;
    zp[1] = want_zp ? atan2f(dy, dx) - x[2] : 0.0f;
    H5[0] = -xd; H5[1] = -yd; H5[2] = 0; H5[3] = xd; H5[4] = yd;
    H5[5] = yd2; H5[6] = -xd2; H5[7] = -1; H5[8] = -yd2; H5[9] = xd2;
}

// 2x2 inverse / determinant through partial-pivot LU, as the host's inverse2
__device__ inline void ekf_inverse2(const float S[4], float X[4], float *det) {
#pragma clang fp contract(off)
    const bool swap = fabsf(S[2]) > fabsf(S[0]);
    const float u00 = swap ? S[2] : S[0], u01 = swap ? S[3] : S[1];
    float l10 = swap ? S[0] : S[2];
    const float r11 = swap ? S[1] : S[3];
    if (u00 != 0.0f) l10 = l10 * (1.0f / u00);
    const float u11 = r11 - l10 * u01;
    float b00 = swap ? 0.0f : 1.0f, b01 = swap ? 1.0f : 0.0f, b10 = swap ? 1.0f : 0.0f, b11 = swap ? 0.0f : 1.0f;
    b10 -= b00 * l10;
    b11 -= b01 * l10;
    float a = 1.0f / u11;
    b10 *= a;
    b11 *= a;
    b00 -= b10 * u01;
    b01 -= b11 * u01;
    a = 1.0f / u00;
    X[0] = b00 * a;
    X[1] = b01 * a;
    X[2] = b10;
    X[3] = b11;
    *det = (swap ? -1.0f : 1.0f) * (u00 * u11);
}

}  // namespace
