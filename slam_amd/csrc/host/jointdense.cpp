// slamhost_joint_dense (include/slamhost.h): the state and the dense total covariance, in the EKF's ordering, of one
// slamgpu_joint_summary: P = scatter + blockdiag(mean Pv, mean Pf_0, ...), and whether a Cholesky factorisation in double finds it
// positive definite.  Plain double arithmetic on at most 255 x 255 numbers; nothing here touches a GPU.
#include "slamhost.h"

#include <cmath>
#include <limits>
#include <vector>

namespace {
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr int kMaxSlots = 126;  // SLAMGPU_JOINT_MAX_SLOTS
}  // namespace

extern "C" int32_t slamhost_joint_dense(const double *joint, int32_t k, double *x, double *P, int32_t ld) {
    if (!joint || !x || !P || k < 0 || k > kMaxSlots || ld < 3 + 2 * k) return -1;
    const int D = 3 + 2 * k, T = D * (D + 1) / 2;
    const double *mu = joint + 1, *C = joint + 1 + D, *pv = C + T, *pf = pv + 6;
    bool bad = !(joint[0] == joint[0]);
    for (int a = 0; a < D; a++) {
        x[a] = mu[a];
        bad |= !(mu[a] == mu[a]);
    }
    if (x[2] == x[2]) {  // the heading into (-pi, pi]
        double th = std::remainder(x[2], kTwoPi);
        if (th <= -kTwoPi / 2) th += kTwoPi;
        x[2] = th;
    }
    for (int r = 0; r < D; r++)
        for (int c = 0; c <= r; c++) {
            const double v = C[r * (r + 1) / 2 + c];
            P[(size_t) r * ld + c] = v;
            P[(size_t) c * ld + r] = v;
        }
    // the within-particle blocks: Pv (p00, p10, p11, p20, p21, p22), then Pf (p00, p10, p11) per listed slot
    static const int pr[6] = {0, 1, 1, 2, 2, 2}, pc[6] = {0, 0, 1, 0, 1, 2};
    for (int q = 0; q < 6; q++) {
        P[(size_t) pr[q] * ld + pc[q]] += pv[q];
        if (pr[q] != pc[q]) P[(size_t) pc[q] * ld + pr[q]] += pv[q];
    }
    for (int s = 0; s < k; s++) {
        const int a = 3 + 2 * s;
        const double *f = pf + 3 * s;
        P[(size_t) a * ld + a] += f[0];
        P[(size_t) (a + 1) * ld + a] += f[1];
        P[(size_t) a * ld + a + 1] += f[1];
        P[(size_t) (a + 1) * ld + a + 1] += f[2];
    }
    for (int r = 0; r < D; r++)
        for (int c = 0; c < D; c++) bad |= !(P[(size_t) r * ld + c] == P[(size_t) r * ld + c]);
    if (bad) return -1;
    // Cholesky P = L L^T, row by row; a pivot that is not positive and finite: P is not positive definite
    std::vector<double> L((size_t) D * D, 0.0);
    for (int r = 0; r < D; r++) {
        for (int c = 0; c <= r; c++) {
            double s = P[(size_t) r * ld + c];
            for (int q = 0; q < c; q++) s -= L[(size_t) r * D + q] * L[(size_t) c * D + q];
            if (c == r) {
                if (!(s > 0.0) || !std::isfinite(s)) return 1;
                L[(size_t) r * D + r] = std::sqrt(s);
            } else {
                L[(size_t) r * D + c] = s / L[(size_t) c * D + c];
            }
        }
    }
    return 0;
}
