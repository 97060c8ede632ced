// slamhost_pose_nees (include/slamhost.h): the normalised estimation error squared of the pose posterior that slamgpu_pose_summary /
// slamgpu_pose_history_fetch report, against the true pose: the consistency measure of Bailey, Nieto & Nebot, "Consistency of the
// FastSLAM algorithm", ICRA 2006.  Plain double arithmetic on a handful of numbers per entry; nothing here touches a GPU.
#include "slamhost.h"

#include <cmath>
#include <limits>

namespace {
constexpr int kStride = 18;  // SLAMGPU_POSE_STRIDE
constexpr double kTwoPi = 6.283185307179586476925286766559;
}  // namespace

extern "C" int32_t slamhost_pose_nees(const double *summary, int32_t count, const float *xtrue, double *nees, double *err) {
    if (count < 0 || (count > 0 && (!summary || !xtrue || !nees))) return -1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int32_t bad = 0;
    for (int32_t k = 0; k < count; k++) {
        const double *s = summary + (size_t) kStride * (size_t) k;
        const float *t = xtrue + 3 * (size_t) k;
        const double e[3] = {s[1] - (double) t[0], s[2] - (double) t[1], std::remainder(s[3] - (double) t[2], kTwoPi)};
        if (err)
            for (int q = 0; q < 3; q++) err[3 * (size_t) k + q] = e[q];
        // P = scatter + mean Pv, lower triangle: (xx, xy, yy, xu, yu, uu) + (p00, p10, p11, p20, p21, p22)
        const double p00 = s[6] + s[12], p10 = s[7] + s[13], p11 = s[8] + s[14], p20 = s[9] + s[15], p21 = s[10] + s[16], p22 = s[11] + s[17];
        // Cholesky P = L L^T; a pivot that is not positive (or not a number): P is not positive definite
        double v = nan;
        const double l00 = std::sqrt(p00);
        if (p00 > 0.0 && std::isfinite(l00)) {
            const double l10 = p10 / l00, l20 = p20 / l00, d1 = p11 - l10 * l10;
            if (d1 > 0.0 && std::isfinite(d1)) {
                const double l11 = std::sqrt(d1), l21 = (p21 - l20 * l10) / l11, d2 = p22 - l20 * l20 - l21 * l21;
                if (d2 > 0.0 && std::isfinite(d2)) {
                    const double l22 = std::sqrt(d2);
                    // y = L^-1 e, NEES = y . y
                    const double y0 = e[0] / l00, y1 = (e[1] - l10 * y0) / l11, y2 = (e[2] - l20 * y0 - l21 * y1) / l22;
                    v = y0 * y0 + y1 * y1 + y2 * y2;
                }
            }
        }
        if (!std::isfinite(v)) {
            v = nan;
            bad++;
        }
        nees[k] = v;
    }
    return bad;
}
