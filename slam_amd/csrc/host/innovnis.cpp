// slamhost_innovation_nis (include/slamhost.h): the normalised innovation squared of the filter's predicted-measurement MIXTURE, from
// the entries slamgpu_innovation_summary / slamgpu_innovation_history_fetch report: Bar-Shalom's innovation test, with the covariance
// a particle filter has to assemble (between-particle scatter + mean within-particle S; Bailey, Nieto & Nebot, ICRA 2006, for why a
// particle's own S is not enough).  Plain double arithmetic on ten numbers per entry; nothing here touches a GPU.
#include "slamhost.h"

#include <cmath>
#include <limits>

namespace {
constexpr int kStride = 10;  // SLAMGPU_INNOV_STRIDE
}  // namespace

extern "C" int32_t slamhost_innovation_nis(const double *entries, int32_t count, double *nis) {
    if (count < 0 || (count > 0 && (!entries || !nis))) return -1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int32_t bad = 0;
    for (int32_t k = 0; k < count; k++) {
        const double *s = entries + (size_t) kStride * (size_t) k;
        double v = nan;
        bool ok = s[0] > 0.0;  // (a share of 0, or NaN: nobody holds the slot, or degenerate weights)
        for (int q = 0; q < kStride; q++) ok = ok && !std::isnan(s[q]);
        if (ok) {
            // P = scatter + mean S, lower triangle: (rr, rb, bb) + (s00, s10, s11)
            const double e0 = s[1], e1 = s[2], p00 = s[3] + s[6], p10 = s[4] + s[7], p11 = s[5] + s[8];
            // Cholesky P = L L^T; a pivot that is not positive (or not a number): P is not positive definite
            const double l00 = std::sqrt(p00);
            if (p00 > 0.0 && std::isfinite(l00)) {
                const double l10 = p10 / l00, d1 = p11 - l10 * l10;
                if (d1 > 0.0 && std::isfinite(d1)) {
                    const double l11 = std::sqrt(d1);
                    // y = L^-1 e, NIS = y . y
                    const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / l11;
                    v = y0 * y0 + y1 * y1;
                }
            }
        }
        if (!std::isfinite(v)) {
            v = nan;
            bad++;
        }
        nis[k] = v;
    }
    return bad;
}
