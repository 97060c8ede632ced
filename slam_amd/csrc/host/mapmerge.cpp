// slamhost_map_candidates / slamhost_map_merge (include/slamhost.h): from the posterior map's slot table (slamgpu_map_summary) and the
// joint shares of nearby slots (slamgpu_map_pairs) to a table of landmarks.  Plain host code, no GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#include "slamhost.h"

namespace {
constexpr int kStride = 9;  // SLAMGPU_MAP_STRIDE

inline bool in_use(const double *e) { return e[0] > 0.0 && std::isfinite(e[1]) && std::isfinite(e[2]); }

struct Cell {
    int64_t ix, iy;
    int32_t slot;
    bool operator<(const Cell &o) const { return ix != o.ix ? ix < o.ix : iy != o.iy ? iy < o.iy : slot < o.slot; }
};

int32_t find(std::vector<int32_t> &up, int32_t a) {
    while (up[a] != a) {
        up[a] = up[up[a]];
        a = up[a];
    }
    return a;
}
}  // namespace

extern "C" int64_t slamhost_map_candidates(const double *summary, int32_t slots, double radius, int32_t *pairs, int64_t max_pairs) {
    if (slots < 0 || (slots > 0 && !summary) || max_pairs < 0 || (max_pairs > 0 && !pairs)) return -1;
    if (!(radius > 0.0) || !std::isfinite(radius)) return 0;
    // a uniform grid of radius-sized cells over the means, kept as a sorted list of the occupied cells' members
    double x0 = INFINITY, y0 = INFINITY;
    for (int32_t j = 0; j < slots; j++) {
        const double *e = summary + (size_t) kStride * j;
        if (!in_use(e)) continue;
        x0 = std::min(x0, e[1]);
        y0 = std::min(y0, e[2]);
    }
    std::vector<Cell> cells;
    std::vector<int64_t> cx((size_t) slots), cy((size_t) slots);
    for (int32_t j = 0; j < slots; j++) {
        const double *e = summary + (size_t) kStride * j;
        if (!in_use(e)) continue;
        const double fx = std::floor((e[1] - x0) / radius), fy = std::floor((e[2] - y0) / radius);
        if (!(fx < 9.0e18) || !(fy < 9.0e18)) continue;  // (a mean 10^18 radii away has no neighbour a double could tell from it)
        cx[j] = (int64_t) fx;
        cy[j] = (int64_t) fy;
        cells.push_back(Cell{cx[j], cy[j], j});
    }
    std::sort(cells.begin(), cells.end());
    const double r2 = radius * radius;
    int64_t n = 0;
    std::vector<int32_t> near;
    std::vector<char> listed((size_t) slots, 0);
    for (const Cell &c : cells) listed[c.slot] = 1;
    for (int32_t a = 0; a < slots; a++) {
        if (!listed[a]) continue;
        const double *ea = summary + (size_t) kStride * a;
        near.clear();
        for (int64_t ix = cx[a] - 1; ix <= cx[a] + 1; ix++) {
            // the three cells of this column are one stretch of the sorted list
            auto it = std::lower_bound(cells.begin(), cells.end(), Cell{ix, cy[a] - 1, -1});
            for (; it != cells.end() && it->ix == ix && it->iy <= cy[a] + 1; ++it) {
                const int32_t b = it->slot;
                if (b <= a) continue;
                const double *eb = summary + (size_t) kStride * b;
                const double dx = ea[1] - eb[1], dy = ea[2] - eb[2];
                if (dx * dx + dy * dy < r2) near.push_back(b);
            }
        }
        std::sort(near.begin(), near.end());
        for (int32_t b : near) {
            if (n < max_pairs) {
                pairs[2 * n] = a;
                pairs[2 * n + 1] = b;
            }
            n++;
        }
    }
    return n;
}

extern "C" int slamhost_map_merge(const double *summary, int32_t slots, const int32_t *pairs, const double *joint, int32_t npairs, double radius,
                                  double cohold, int32_t *cluster, double *merged, int32_t *nmerged) {
    if (slots < 0 || npairs < 0 || (slots > 0 && (!summary || !cluster || !merged)) || (npairs > 0 && (!pairs || !joint)) || !nmerged) return -1;
    for (int64_t k = 0; k < 2 * (int64_t) npairs; k++)
        if (pairs[k] < 0 || pairs[k] >= slots) return -1;
    std::vector<int32_t> up((size_t) slots);
    std::iota(up.begin(), up.end(), 0);
    const double r2 = radius * radius;
    for (int32_t k = 0; k < npairs; k++) {
        const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a == b) continue;
        const double *ea = summary + (size_t) kStride * a, *eb = summary + (size_t) kStride * b;
        if (!(ea[0] > 0.0) || !(eb[0] > 0.0)) continue;
        const double dx = ea[1] - eb[1], dy = ea[2] - eb[2];
        if (!(radius > 0.0) || !(dx * dx + dy * dy < r2)) continue;
        if (!(joint[(size_t) kStride * k] <= cohold * std::min(ea[0], eb[0]))) continue;  // (held together too often, or NaN: two landmarks)
        const int32_t ra = find(up, a), rb = find(up, b);
        if (ra != rb) up[std::max(ra, rb)] = std::min(ra, rb);  // (the root is the cluster's lowest slot)
    }
    // clusters numbered in ascending order of their lowest slot
    std::vector<int32_t> id((size_t) slots, -1);
    int32_t n = 0;
    for (int32_t j = 0; j < slots; j++) {
        const double *e = summary + (size_t) kStride * j;
        if (!(e[0] > 0.0)) {
            cluster[j] = -1;
            continue;
        }
        const int32_t r = find(up, j);
        if (r == j) id[j] = n++;
        cluster[j] = id[r];  // (r <= j: numbered already)
    }
    std::vector<int32_t> size((size_t) n, 0);
    for (int32_t j = 0; j < slots; j++)
        if (cluster[j] >= 0) size[cluster[j]]++;
    // singletons: the slot's nine numbers as they are; the others: sums over the members in ascending slot order
    std::vector<double> S((size_t) n, 0.0), top((size_t) n, 0.0);
    for (int32_t j = 0; j < slots; j++) {
        const int32_t c = cluster[j];
        if (c < 0) continue;
        const double *e = summary + (size_t) kStride * j;
        double *m = merged + (size_t) kStride * c;
        if (size[c] == 1) {
            std::copy(e, e + kStride, m);
            continue;
        }
        if (S[c] == 0.0) std::fill(m, m + kStride, 0.0);
        S[c] += e[0];
        top[c] = std::max(top[c], e[0]);
        m[1] += e[0] * e[1];
        m[2] += e[0] * e[2];
    }
    for (int32_t c = 0; c < n; c++)
        if (size[c] > 1) {
            merged[(size_t) kStride * c + 1] /= S[c];
            merged[(size_t) kStride * c + 2] /= S[c];
        }
    for (int32_t j = 0; j < slots; j++) {
        const int32_t c = cluster[j];
        if (c < 0 || size[c] == 1) continue;
        const double *e = summary + (size_t) kStride * j;
        double *m = merged + (size_t) kStride * c;
        const double dx = e[1] - m[1], dy = e[2] - m[2];
        m[3] += e[0] * (e[3] + dx * dx);
        m[4] += e[0] * (e[4] + dx * dy);
        m[5] += e[0] * (e[5] + dy * dy);
        m[6] += e[0] * e[6];
        m[7] += e[0] * e[7];
        m[8] += e[0] * e[8];
    }
    // share: sum of the members' shares less the joint shares of the given pairs inside the cluster (each unordered pair once)
    std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>> inside;
    for (int32_t k = 0; k < npairs; k++) {
        const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a == b || cluster[a] < 0 || cluster[a] != cluster[b] || size[cluster[a]] == 1) continue;
        inside.push_back({{std::min(a, b), std::max(a, b)}, k});
    }
    std::sort(inside.begin(), inside.end());
    std::vector<double> J((size_t) n, 0.0);
    for (size_t q = 0; q < inside.size(); q++) {
        if (q > 0 && inside[q].first == inside[q - 1].first) continue;
        const double s = joint[(size_t) kStride * inside[q].second];
        if (s > 0.0) J[cluster[inside[q].first.first]] += s;
    }
    for (int32_t c = 0; c < n; c++) {
        if (size[c] == 1) continue;
        double *m = merged + (size_t) kStride * c;
        m[0] = std::min(1.0, std::max(top[c], S[c] - J[c]));
        for (int q = 3; q < kStride; q++) m[q] /= S[c];
    }
    *nmerged = n;
    return 0;
}
