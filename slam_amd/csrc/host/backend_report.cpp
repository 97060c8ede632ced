// slam-backend: the lines a run prints about its result beyond the estimate (backend_report.h)
#include "backend_report.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../../include/slamhost.h"

using namespace slamhost;

void StepLedger::path_step(const float xt[3], const double est[3]) {
    if (keep_pose) {
        for (int q = 0; q < 3; q++) pose.push_back(xt[q]);
        pose.push_back(est[0]);
        pose.push_back(est[1]);
    }
    if (!keep_path) return;
    path.push_back(xt[0]);
    path.push_back(xt[1]);
    path.push_back(est[0]);
    path.push_back(est[1]);
}

// -map merged: the landmarks left after merging the slots that are alternatives for one landmark
static void print_merged_map(slamgpu_ctx *ctx, const Simulator &sim, const Options &o, const std::vector<double> &sum, int slots) {
    const int64_t ncand = slamhost_map_candidates(sum.data(), slots, o.merge_radius, nullptr, 0);
    if (ncand < 0 || ncand > INT32_MAX) {
        fprintf(stderr, "-map merged: %lld candidate pairs\n", (long long) ncand);
        return;
    }
    std::vector<int32_t> pairs(2 * (size_t) std::max<int64_t>(ncand, 1)), cluster((size_t) std::max(slots, 1));
    std::vector<double> joint((size_t) SLAMGPU_MAP_STRIDE * (size_t) std::max<int64_t>(ncand, 1)), merged((size_t) SLAMGPU_MAP_STRIDE * (size_t) std::max(slots, 1));
    slamhost_map_candidates(sum.data(), slots, o.merge_radius, pairs.data(), ncand);
    if (slamgpu_map_pairs(ctx, pairs.data(), (int32_t) ncand, joint.data(), nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    int32_t nmerged = 0;
    if (slamhost_map_merge(sum.data(), slots, pairs.data(), joint.data(), (int32_t) ncand, o.merge_radius, o.merge_cohold, cluster.data(), merged.data(),
                           &nmerged) != 0) {
        fprintf(stderr, "-map merged: slamhost_map_merge refused its arguments\n");
        return;
    }
    int confident = 0, covered = 0, stray = 0, multi = 0;
    std::vector<char> hit((size_t) sim.map.nlm, 0);
    std::vector<int> members((size_t) std::max(nmerged, 1), 0);
    for (int j = 0; j < slots; j++)
        if (cluster[(size_t) j] >= 0) members[(size_t) cluster[(size_t) j]]++;
    for (int q = 0; q < nmerged; q++) {
        multi += members[(size_t) q] > 1;
        const double *e = merged.data() + (size_t) SLAMGPU_MAP_STRIDE * (size_t) q;
        if (!(e[0] >= 0.5)) continue;
        confident++;
        bool near = false;
        for (int t = 0; t < sim.map.nlm; t++) {
            const double dx = e[1] - (double) sim.map.lm[(size_t) t], dy = e[2] - (double) sim.map.lm[(size_t) sim.map.nlm + t];
            if (dx * dx + dy * dy < 1.0) hit[(size_t) t] = 1, near = true;
        }
        if (!near) stray++;
    }
    for (char h : hit) covered += h;
    double top = 0.0;
    for (int64_t k = 0; k < ncand; k++) top = std::max(top, joint[(size_t) SLAMGPU_MAP_STRIDE * (size_t) k]);
    printf("merged map: %d landmarks held by at least half of the weight (%d of the %d true landmarks within 1 m of one of them, %d of them within 1 m of "
           "no true landmark); %d clusters of more than one slot; largest joint share of the %lld candidate pairs %.6f (radius %g m, cohold %g)\n",
           confident, covered, sim.map.nlm, stray, multi, (long long) ncand, top, o.merge_radius, o.merge_cohold);
}
// -map joint: the joint posterior of the pose and the confident slots (slamgpu_joint_summary)
static void print_joint(slamgpu_ctx *ctx, const Options &o, const std::vector<double> &sum, int slots) {
    std::vector<int32_t> list;
    for (int j = 0; j < slots && (int) list.size() < SLAMGPU_JOINT_MAX_SLOTS; j++)
        if (sum[(size_t) SLAMGPU_MAP_STRIDE * (size_t) j] >= 0.5) list.push_back(j);
    const int k = (int) list.size(), D = 3 + 2 * k;
    std::vector<double> out((size_t) SLAMGPU_JOINT_SIZE(k)), x((size_t) D), P((size_t) D * (size_t) D);
    int32_t both = 0;
    if (slamgpu_joint_summary(ctx, list.data(), k, out.data(), &both) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int32_t status = slamhost_joint_dense(out.data(), k, x.data(), P.data(), D);
    if (status < 0) {
        printf("joint posterior: not available, k %d, %d particles hold them all (joint share %.6f)\n", k, both, out[0]);
        return;
    }
    auto corr = [&](int a, int b) {
        const double d = P[(size_t) a * D + a] * P[(size_t) b * D + b];
        return d > 0.0 ? fabs(P[(size_t) a * D + b]) / sqrt(d) : 0.0;
    };
    double cpl = 0.0, cll = 0.0;
    for (int a = 3; a < D; a++) {
        for (int b = 0; b < 3; b++) cpl = std::max(cpl, corr(a, b));
        for (int b = 3; b < a; b++)
            if ((a - 3) / 2 != (b - 3) / 2) cll = std::max(cll, corr(a, b));
    }
    printf("joint posterior: k %d, D %d, joint share %.6f, %d particles hold them all; pose position sigma %.6f m; P is %s; largest |correlation| "
           "pose-landmark %.6f, landmark-landmark %.6f\n",
           k, D, out[0], both, sqrt(P[0] + P[(size_t) D + 1]), status == 0 ? "positive definite" : "NOT positive definite", cpl, cll);
    if (!o.joint_out.empty()) {
        FILE *f = fopen(o.joint_out.c_str(), "w");
        if (!f) {
            fprintf(stderr, "-JOINT_OUT %s: cannot write\n", o.joint_out.c_str());
            return;
        }
        fprintf(f, "%d\n", D);
        for (int a = 0; a < D; a++) fprintf(f, "%.17g%c", x[(size_t) a], a + 1 < D ? ' ' : '\n');
        for (int r = 0; r < D; r++)
            for (int c = 0; c < D; c++) fprintf(f, "%.17g%c", P[(size_t) r * D + c], c + 1 < D ? ' ' : '\n');
        fclose(f);
    }
}
// -map posterior: the slots as the whole particle set sees them (slamgpu_map_summary): confident = held by at least half of the weight;
// then -map merged's or -map joint's line
void print_posterior_map(slamgpu_ctx *ctx, const Simulator &sim, const Options &o) {
    if (!o.map_posterior) return;
    const int slots = slamgpu_num_landmarks(ctx);
    std::vector<double> sum((size_t) SLAMGPU_MAP_STRIDE * (size_t) std::max(slots, 1));
    if (slots < 0 || slamgpu_map_summary(ctx, 0, slots, sum.data(), nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    if (slots > 0 && sum[0] != sum[0]) {  // (every entry NaN: slamgpu_map_summary's answer to weights that sum to zero or to nothing finite)
        printf("posterior map: not available, the weights are degenerate (SLAMGPU_STATUS_DEGENERATE: their sum is zero or not finite)\n");
        if (o.map_joint) printf("joint posterior: not available, the weights are degenerate\n");
        return;
    }
    int confident = 0, covered = 0, stray = 0, minority = 0, dead = 0;
    std::vector<char> hit((size_t) sim.map.nlm, 0);
    for (int j = 0; j < slots; j++) {
        const double *e = sum.data() + (size_t) SLAMGPU_MAP_STRIDE * (size_t) j;
        if (e[0] >= 0.5) {
            confident++;
            bool near = false;
            for (int t = 0; t < sim.map.nlm; t++) {
                const double dx = e[1] - (double) sim.map.lm[(size_t) t], dy = e[2] - (double) sim.map.lm[(size_t) sim.map.nlm + t];
                if (dx * dx + dy * dy < 1.0) hit[(size_t) t] = 1, near = true;
            }
            if (!near) stray++;
        } else if (e[0] > 0.0) {
            minority++;
        } else {
            dead++;
        }
    }
    for (char h : hit) covered += h;
    printf("posterior map: %d slots held by at least half of the weight (%d of the %d true landmarks within 1 m of the mean of one of them, %d of them "
           "within 1 m of no true landmark); %d slots held by less than half, %d by none\n",
           confident, covered, sim.map.nlm, stray, minority, dead);
    if (o.map_merged) print_merged_map(ctx, sim, o, sum, slots);
    if (o.map_joint) print_joint(ctx, o, sum, slots);
}
// -pose posterior: the per-step pose posterior (slamgpu_pose_history_*)
void print_pose_posterior(slamgpu_ctx *ctx, const Options &o, const StepLedger &ledger) {
    if (!o.pose_records) return;
    int64_t first = 0, next = 0;
    if (slamgpu_pose_history_info(ctx, &first, &next, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int64_t n = next - first;
    if (n <= 0 || (size_t) next * 5 > ledger.pose.size()) {
        printf("pose posterior: no entries\n");
        return;
    }
    std::vector<double> sum((size_t) SLAMGPU_POSE_STRIDE * (size_t) n), nees((size_t) n), inv;
    std::vector<float> xt(3 * (size_t) n);
    if (slamgpu_pose_history_fetch(ctx, first, (int32_t) n, sum.data()) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    double dw = 0, df = 0;
    for (int64_t r = first; r < next; r++) {
        const double *e = sum.data() + (size_t) SLAMGPU_POSE_STRIDE * (size_t) (r - first), *t = ledger.pose.data() + 5 * (size_t) r;
        for (int q = 0; q < 3; q++) xt[3 * (size_t) (r - first) + q] = (float) t[q];
        dw += std::sqrt((e[1] - t[0]) * (e[1] - t[0]) + (e[2] - t[1]) * (e[2] - t[1]));
        df += std::sqrt((t[3] - t[0]) * (t[3] - t[0]) + (t[4] - t[1]) * (t[4] - t[1]));
        if (e[0] > 0.0) inv.push_back(1.0 / e[0]);
    }
    const int32_t bad = slamhost_pose_nees(sum.data(), (int32_t) n, xt.data(), nees.data(), nullptr);
    double tot = 0;
    int64_t ok = 0, in95 = 0;
    for (int64_t k = 0; k < n; k++)
        if (nees[(size_t) k] == nees[(size_t) k]) {
            tot += nees[(size_t) k];
            ok++;
            in95 += nees[(size_t) k] <= 7.8147;  // the 95 % point of chi^2 with 3 degrees of freedom
        }
    std::sort(inv.begin(), inv.end());
    const double med = inv.empty() ? std::nan("") : (inv.size() % 2 ? inv[inv.size() / 2] : 0.5 * (inv[inv.size() / 2 - 1] + inv[inv.size() / 2]));
    printf("pose posterior: %lld entries kept, mean distance to the true position %.4f m (filtered estimates of the same steps: %.4f m); mean NEES %.4f, "
           "NEES <= 7.8147 in %.4f of the steps (%d entries without a NEES); median effective sample size %.1f\n",
           (long long) n, dw / (double) n, df / (double) n, ok ? tot / (double) ok : std::nan(""), ok ? (double) in95 / (double) ok : std::nan(""), (int) bad, med);
}
// -innovation posterior: the innovation entries of every packet handed to slamgpu_update (slamgpu_innovation_*), -INNOVATION_RECORDS n
// entries kept
void print_innovation_posterior(slamgpu_ctx *ctx, const Options &o) {
    if (!o.innov_records) return;
    int64_t first = 0, next = 0;
    if (slamgpu_innovation_history_info(ctx, &first, &next, nullptr, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int64_t n = next - first;
    if (n <= 0) {
        printf("innovation posterior: no entries\n");
        return;
    }
    std::vector<double> ent((size_t) SLAMGPU_INNOV_STRIDE * (size_t) n), nis((size_t) n);
    if (slamgpu_innovation_history_fetch(ctx, first, (int32_t) n, ent.data(), nullptr, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int32_t bad = slamhost_innovation_nis(ent.data(), (int32_t) n, nis.data());
    double tot = 0, own = 0, share = 0;
    int64_t ok = 0, in95 = 0, nown = 0;
    for (int64_t k = 0; k < n; k++) {
        const double *e = ent.data() + (size_t) SLAMGPU_INNOV_STRIDE * (size_t) k;
        if (e[0] == e[0]) share += e[0];
        if (e[9] == e[9]) {
            own += e[9];
            nown++;
        }
        if (nis[(size_t) k] == nis[(size_t) k]) {
            tot += nis[(size_t) k];
            ok++;
            in95 += nis[(size_t) k] <= 5.9915;  // -2 ln 0.05: the 95 % point of chi^2 with 2 degrees of freedom
        }
    }
    printf("innovation posterior: %lld entries summarised, %lld retained; mean mixture NIS %.4f, NIS <= 5.9915 in %.4f of the entries; "
           "mean per-particle NIS %.4f; mean share %.4f; %d bad entries\n",
           (long long) next, (long long) n, ok ? tot / (double) ok : std::nan(""), ok ? (double) in95 / (double) ok : std::nan(""),
           nown ? own / (double) nown : std::nan(""), share / (double) n, (int) bad);
}
// -path smoothed: the recorded path posterior (slamgpu_path_*)
void print_smoothed_path(slamgpu_ctx *ctx, const Options &o, const StepLedger &ledger) {
    if (!o.path_records) return;
    int64_t first = 0, next = 0;
    if (slamgpu_path_info(ctx, &first, &next, nullptr) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    const int64_t n = next - first;
    if (n <= 0 || (size_t) next * 4 > ledger.path.size()) {
        printf("smoothed path: no records\n");
        return;
    }
    std::vector<double> sum((size_t) SLAMGPU_PATH_STRIDE * (size_t) n);
    std::vector<int32_t> distinct((size_t) n);
    if (slamgpu_path_summary(ctx, first, (int32_t) n, sum.data(), distinct.data()) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return;
    }
    if (sum[0] != sum[0]) {
        printf("smoothed path: not available, the weights are degenerate (SLAMGPU_STATUS_DEGENERATE: their sum is zero or not finite)\n");
        return;
    }
    double ds = 0, df = 0;
    for (int64_t r = first; r < next; r++) {
        const double *e = sum.data() + (size_t) SLAMGPU_PATH_STRIDE * (size_t) (r - first), *t = ledger.path.data() + 4 * (size_t) r;
        ds += std::sqrt((e[0] - t[0]) * (e[0] - t[0]) + (e[1] - t[1]) * (e[1] - t[1]));
        df += std::sqrt((t[2] - t[0]) * (t[2] - t[0]) + (t[3] - t[1]) * (t[3] - t[1]));
    }
    auto back = [&](int64_t k) -> std::string { return k < n ? std::to_string(distinct[(size_t) (n - 1 - k)]) : std::string("-"); };
    printf("smoothed path: %lld records kept, mean distance to the true path %.4f m (filtered estimates of the same steps: %.4f m); distinct ancestors "
           "1 / 10 / 100 records back %s / %s / %s, at the oldest record %d\n",
           (long long) n, ds / (double) n, df / (double) n, back(1).c_str(), back(10).c_str(), back(100).c_str(), (int) distinct[0]);
}

// -assoc particle: the map of the best (largest-weight) particle: what a FastSLAM with per-particle association reports
void print_particle_map(slamgpu_ctx *ctx, const Simulator &sim, const ParticleCounts &pp) {
    const int N = sim.conf.NPARTICLES;
    const int slots = slamgpu_num_landmarks(ctx);
    std::vector<float> w((size_t) N);
    int held = 0, covered = 0, best = 0;
    if (slots >= 0 && slamgpu_download_range(ctx, 0, N, nullptr, nullptr, w.data(), nullptr, nullptr) == 0) {
        for (int i = 1; i < N; i++)
            if (w[(size_t) i] > w[(size_t) best]) best = i;
        std::vector<float> xf(2 * (size_t) std::max(slots, 1));
        if (slots > 0 && slamgpu_download_range(ctx, best, 1, nullptr, nullptr, nullptr, xf.data(), nullptr) == 0) {
            std::vector<char> hit((size_t) sim.map.nlm, 0);
            for (int j = 0; j < slots; j++) {
                if (xf[2 * (size_t) j] != xf[2 * (size_t) j]) continue;  // absent
                held++;
                for (int t = 0; t < sim.map.nlm; t++) {
                    const float dx = xf[2 * (size_t) j] - sim.map.lm[(size_t) t], dy = xf[2 * (size_t) j + 1] - sim.map.lm[(size_t) sim.map.nlm + t];
                    if (dx * dx + dy * dy < 1.0f) hit[(size_t) t] = 1;
                }
            }
            for (char h : hit) covered += h;
        }
    }
    printf("landmarks in map: %d (the best particle's, number %d; %d of the %d true landmarks within 1 m of one of them; %d slots in use by all particles "
           "together, %ld opened, %ld of them dead slots reused, %ld observations dropped for want of a slot, at most %d slots rewritten in a step)\n",
           held, best, covered, sim.map.nlm, slots, pp.opened, pp.reused, pp.dropped, pp.most);
    int64_t st[3] = {0, 0, 0};
    if (slamgpu_particle_sample_stats(ctx, st) == 0 && st[0] > 0)
        printf("association sampling: %lld steps, %lld ambiguous (particle, observation) pairs, %lld drawn away from the nearest\n", (long long) st[0],
               (long long) st[1], (long long) st[2]);
    int64_t ms[3] = {0, 0, 0};
    if (slamgpu_particle_miss_stats(ctx, ms) == 0 && ms[0] > 0)
        printf("negative information: %lld steps, %lld held landmarks in view and unmatched (summed over particles and steps), %lld particles with one or more\n",
               (long long) ms[0], (long long) ms[1], (long long) ms[2]);
    int64_t mx[5] = {0, 0, 0, 0, 0};
    if (slamgpu_particle_mutex_stats(ctx, mx) == 0 && mx[0] > 0)
        printf("mutual exclusion: %lld steps, %lld contested (particle, landmark) pairs, %lld claims lost, %lld of them re-matched, %lld contests "
               "overturned (the keeper is not the first claimant)\n",
               (long long) mx[0], (long long) mx[1], (long long) mx[2], (long long) mx[3], (long long) mx[4]);
}

// -RUNS_MOMENTS: the figures of slam_amd.moments_summary, one line; D = 3 with the gates (the feature order is each member's own), the
// members' common dimension with the known association, where `order` says which landmark feature f is.  A member that ran out of
// capacity has parted from that order: the landmark bias is left out then
int print_ens_moments(slamgpu_ekf_ens *ens, const Simulator &sim, const Options &o, int D, const std::vector<int32_t> &order, int n_cap) {
    std::vector<double> mean((size_t) D), C((size_t) D * D), Pb((size_t) D * D);
    int32_t counted = 0, left_out = 0, pivot = -1;
    if (slamgpu_ens_moments(ens, D, 0, mean.data(), C.data(), Pb.data(), &counted, &left_out, &pivot) != 0) {
        fprintf(stderr, "slamgpu: %s\n", slamgpu_last_error());
        return EXIT_FAILURE;
    }
    auto at = [&](const std::vector<double> &M, int a, int b) { return M[(size_t) a * D + b]; };
    auto max_corr = [&](const std::vector<double> &M) {
        double m = D < 2 ? NAN : 0.0;
        for (int a = 0; a < D; a++)
            if (!(at(M, a, a) > 0.0)) return (double) NAN;
        for (int a = 0; a < D; a++)
            for (int b = 0; b < a; b++) m = std::max(m, std::fabs(at(M, a, b) / std::sqrt(at(M, a, a) * at(M, b, b))));
        return m;
    };
    const int nf = (D - 3) / 2;
    double fsum = 0.0, fmin = INFINITY, fmax = -INFINITY;
    for (int f = 0; f < nf; f++) {
        const int a = 3 + 2 * f;
        const double r = (at(C, a, a) + at(C, a + 1, a + 1)) / (at(Pb, a, a) + at(Pb, a + 1, a + 1));
        fsum += r;
        fmin = std::min(fmin, r);
        fmax = std::max(fmax, r);
    }
    const double two_pi = 6.283185307179586476925286766559;
    printf("ensemble moments: D %d, members counted %d, left out %d; tr C / tr Pbar position %.6f, heading %.6f, per feature mean %.6f smallest %.6f largest %.6f; "
           "largest |correlation| of C %.6f, of Pbar %.6f; bias of the mean: position %.6f m, heading %.6f rad",
           D, counted, left_out, (at(C, 0, 0) + at(C, 1, 1)) / (at(Pb, 0, 0) + at(Pb, 1, 1)), at(C, 2, 2) / at(Pb, 2, 2), nf ? fsum / nf : NAN, nf ? fmin : NAN,
           nf ? fmax : NAN, max_corr(C), max_corr(Pb), std::hypot(mean[0] - sim.xTrue[0], mean[1] - sim.xTrue[1]),
           std::remainder(mean[2] - (double) sim.xTrue[2], two_pi));
    if (D == 3) printf(", landmarks: not summarised (D = 3)\n");
    else if (n_cap > 0 || (int) order.size() < nf) printf(", landmarks: left out (%d members ran out of capacity)\n", n_cap);
    else {
        double dsum = 0.0;
        for (int f = 0; f < nf; f++) {
            const size_t id = (size_t) order[(size_t) f];
            dsum += std::hypot(mean[3 + 2 * (size_t) f] - sim.map.lm[id], mean[4 + 2 * (size_t) f] - sim.map.lm[(size_t) sim.map.nlm + id]);
        }
        printf(", mean landmark distance %.6f m\n", nf ? dsum / nf : NAN);
    }
    if (!o.runs_moments_out.empty()) {
        FILE *f = fopen(o.runs_moments_out.c_str(), "w");
        if (!f) {
            fprintf(stderr, "-RUNS_MOMENTS_OUT %s: cannot write\n", o.runs_moments_out.c_str());
            return EXIT_FAILURE;
        }
        fprintf(f, "%d\n", D);
        for (int a = 0; a < D; a++) fprintf(f, "%.17g%c", mean[(size_t) a], a + 1 < D ? ' ' : '\n');
        for (const std::vector<double> *M : {&C, &Pb})
            for (int r = 0; r < D; r++)
                for (int q = 0; q < D; q++) fprintf(f, "%.17g%c", at(*M, r, q), q + 1 < D ? ' ' : '\n');
        fclose(f);
    }
    return 0;
}
