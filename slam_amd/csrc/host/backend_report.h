// slam-backend: the lines a run prints about its result beyond the estimate, and the bookkeeping they read (backend_report.cpp)
#pragma once
#include <cstdint>
#include <vector>

#include "backend_options.h"

// -path smoothed / -pose posterior: record r of the device's history belongs to observation step r of the run.  The loop that makes the
// steps owns the ledger and notes every step's truth and filtered estimate in it; the reports set the posterior against them
struct StepLedger {
    explicit StepLedger(const Options &o) : keep_path(o.path_records != 0), keep_pose(o.pose_records != 0) {}
    void path_step(const float xt[3], const double est[3]);
    std::vector<double> path;  // per step: true x, y, estimated x, y
    std::vector<double> pose;  // per step: true x, y, theta, estimated x, y
   private:
    bool keep_path, keep_pose;
};

// -assoc particle: the slot counters of the steps' reports (slamgpu_update_particle, slamgpu_particle_report_fetch)
struct ParticleCounts {
    long opened = 0, reused = 0, dropped = 0;
    int most = 0;
    void add(const int32_t rep[8]) {
        opened += rep[1];
        reused += rep[2];
        dropped += rep[3];
        if (rep[0] > most) most = rep[0];
    }
};

void print_particle_map(slamgpu_ctx *ctx, const slamhost::Simulator &sim, const ParticleCounts &pp);
void print_posterior_map(slamgpu_ctx *ctx, const slamhost::Simulator &sim, const Options &o);  // -map posterior | merged | joint
void print_smoothed_path(slamgpu_ctx *ctx, const Options &o, const StepLedger &ledger);
void print_pose_posterior(slamgpu_ctx *ctx, const Options &o, const StepLedger &ledger);
void print_innovation_posterior(slamgpu_ctx *ctx, const Options &o);
int print_ens_moments(slamgpu_ekf_ens *ens, const slamhost::Simulator &sim, const Options &o, int D, const std::vector<int32_t> &order, int n_cap);
