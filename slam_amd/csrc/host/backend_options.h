// slam-backend's own options: everything the driver decides from its arguments, in one struct that is filled once and read everywhere
// else as const &.  Their meaning: usage() (slam-backend -h) and INTEGRATION.md.
#pragma once
#include <cstdint>
#include <string>

#include "../../../include/slamgpu.h"
#include "frontend.h"
#include "gated.h"

struct Options {
    // what the run is
    long maxsteps = -1;  // -maxsteps n: stop after n control steps (< 0: the whole path)
    bool parity = false, strict_math = false;                                        // -rng parity, -math strict
    bool gated = false, particle = false;                                            // -assoc gated | particle
    bool observe_dev = false, particle_dev = false, loop_step = false, batched = false;  // -observe device, with -assoc particle, -loop step; run_batched
    bool distributed = false;  // -gpus k, k != 1, with a FastSLAM method
    int gpus = 1;
    bool gpubusy = false, log_weights = false;
    std::string log, plot = "none", assoclog;
    bool plots = false;  // -plot names a sink
    int stride = 1;      // -plotstride k
    // -assoc particle
    slamgpu_particle_assoc popt{};
    bool particle_assoc_word = true;  // -PARTICLE_ASSOC is lists, auto or absent
    int particle_slots = 4;
    double excl_spacing = 0.0;
    std::string assoc_sample, mutex;  // -PARTICLE_ASSOC_SAMPLE, -PARTICLE_MUTEX as given
    bool miss = false;
    double miss_p = 1.0, miss_m = 0.0;
    slamhost::GatedPolicy policy;  // -assoc gated: the -ASSOC_* numbers
    // the reports at the end of a FastSLAM run
    bool map_posterior = false, map_merged = false, map_joint = false;  // -map posterior | merged | joint (each of the last two sets the first)
    std::string joint_out;
    double merge_radius = 1.0, merge_cohold = 0.1;
    int path_records = 0, pose_records = 0, innov_records = 0;  // -path smoothed, -pose posterior, -innovation posterior: the entries kept; 0: off
    // the device EKF
    bool ekf_device = false;
    double ekf_local = 0.0;  // -EKF_LOCAL margin; 0: off
    int ekf_local_new = 64;
    int ekf_prune_age = 0, ekf_prune_hits = 0;  // -EKF_PRUNE_AGE a -EKF_PRUNE_HITS h (host filter too); 0: off
    int runs = 0;  // -runs B; 0: one filter
    uint64_t runs_seed = 0;
    int runs_batch = 0;  // -RUNS_BATCH K; 0: by B (run_ekf_ensemble)
    std::string runs_trace, runs_moments_out;
    bool runs_moments = false;
};

void usage(const char *a0);
// one refusal line on stderr: "<option>: <why>", or <option> alone; false
bool refuse(const std::string &option, const char *why = nullptr);
// Everything that is decided from the arguments alone.  Takes the driver's own report options out of sim.conf.kv, so that they stay out
// of the settings listing.  Writes nothing but the refusal line of the first rule broken; false then
bool parse_options(slamhost::Simulator &sim, Options &o);
// the refusals whose place in the output is after the settings listing and the plot's opening
bool refuse_after_listing(const slamhost::Conf &c, const Options &o);
