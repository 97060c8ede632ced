/* slamhost — C ABI of the host-side front end that surrounds the hot path in matzipan/slam's wrappers
 * (libslamhost.so, plain C++, no GPU code).  It is what slam-backend links and what bench.py / the
 * tests use to produce the control / observation tape.  Citations are file:line under the reference.
 *
 *  - Conf::parse keys + defaults (src/backend/core.cpp:971-1073), `<map stem>.ini` then `-KEY value`
 *    overrides (SLAMBackendApplication.cpp:59-89, utils.cpp:504-565,1032-1046)
 *  - map reader (core.cpp:855-962)
 *  - SLAMWrapper::control(): updateSteering, predictTruePosition, addControlNoise
 *    (wrappers/slamwrapper.cpp:174-238, core.cpp:24-78)
 *  - getObservations / addObservationNoise / dataAssociationKnown (core.cpp:91-120,185-273,438-449)
 *  - the libc rand() draws of nRandMat::randn and stratifiedRandom in the reference's order
 *    (core.cpp:383-419,751-769), used to feed slamgpu's TAPE mode.
 */
#ifndef SLAMHOST_H
#define SLAMHOST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct slamhost_sim slamhost_sim;

typedef struct {
    float V, MAXG, RATEG, WHEELBASE, DT_CONTROLS, sigmaV, sigmaG, MAX_RANGE, DT_OBSERVE, sigmaR, sigmaB, sigmaT;
    float GATE_REJECT, GATE_AUGMENT, AT_WAYPOINT;
    int32_t NUMBER_LOOPS, NPARTICLES, NEFFECTIVE;
    int32_t SWITCH_CONTROL_NOISE, SWITCH_SENSOR_NOISE, SWITCH_INFLATE_NOISE, SWITCH_PREDICT_NOISE,
        SWITCH_SAMPLE_PROPOSAL, SWITCH_HEADING_KNOWN, SWITCH_RESAMPLE, SWITCH_PROFILE, SWITCH_SEED_RANDOM,
        SWITCH_ASSOCIATION_KNOWN, SWITCH_BATCH_UPDATE, SWITCH_USE_IEKF;
    int32_t method;      /* 0 EKF1, 1 FASTSLAM1, 2 FASTSLAM2 (anything else => EKF, SLAMBackendApplication.cpp:26-29) */
    int32_t n_landmarks; /* columns of lm */
    int32_t n_waypoints;
    float Q[4], R[4], Qe[4], Re[4]; /* slamwrapper.cpp:25-37 */
} slamhost_conf;

const char *slamhost_last_error(void);
/* argv as given to slam-backend: -m map.mat -method M [-KEY value]... ; seeds libc rand() (slamwrapper.cpp:48-52) */
slamhost_sim *slamhost_sim_create(int argc, char **argv);
void slamhost_sim_destroy(slamhost_sim *s);
int slamhost_sim_conf(const slamhost_sim *s, slamhost_conf *out);
/* landmarks / waypoints, 2 x n row-major */
int slamhost_sim_map(const slamhost_sim *s, float *lm, float *wp);
/* control(): -1 = run finished, 0 = step without observation, 1 = observation due.  Outputs the noisy
 * controls handed to predict and the true heading. */
int slamhost_sim_control(slamhost_sim *s, float *Vn, float *Gn, float *phi_true);
/* getObservations + noise + dataAssociationKnown against nf_known landmarks already in the map.
 * zf/zn sized 2*n_landmarks, idf n_landmarks.  Returns 0. */
int slamhost_sim_observe(slamhost_sim *s, int32_t nf_known, float *zf, int32_t *idf, int32_t *m, float *zn, int32_t *n);
/* raw observation of the last slamhost_sim_observe: z[2*nz], visible ids */
int slamhost_sim_last_z(const slamhost_sim *s, float *z, int32_t *vis, int32_t *nz);
void slamhost_sim_true(const slamhost_sim *s, float x[3]);
/* the TRUE controls of the last slamhost_sim_control, the ones that moved the true pose (what slamgpu_ens_sim_noise perturbs itself) */
void slamhost_sim_true_controls(const slamhost_sim *s, float *V, float *G);
int64_t slamhost_sim_control_steps(const slamhost_sim *s);

/* EKF-SLAM on the host CPU (-method EKF1; BASELINE config 1): EKFSLAMWrapper::run's loop body
 * (wrappers/ekfslamwrapper.cpp:50-84) = control(), observation when due, EKFSLAM::sim (algorithms/ekfslam.cpp:17-43). */
typedef struct slamhost_ekf slamhost_ekf;
slamhost_ekf *slamhost_ekf_create(const slamhost_sim *s);
void slamhost_ekf_destroy(slamhost_ekf *e);
int slamhost_ekf_step(slamhost_ekf *e, slamhost_sim *s); /* -1 finished, 0 control step, 1 with observation */
int slamhost_ekf_state(const slamhost_ekf *e, float *x, float *P, int32_t cap); /* returns dim; P row-major, ld = cap */
/* The same filter with explicit inputs, so that a device filter (slamgpu.h: the slamgpu_ekf entry points) can be fed exactly what a
 * host run was fed.  last_inputs: the noisy controls V, G, the heading observation phi and whether slamhost_sim_last_z was observed, as
 * the last slamhost_ekf_step handed them to EKFSLAM::sim; slamhost_sim_noise: the simulator's Q, R, Qe, Re (slamwrapper.cpp:25-37) and
 * its control period, any pointer may be NULL.  sim: one EKFSLAM::sim on these inputs (ids: the visible landmark ids, read with
 * SWITCH_ASSOCIATION_KNOWN only); fed last_inputs and last_z it reproduces slamhost_ekf_step bit for bit.  upload: x[dim] and P
 * (row-major, leading dimension ld) replace the state; the id table of the known association starts over with id f = feature f
 * for the uploaded features.  0, or -1 for bad arguments. */
int slamhost_ekf_last_inputs(const slamhost_ekf *e, float vgphi[3], int32_t *observe);
int slamhost_sim_noise(const slamhost_sim *s, float Q[4], float R[4], float Qe[4], float Re[4], float *dt);
int slamhost_ekf_sim(slamhost_ekf *e, float V, float G, const float Q[4], float dt, float phi, const float *z, const int32_t *ids, int32_t nz,
                     const float Re[4], const float R[4], int32_t observe);
int slamhost_ekf_upload(slamhost_ekf *e, int32_t dim, const float *x, const float *P, int32_t ld);
/* The twins of slamgpu_ekf_remove and slamgpu_ekf_feature_stats (slamgpu.h has the index map and the counters' rules) on the host
 * filter.  remove: features[k] ascending and distinct in [0, nf); x and P become the gather over the surviving indices -- P from its
 * LOWER triangle, mirrored, wherever an index at or beyond the first removed entry is involved, the rest as it was -- the id table
 * forgets the removed features' ids and renumbers the others, the counters are compacted; 0, or -1 for bad arguments with nothing
 * applied.  feature_stats: any output may be NULL, arrays [nf]; returns nf.  The host filter has no direct update: its epoch counts
 * the sim / step calls with an observation. */
int slamhost_ekf_remove(slamhost_ekf *e, const int32_t *features, int32_t k);
int slamhost_ekf_feature_stats(const slamhost_ekf *e, int32_t *hits, int32_t *born, int32_t *last, int32_t *epoch);
/* The region of a local period of the device filter (slamgpu.h: slamgpu_ekf_local_begin): the features of the EKF-SLAM state x[dim]
 * (dim = 3 + 2 nf) whose estimate lies within `radius` of the pose estimate (x[0], x[1]) -- dx dx + dy dy <= radius radius in float32,
 * the boundary included -- ascending into features_out[max_count].  Returns their number, -1 if there are more than max_count
 * (features_out then holds the first max_count), -2 for bad arguments.  Pure host code. */
int slamhost_ekf_local_region(const float *x, int32_t dim, float radius, int32_t *features_out, int32_t max_count);

/* libc rand() tape in the reference's draw order */
/* The policy that turns the vote of the gated per-particle association (slamgpu_associate: labels by EKFSLAM::dataAssociate,
 * ekfslam.cpp:151-189, per particle) into ONE association per step, as slam-backend -assoc gated applies it (slam_amd/csrc/host/
 * gated.h: supermajority to open, the second stage in world coordinates, landmark credits).  set: tunables by name -- "enabled",
 * "new_share", "match_share", "credit_start", "credit_max", "retire_below", "rescue", "rescue_base", "rescue_per_m",
 * "unique_ratio", "new_factor" (returns -1 for an unknown name).  step: z[2 nz], consensus / support of slamgpu_associate, the
 * pose xv[3] and landmark means xf[2 nf] of ONE particle (slamgpu_peek), MAX_RANGE, room = landmarks that may still be opened;
 * out (sized for nz / nz / nf): the packet of slamgpu_update and the landmarks to hand to slamgpu_retire_landmarks.
 * counts[6]: opened, retired, matched by the second stage, observations left unused, refused as new, landmarks in use. */
typedef struct slamhost_gated slamhost_gated;
slamhost_gated *slamhost_gated_create(void);
void slamhost_gated_destroy(slamhost_gated *g);
int slamhost_gated_set(slamhost_gated *g, const char *name, double value);
int slamhost_gated_step(slamhost_gated *g, const float *z, int32_t nz, const int32_t *consensus, const float *support, const float xv[3],
                        const float *xf, int32_t nf, float max_range, int32_t room, float *zf, int32_t *idf, int32_t *m, float *zn, int32_t *n,
                        int32_t *retire, int32_t *n_retire);
void slamhost_gated_counts(const slamhost_gated *g, int32_t counts[6]);

/* From the slot table of the posterior map to a table of LANDMARKS.  A run with the association unknown opens a second slot beside a
 * mapped landmark whenever a particle off its true pose calls an observation of it new; the marginal shares of slamgpu_map_summary
 * cannot tell such ALTERNATIVES (no particle holds both) from two NEIGHBOURING landmarks (most holders of one hold the other).  The
 * joint share of slamgpu_map_pairs can.  Both functions are pure: no GPU, no state.
 *
 * summary[slots][9] is slamgpu_map_summary's output (share | mean x, y | scatter xx, xy, yy | mean Pf 00, 10, 11), joint[npairs][9]
 * slamgpu_map_pairs' for pairs[npairs][2] (only its share, joint[k][0], is read).
 *
 * candidates: every a < b with both shares > 0 and the means closer than `radius`, in ascending order (a, then b), found through a
 * uniform grid over the means.  Returns their number; the first max_pairs of them are written (pairs may be NULL with max_pairs 0:
 * count, allocate, call again).  -1: bad arguments.
 *
 * merge: an edge joins a and b when both shares are > 0, |mu_a - mu_b| < radius and s_ab <= cohold * min(s_a, s_b) -- near each other and
 * (almost) never held together.  Clusters are the connected components (single linkage), numbered in ascending order of their lowest
 * slot; cluster[j] is slot j's, -1 for a slot of share 0.  merged[c][9], in the summary's layout, with S = sum of the members' shares:
 *     share      sum_C s_j - sum of s_jk over the given pairs inside C (an unordered pair given twice counts once), clamped to
 *                [max_C s_j, 1]: the second-order inclusion-exclusion (Bonferroni) lower bound of the weight that holds at least one
 *                member.  It is exact for clusters of two and whenever no particle holds three members; pairs inside C that the
 *                caller did not give count as never held together.
 *     mean       sum s_j mu_j / S
 *     [3..5]     sum s_j (scatter_j + (mu_j - mean)(mu_j - mean)^T) / S
 *     [6..8]     sum s_j Pf_j / S
 * A cluster of one slot reproduces the slot's nine numbers bit for bit.  *nmerged = the number of clusters.  radius and cohold are the
 * caller's; slam-backend's defaults are 1.0 m and 0.1, and no accuracy claim rests on the 0.1 yet.  Returns 0; -1: bad arguments (a
 * pair outside [0, slots), a NULL array that is needed). */
int64_t slamhost_map_candidates(const double *summary, int32_t slots, double radius, int32_t *pairs, int64_t max_pairs);
int slamhost_map_merge(const double *summary, int32_t slots, const int32_t *pairs, const double *joint, int32_t npairs, double radius,
                       double cohold, int32_t *cluster /*[slots]*/, double *merged /*[slots][9]*/, int32_t *nmerged);

/* The consistency of the pose posterior (Bailey, Nieto & Nebot, "Consistency of the FastSLAM algorithm", ICRA 2006): the normalised
 * estimation error squared of `count` entries of slamgpu_pose_summary / slamgpu_pose_history_fetch (summary[count][18]) against the
 * true poses xtrue[count][3].  Per entry, in double:
 *     e    = (out[1] - x_t, out[2] - y_t, IEEE remainder(out[3] - theta_t, 2 pi))
 *     P    = scatter + mean Pv, 3 x 3 symmetric: (out[6..11]) + (out[12..17]) in the order xx, xy, yy, xu, yu, uu
 *     NEES = e^T P^-1 e through the Cholesky factor of P
 * nees[k] is NaN for an entry whose P is not positive definite (N = 1, a collapsed set) or whose summary holds a NaN (degenerate
 * weights); the return value counts such entries.  err[count][3] (may be NULL) receives e.  A consistent filter's NEES has mean 3
 * and lies below 7.8147 -- the 95 % point of chi^2 with 3 degrees of freedom -- 95 % of the time.  -1: bad arguments (a negative
 * count, a NULL array that is needed). */
int32_t slamhost_pose_nees(const double *summary, int32_t count, const float *xtrue /*3 per entry*/, double *nees, double *err /*3 per entry, may be NULL*/);

/* The innovation test without ground truth (Bar-Shalom's NIS test): the normalised innovation squared of the filter's predicted-
 * measurement mixture, for `count` entries of slamgpu_innovation_summary / slamgpu_innovation_history_fetch (entries[count][10]).
 * Per entry, in double:
 *     e   = (out[1], out[2])                                   the mean innovation
 *     P   = scatter + mean S, 2 x 2 symmetric: (out[3..5]) + (out[6..8]) in the order 00, 10, 11
 *     NIS = e^T P^-1 e through the Cholesky factor of P
 * nis[k] is NaN for an entry whose share out[0] is 0 (nobody holds the slot), that holds a NaN anywhere (degenerate weights), or
 * whose P is not positive definite; the return value counts such entries.  A consistent filter's NIS has mean 2 and lies below
 * 5.9915 -- -2 ln 0.05, the 95 % point of chi^2 with 2 degrees of freedom -- 95 % of the time; out[9], the mean of the particles' own
 * NIS, leaves the pose uncertainty out of S and reads too large.  -1: bad arguments (a negative count, a NULL array with count > 0). */
int32_t slamhost_innovation_nis(const double *entries, int32_t count, double *nis);

/* The joint posterior of one slamgpu_joint_summary (joint[SLAMGPU_JOINT_SIZE(k)], k listed slots, D = 3 + 2 k) as an EKF-SLAM state
 * in the ordering of slamhost_ekf_state: x[D] = the mean, the heading wrapped into (-pi, pi], and P (D x D, row-major, leading
 * dimension ld >= D) = the dense symmetric total covariance: the scatter, plus mean Pv on the 3 x 3 pose block and the mean Pf of
 * listed slot s on the 2 x 2 block at 3 + 2 s.  The off-diagonal blocks are the scatter's alone: inside a particle the landmarks are
 * independent given its path.  Returns 0 when P is positive definite, judged by a Cholesky factorisation in double; 1 when it is not
 * (N = 1, a collapsed set); -1 for bad arguments (a NULL array, k outside [0, 126], ld < D: nothing is written) or an
 * input that holds a NaN (J empty, degenerate weights): x and P are then filled as far as the input goes, NaN where it is NaN. */
int32_t slamhost_joint_dense(const double *joint, int32_t k, double *x, double *P, int32_t ld);

void slamhost_draw_normals(int32_t count, int32_t dim, float *out); /* count x randn(dim,1): dim+1 rand() each */
int32_t slamhost_draw_strata(int32_t N, float *out);                /* returns the reference's strata count (== N when supported) */
double slamhost_unif_rand(void);                                    /* unifRand (core.cpp:775) */

/* synthetic map generator for BASELINE config 5: n landmarks i.i.d. uniform on [x0,x1]x[y0,y1], SplitMix64(seed) */
void slamhost_synthetic_landmarks(uint64_t seed, int32_t n, float x0, float x1, float y0, float y1, float *lm /*2 x n*/);
int slamhost_write_map(const char *path, const float *lm, int32_t nlm, const float *wp, int32_t nwp);

/* ---- plot wire format + headless sink --------------------------------------------------
 * The backend -> GUI link of the reference: NetworkPlot (src/backend/plotting/NetworkPlot.cpp:22-218) sends one ZeroMQ
 * multipart message per command -- command name, then one frame per value in network byte order as the vendored zmqpp
 * serialises it (libs/zmqpp/message.cpp:225-328) -- over a PAIR socket to tcp://127.0.0.1:4242.  These entry points
 * produce exactly those frames and carry them to any of
 *     tcp://host:port   a ZMTP 3.0 PAIR client: the reference's slam-gui (libzmq) on the other side
 *     file:<path>       a frame file: u32 n_messages, per message u32 n_frames, per frame u32 length + bytes (LE)
 *     gather:<dir>      the GUI's DataGatherer (src/gui/plotting/DataGatherer.cpp:50-138), headless: results.txt,
 *                       errors.txt, times.txt, positions.txt, observedCounts.txt, averageLengthLandmark.txt under
 *                       <dir>/<simulation name>/
 * (several sinks separated by ','; "none" = no sink).  Every call returns 0 on success, -1 on failure
 * (slamhost_last_error). */
typedef struct slamhost_plot slamhost_plot;
slamhost_plot *slamhost_plot_open(const char *spec);
void slamhost_plot_close(slamhost_plot *p);
/* cmd = setLandmarks | setWaypoints | setParticles | setFeatureParticles (NetworkPlot.cpp:22-69) */
int slamhost_plot_xy(slamhost_plot *p, const char *cmd, const double *xs, int32_t nx, const double *ys, int32_t ny);
/* cmd = setLaserLines (idx ignored) | setCovEllipse; the matrix row-major (:71-101) */
int slamhost_plot_matrix(slamhost_plot *p, const char *cmd, uint32_t rows, uint32_t cols, const float *row_major, int32_t idx);
/* cmd = addTruePosition | addEstimatedPosition (2) | setCarTruePosition | setCarEstimatedPosition (3) | setPlotRange (4) */
int slamhost_plot_doubles(slamhost_plot *p, const char *cmd, const double *v, int32_t n);
int slamhost_plot_car_size(slamhost_plot *p, double s, uint32_t id);          /* setCarSize (:123-131) */
int slamhost_plot_u32(slamhost_plot *p, const char *cmd, uint32_t v);         /* loopTime | covEllipseAdd | setCurrentIteration (sends nothing, :176-186) */
int slamhost_plot_cmd(slamhost_plot *p, const char *cmd);                     /* clear | plot | endPlot */
int slamhost_plot_name(slamhost_plot *p, const char *name);                   /* setSimulationName (:168-174) */

#ifdef __cplusplus
}
#endif
#endif
