// EKF-SLAM ensemble on the device (include/slamgpu.h: slamgpu_ens_*): B independent filters, member-major slabs resident in
// device memory, ONE launch per EKFSLAM::sim of all of them.  Kernels and host side in one unit.  Workgroup b owns member b from
// predict to augment, __syncthreads() between the stages: no grid-wide meeting, no spin, no atomics.  The arithmetic of the
// stages is the single filter's, the same functions (ekf_helpers.h); the ensemble's own are the in-place W1 and the VALU rank update.
#include "slamgpu_ctx.h"
#define SLAM_KNS slam_ekf_ens
#include "device_math.h"  // philox4x32, u01, box_muller3, as they are
#include "ekf_helpers.h"
#include "ring.h"

namespace {

using slam_ekf_ens::box_muller3;
using slam_ekf_ens::philox4x32;
using slam_ekf_ens::U4;
using slam_ekf_ens::u01;

constexpr int kWork = 10 * kChunk + 2 * kKMax;  // floats of a member's small work area: H5 [kChunk][10] | v [kKMax] | t [kKMax]
constexpr int kMaxNz = 4096;
constexpr int kMaxId = 1 << 20;  // known association: ids index the host's table
constexpr double kChi2_3_95 = 7.8147;
constexpr int kMaxRun = 4096;         // steps of one slamgpu_ens_run_noise
constexpr int kMaxTrace = 1 << 24;    // records the trace may retain

// one step of every member, by value.  io is the step's packet in device memory: lab [nz] int32 (known association: feature or
// SLAMGPU_ASSOC_NEW per observation, shared) | z_true [nz][2] (sim_noise, shared) | VG [B][2] | phi [B] | z [B][nz][2]; the last
// three are what the members used (the host's for sim, the members' own draws for sim_noise): slamgpu_ens_last_inputs
// a step as the device reads it, uniform across the workgroup: the single step has one inside its by-value arguments, the K-step launch
// (slamgpu_ens_run_noise) reads them from its tape.  64 bytes.  off: where the step's lab [nz] | z_true [nz][2] start in the launch's
// packet, in floats; np: the row stride of the innovation covariance in LDS, a power of two >= 2 min(nz, kChunk); refuse: known
// association, the shared table has no room for the step's new ids, so NO member applies its update or augment; q: the step's row of
// the trace scratch, -1: not traced
struct EnsTapeRec {
    float V, G, phi_true, dt, truth[3];
    int32_t has_truth, observe, nz, off, refuse, np, q;
    uint32_t step;
    int32_t pad;
};
static_assert(sizeof(EnsTapeRec) == 64, "EnsTapeRec");

struct EnsArgs {
    float *P;         // [B][cap_dim][ld]
    float *x;         // [B][ld]
    int32_t *dim;     // [B]
    int32_t *status;  // [B] sticky
    double *acc;      // [B][6], and behind them the trace's scratch: the members' values of the launch's traced steps, [q][B][6]
    float *PHt;       // [B][kKMax][ld]: P H^T of a chunk, k-major, then W1 in its place
    float *work;      // [B][kWork]
    int32_t *iw;      // [B][4 + 3 nzcap]: m, n_new, -, - | labels | observations matched | observations new
    float *io;
    int32_t members, ld, cap_dim, max_landmarks, nzcap;
    int32_t use_heading, batch_update, known, draw;
    uint32_t noise, k0, k1;
    float wheel_base, sigma_phi, r_phi, gate_reject, gate_augment;
    float Q[4], Re[4], R[4];
    float L00, L10, L11, sr0, sr1;  // the lower Cholesky factor of Q; sqrt(R00), sqrt(R11)
    EnsTapeRec st;                  // the single step's own (the K-step launch leaves it alone)
};

// ---- consistency: the member's own row, one lane, in double (slamhost_pose_nees's definitions), every operation rounded on its
// own: the float64 model of the tests evaluates the same formulas in the same order.  With the ring on, the step's own six values go
// to the trace scratch as well: row s.q behind the accumulators (no argument of its own: one more pointer in EnsArgs and the scalar
// registers of ekf_ens_kernel no longer fit without a stack slot)
template <bool kTrace>
__device__ __forceinline__ void ens_consistency(const EnsArgs &a, const EnsTapeRec &s, int b, const float *x, const float *P, int ld) {
#pragma clang fp contract(off)
    double *A6 = a.acc + 6 * (size_t) b;
    double *T6 = kTrace && s.q >= 0 ? a.acc + 6 * ((size_t) a.members * (1 + s.q) + b) : nullptr;
    const double ex = (double) x[0] - (double) s.truth[0], ey = (double) x[1] - (double) s.truth[1];
    const double et = remainder((double) x[2] - (double) s.truth[2], 2.0 * 3.14159265358979323846);
    const double p00 = P[0], p10 = P[(size_t) ld], p11 = P[(size_t) ld + 1], p20 = P[2 * (size_t) ld], p21 = P[2 * (size_t) ld + 1],
                 p22 = P[2 * (size_t) ld + 2];
    bool ok = isfinite(ex) && isfinite(ey) && isfinite(et) && isfinite(p00) && isfinite(p10) && isfinite(p11) && isfinite(p20) && isfinite(p21) &&
              isfinite(p22);
    double nees = 0.0;
    if (ok && p00 > 0.0) {
        const double l00 = sqrt(p00), l10 = p10 / l00, l20 = p20 / l00;
        const double d1 = p11 - l10 * l10;
        if (d1 > 0.0) {
            const double l11 = sqrt(d1), l21 = (p21 - l20 * l10) / l11;
            const double d2 = p22 - l20 * l20 - l21 * l21;
            if (d2 > 0.0) {
                const double l22 = sqrt(d2);
                const double y0 = ex / l00, y1 = (ey - l10 * y0) / l11, y2 = (et - l20 * y0 - l21 * y1) / l22;
                nees = y0 * y0 + y1 * y1 + y2 * y2;
                ok = isfinite(nees);
            } else ok = false;
        } else ok = false;
    } else ok = false;
    if (!ok) {
        A6[1] += 1.0;
        if (T6) {
            T6[0] = 0.0;
            T6[1] = 1.0;
            T6[2] = T6[3] = T6[4] = T6[5] = 0.0;
        }
        return;
    }
    A6[0] += 1.0;
    A6[2] += nees;
    if (nees <= kChi2_3_95) A6[3] += 1.0;
    A6[4] += ex * ex + ey * ey;
    A6[5] += et * et;
    if (T6) {
        T6[0] = 1.0;
        T6[1] = 0.0;
        T6[2] = nees;
        T6[3] = nees <= kChi2_3_95 ? 1.0 : 0.0;
        T6[4] = ex * ex + ey * ey;
        T6[5] = et * et;
    }
}

// one step of member b, from its own draws to the consistency row: THE copy of the ensemble's stages, inlined into the single-step
// kernel and into the K-step kernel's loop.  s is read where it is used (the single step's sits in the kernel's arguments, the tape's in
// device memory that the kernel only reads); packet: the step's lab [nz] | z_true [nz][2]; own: where the member's inputs go, null: the
// io area in the layout of this step's nz (slamgpu_ens_last_inputs reads them there).  dim is the member's dimension, held by every
// lane from step to step: in, and returned
template <bool kTrace>
__device__ __forceinline__ int ens_member_step(const EnsArgs &a, const EnsTapeRec &s, const float *packet, float *own, float *lds, const int b,
                                               const int tid, int dim) {
    const int ld = a.ld, nz = s.nz;
    float *P = a.P + (size_t) b * a.cap_dim * ld;
    float *x = a.x + (size_t) b * ld;
    float *PHt = a.PHt + (size_t) b * kKMax * ld;
    float *H5g = a.work + (size_t) b * kWork, *vg = H5g + 10 * kChunk, *tg = vg + kKMax;
    int32_t *cnt = a.iw + (size_t) b * (4 + 3 * (size_t) a.nzcap), *lab = cnt + 4, *mi = lab + a.nzcap, *ni = mi + a.nzcap;
    const int32_t *lab_known = reinterpret_cast<const int32_t *>(packet);
    const float *z_true = packet + nz;
    float *vg_in = own ? own : a.io + 3 * (size_t) nz + 2 * (size_t) b;
    float *phi_in = own ? own + 2 : a.io + 3 * (size_t) nz + 2 * (size_t) a.members + b;
    float *z_in = own ? own + 3 : a.io + 3 * (size_t) nz + 3 * (size_t) a.members + 2 * (size_t) nz * b;

    // ---- the member's own inputs (sim_noise): Philox stream 5, counter (member, step, 5, q) ------------------------------------
    if (a.draw) {
        if (tid == 0) {
            float V = s.V, G = s.G, phi = s.phi_true;
            if (a.noise & SLAMGPU_EKF_ENS_NOISE_CONTROL) {  // multivariate_gauss2: x + chol(Q) g
                float g0, g1, g2;
                box_muller3(philox4x32((uint32_t) b, s.step, 5u, 0u, a.k0, a.k1), g0, g1, g2);
                V = s.V + a.L00 * g0;
                G = s.G + a.L10 * g0 + a.L11 * g1;
            }
            if (a.noise & SLAMGPU_EKF_ENS_NOISE_HEADING)  // (uncentred, as the reference's unifRand(): ekfslamwrapper.cpp:81)
                phi = s.phi_true + a.sigma_phi * u01(philox4x32((uint32_t) b, s.step, 5u, 1u, a.k0, a.k1).x);
            vg_in[0] = V;
            vg_in[1] = G;
            *phi_in = phi;
        }
        for (int i = tid; i < nz; i += kEkfBlock) {
            float zr = z_true[2 * i], zb = z_true[2 * i + 1];
            if (a.noise & SLAMGPU_EKF_ENS_NOISE_SENSOR) {  // Simulator::observe
                float g0, g1, g2;
                box_muller3(philox4x32((uint32_t) b, s.step, 5u, 2u + (uint32_t) i, a.k0, a.k1), g0, g1, g2);
                zr = zr + g0 * a.sr0;
                zb = zb + g1 * a.sr1;
            }
            z_in[2 * i] = zr;
            z_in[2 * i + 1] = zb;
        }
        __syncthreads();
    }
    const float V = vg_in[0], G = vg_in[1], phi = *phi_in;

    // ---- EkfSlam::predict: everything read into registers, a barrier, then the writes (no ticket: one workgroup) ---------------
    {
        const float th = x[2], x0 = x[0], x1 = x[1];
        const EkfMotion mo = ekf_motion(V, G, th, s.dt);
        float Pvv[3][3];
        ekf_load_pose_block(P, ld, Pvv);
        __syncthreads();
        for (int j = 3 + tid; j < dim; j += kEkfBlock) ekf_predict_column(P, ld, j, mo.vts, mo.vtc);
        if (tid == 0) ekf_predict_pose(P, ld, x, Pvv, x0, x1, th, mo, V, G, s.dt, a.wheel_base, a.Q);
        __syncthreads();
    }

    // ---- EkfSlam::observe_heading: the one-pass form, column 2 of P and the gain in LDS, a lane per column ----------------------
    if (a.use_heading) {
        float *c2 = lds, *Wh = lds + ld;
        const float S = P[2 * (size_t) ld + 2] + a.r_phi;
        const float Si = 1.0f / S;
        const float hv = ekf_trig_offset(phi - x[2]);
        for (int i = tid; i < dim; i += kEkfBlock) ekf_heading_gain(P, ld, i, Si, c2, Wh);
        __syncthreads();
        for (int j = tid; j < dim; j += kEkfBlock) {
            const float wj = Wh[j], cj = c2[j];
            x[j] = x[j] + wj * hv;
            for (int i = 0; i < dim; i++) P[(size_t) i * ld + j] = ekf_heading_element(P[(size_t) i * ld + j], Wh[i], c2[i], wj, cj, S, i == j);
        }
        __syncthreads();
    }

    if (s.observe) {
        const int nf = (dim - 3) / 2;
        // ---- labels: the shared table's, or the gates over (observation, feature) pairs against the state as it stands --------------
        if (a.known) {
            for (int i = tid; i < nz; i += kEkfBlock) {
                const int l = lab_known[i];
                lab[i] = l >= nf ? SLAMGPU_ASSOC_DISCARD : l;  // (a member that lacks the feature ignores the observation)
            }
        } else {
            // a wave per observation, its lanes over the features, the lanes' candidates merged through the wave's shuffles
            const int wave = tid >> 6, lane = tid & 63;
            float Pvv[3][3];
            ekf_load_pose_block(P, ld, Pvv);
            const float inf = __builtin_huge_valf();
            for (int i = wave; i < nz; i += kEkfBlock / 64) {
                const float z0 = z_in[2 * i], z1 = z_in[2 * i + 1];
                float nbest = inf, outer = inf;
                int jbest = -1;
                for (int j = lane; j < nf; j += 64) {
                    float nis, nd;
                    ekf_gate_pair(P, ld, x, Pvv, a.Re, z0, z1, j, &nis, &nd);
                    ekf_gate_keep(nbest, outer, jbest, nis, nd, j, a.gate_reject);
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const float nb = __shfl_xor(nbest, s, 64), ob = __shfl_xor(outer, s, 64);
                    const int jb = __shfl_xor(jbest, s, 64);
                    ekf_gate_merge(nbest, outer, jbest, nb, ob, jb);
                }
                if (lane == 0) lab[i] = ekf_gate_label(outer, jbest, a.gate_augment);
            }
        }
        __syncthreads();
        if (tid == 0) {  // the step's matched and new observations, in observation order
            int m = 0, nn = 0;
            for (int i = 0; i < nz; i++) {
                const int l = lab[i];
                if (l >= 0) mi[m++] = i;
                else if (l == SLAMGPU_ASSOC_NEW) ni[nn++] = i;
            }
            if (nf + nn > a.max_landmarks || s.refuse) {  // the step does not fit: neither its update nor its augment is applied
                a.status[b] |= SLAMGPU_EKF_STATUS_CAPACITY;
                m = nn = 0;
            }
            cnt[0] = a.batch_update ? m : 0;
            cnt[1] = nn;
        }
        __syncthreads();
        const int m = cnt[0], nn = cnt[1];
        const int np = s.np;

        // ---- EkfSlam::batch_update, chunk by chunk ----------------------------------------------------------------------------------
        for (int at = 0; at < m; at += kChunk) {
            const int mc = min(kChunk, m - at), n = 2 * mc;
            if (tid < mc) {  // H5 and the innovation of observation at + tid
                const int o = mi[at + tid];
                float H5[10];
                ekf_innovation(x, lab[o], true, z_in[2 * o], z_in[2 * o + 1], tid, H5, H5g, vg);
            }
            __syncthreads();
            for (int r = tid; r < dim; r += kEkfBlock) {  // P H^T: rows of P, coalesced along r
                const float p0 = P[r], p1 = P[(size_t) ld + r], p2 = P[2 * (size_t) ld + r];
                for (int i = 0; i < mc; i++) {
                    const size_t f = 3 + 2 * (size_t) lab[mi[at + i]];
                    const float p[5] = {p0, p1, p2, P[f * ld + r], P[(f + 1) * ld + r]};
                    ekf_pht(p, H5g + 10 * i, PHt, ld, i, r);
                }
            }
            __syncthreads();
            ekf_innov_cov(lds, np, n, H5g, PHt, ld, a.R, [&](int i) { return lab[mi[at + i]]; });
            if (ekf_llt_lower(lds, np, n)) {  // the chunk is skipped: neither x nor P changes (the verdict is uniform)
                if (tid == 0) a.status[b] |= SLAMGPU_EKF_STATUS_NOT_PD;
                __syncthreads();
                continue;
            }
            ekf_upper_inverse(lds, np, n, vg, tg);
            __syncthreads();
            if (tid < n) ekf_at(lds, np, tid, tid) = 1.0f / ekf_at(lds, np, tid, tid);  // the diagonal of U^-1 in its place: (k, c), k <= c, is now X(k, c)
            __syncthreads();
            // W1 = PHt U^-1 (k ascending, as the host's mul) IN PLACE of PHt: column c needs the columns k <= c only, so c runs
            // downwards; and x += W1 t (the host forms W = W1 U^-T and W v: the same sum, associated the other way)
            for (int r = tid; r < dim; r += kEkfBlock) {
                float xacc = 0.0f;
                for (int c = n - 1; c >= 0; c--) {
                    float acc = 0.0f;
                    for (int k = 0; k <= c; k++) acc = acc + PHt[(size_t) k * ld + r] * ekf_at(lds, np, k, c);
                    PHt[(size_t) c * ld + r] = acc;
                    xacc = xacc + acc * tg[c];
                }
                x[r] = x[r] + xacc;
            }
            __syncthreads();
            // P -= W1 W1^T on the VALU: four rows i0 .. i0 + 3 per wave at a time, its lanes over the columns j <= i0 + 3, a k-ordered
            // fma chain per element.  Only elements on or below the diagonal are computed; each is written twice, the second time
            // mirrored: P == P^T bit for bit.  W1's columns >= dim (allocated, never data) only reach accumulators that are not stored
            {
                const int wave = tid >> 6, lane = tid & 63;
                for (int i0 = 4 * wave; i0 < dim; i0 += 4 * (kEkfBlock / 64))
                    for (int j = lane; j <= i0 + 3 && j < dim; j += 64) {
                        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
                        for (int k = 0; k < n; k++) {
                            const float *w = PHt + (size_t) k * ld;
                            const float wj = w[j];
                            acc0 = acc0 + w[i0] * wj;
                            acc1 = acc1 + w[i0 + 1] * wj;
                            acc2 = acc2 + w[i0 + 2] * wj;
                            acc3 = acc3 + w[i0 + 3] * wj;
                        }
                        const float acc[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int i = i0 + e;
                            if (i < dim && j <= i) {
                                const float p = P[(size_t) i * ld + j] - acc[e];
                                P[(size_t) i * ld + j] = p;
                                if (j < i) P[(size_t) j * ld + i] = p;
                            }
                        }
                    }
            }
            __syncthreads();
        }

        // ---- EkfSlam::augment, one feature after another: each one's rows start from the pose rows, which the previous one left alone
        for (int q = 0; q < nn; q++) {
            const int o = ni[q], len = dim;
            const float r = z_in[2 * o];
            const EkfBearing g = ekf_bearing(x, r, z_in[2 * o + 1]);
            for (int j = tid; j < len; j += kEkfBlock) ekf_augment_column(P, ld, len, j, g.g02, g.g12);
            if (tid == 0) ekf_augment_block(P, ld, len, x, r, g, a.Re);
            dim += 2;
            __syncthreads();
        }
    }

    if (tid == 0) {
        a.dim[b] = dim;
        if (s.has_truth) ens_consistency<kTrace>(a, s, b, x, P, ld);
    }
    return dim;
}

// kTrace: the step leaves its row of the trace (the ring is on and the step has a truth); without it the kernel has no trace code at all
template <bool kTrace>
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_kernel(EnsArgs a) {
    extern __shared__ float lds[];  // heading: column 2 of P and the gain, [2][ld]; update: the innovation covariance, [np][np]
    const int b = blockIdx.x, tid = threadIdx.x;
    ens_member_step<kTrace>(a, a.st, a.io, nullptr, lds, b, tid, a.dim[b]);
}

// K steps of every member in one launch (slamgpu_ens_run_noise): workgroup b owns member b from the tape's first step to its last, a
// barrier after the last stage of each step -- it is what makes the step's global writes to P, x, status and the accumulators visible
// to the same workgroup's next step.  tape and packet are only read.  The member's draws of the steps before the last go to its own
// row of `draws` (3 + 2 zstride floats: steps of different nz would overlap other members' rows in the io layout while those still
// read them); the last step's go to the io area in that step's layout
// (tape and packet are NOT __restrict__: declared so, a step's record arrives in sixteen scalar registers at once, the scalar allocator
// runs out, and the kernel is left with a stack slot nothing uses and a private segment; as they are it has none)
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_run_kernel(EnsArgs a, const EnsTapeRec *tape, const float *packet,
                                                                 float *draws, int K, int zstride) {
    extern __shared__ float lds[];  // sized by the host to the largest need of any step of the tape
    const int b = blockIdx.x, tid = threadIdx.x;
    float *own = draws + (size_t) b * (3 + 2 * (size_t) zstride);
    int dim = a.dim[b];
    for (int k = 0; k < K; k++) {
        dim = ens_member_step<true>(a, tape[k], packet + tape[k].off, k == K - 1 ? nullptr : own, lds, b, tid, dim);
        __syncthreads();
    }
}

// the trace's records of a launch: workgroup q sums the members' values of traced step q in an order that depends on `members` alone
// (lane t takes members t, t + 256, ... in turn, then the lanes meet in a fixed tree) and writes the record into its slot of the ring
// The record's tag is the step word of the tape's step whose row is q, or `tag` for a single step (tape null)
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_trace_kernel(const double *__restrict__ val, const EnsTapeRec *__restrict__ tape, int K, uint32_t tag,
                                                                   int members, double *__restrict__ rec, uint32_t *__restrict__ rtag, long long next, int cap) {
    __shared__ double sh[6][kEkfBlock];
    const int q = blockIdx.x, tid = threadIdx.x;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < members; b += kEkfBlock) {
        const double *v = val + 6 * ((size_t) q * members + b);
#pragma unroll
        for (int c = 0; c < 6; c++) acc[c] = acc[c] + v[c];
    }
#pragma unroll
    for (int c = 0; c < 6; c++) sh[c][tid] = acc[c];
    __syncthreads();
    for (int w = kEkfBlock / 2; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int c = 0; c < 6; c++) sh[c][tid] = sh[c][tid] + sh[c][tid + w];
        __syncthreads();
    }
    const size_t slot = (size_t) ((next + q) % cap);
    if (tid < 6) rec[6 * slot + tid] = sh[tid][0];
    if (!tape) {
        if (tid == 0) rtag[slot] = tag;
    } else
        for (int k = tid; k < K; k += kEkfBlock)  // (one step of the tape has this row)
            if (tape[k].q == q) rtag[slot] = tape[k].step;
}

// slamgpu_ens_poses: out[b][12] = x, y, theta, Pvv row-major
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_pose_kernel(const float *__restrict__ P, const float *__restrict__ x, int ld, int cap_dim, int members,
                                                                  double *__restrict__ out) {
    const int e = blockIdx.x * kEkfBlock + threadIdx.x;
    if (e >= 12 * members) return;
    const int b = e / 12, q = e - 12 * b;
    out[e] = q < 3 ? (double) x[(size_t) b * ld + q] : (double) P[(size_t) b * cap_dim * ld + (size_t) ((q - 3) / 3) * ld + (q - 3) % 3];
}

// ---- slamgpu_ens_moments: the sample mean and covariance of the members' states and the mean of their P, over the set J of the header.
// Tiles of kMomTile consecutive members; every sum over members ascending within a tile, the tiles ascending, no atomics.  The Gram
// pass is slamgpu_joint_summary's (kernels.hip, joint_gram_kernel) without weights, genealogy or records: a copy of its own, because
// that kernel lives in the particle filter's unit behind its Buffers and a shared form would change its instructions.
constexpr int kMomTile = 256;   // consecutive members of a tile (= kEkfBlock: a lane per member where a tile's flags are staged)
constexpr int kMomSubMax = 16;  // members centred into LDS at a time: 16 (four matrix instructions' worth) up to 320 columns of d_ext, 4 beyond
constexpr int kMomGroup = 16;   // block pairs of a workgroup of the Gram pass: four per wave
constexpr int kMomBatch = 32;   // members whose loads a lane of the mean-of-P pass has in flight (one word of the tile's flag bits)
constexpr int kMomSelLanes = 4; // lanes of the select pass that share a member
constexpr double kMomTwoPi = 6.283185307179586476925286766559;
typedef double mom_d4 __attribute__((ext_vector_type(4)));

// first, count: the chunk of block pairs (Gram, reduce) or of row blocks of `rows` rows of P (mean of P) that goes through `part`
struct MomArgs {
    const float *P, *x;
    const int32_t *dim, *status;
    int32_t members, ld, cap_dim, D, Dp, tiles, first, count, rows;
    uint32_t exclude;
    int32_t *flag;       // [members] 1: in J
    int32_t *info;       // pivot (-1: J is empty), n
    double *pivot;       // [Dp] the pivot's x[0:D], then zeros
    double *sums;        // [block pairs][256] sum d_ext d_ext^T, lower-triangle block pairs R (R + 1) / 2 + C
    double *part;        // the chunk's partials, per tile
    double *mean, *C, *Pbar;
};

// the lowest member and the count of a workgroup's lanes: in every lane on return
__device__ __forceinline__ void mom_first_count(int &first, int &cnt, int *sh) {
    for (int d = 32; d > 0; d >>= 1) {
        first = min(first, __shfl_xor(first, d, 64));
        cnt += __shfl_xor(cnt, d, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[2 * wave] = first;
        sh[2 * wave + 1] = cnt;
    }
    __syncthreads();
    first = sh[0];
    cnt = sh[1];
    for (int v = 1; v < kEkfBlock / 64; v++) {
        first = min(first, sh[2 * v]);
        cnt += sh[2 * v + 1];
    }
}

// select: kMomSelLanes lanes per member, each every kMomSelLanes-th component; integers only (finite: the exponent field is not all ones)
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_select_kernel(MomArgs m) {
    const int b = blockIdx.x * (kEkfBlock / kMomSelLanes) + threadIdx.x / kMomSelLanes, q = threadIdx.x & (kMomSelLanes - 1);
    int ok = 0;
    if (b < m.members) {
        ok = m.dim[b] >= m.D && ((uint32_t) m.status[b] & m.exclude) == 0u;
        if (ok) {
            const float *xb = m.x + (size_t) b * m.ld, *Pb = m.P + (size_t) b * m.cap_dim * m.ld;
            for (int c = q; c < m.D; c += kMomSelLanes) {
                const uint32_t ux = __float_as_uint(xb[c]), up = __float_as_uint(Pb[(size_t) c * m.ld + c]);
                ok &= (ux & 0x7f800000u) != 0x7f800000u && (up & 0x7f800000u) != 0x7f800000u;
            }
        }
    }
    for (int d = 1; d < kMomSelLanes; d <<= 1) ok &= __shfl_xor(ok, d, 64);
    if (b < m.members && q == 0) m.flag[b] = ok;
}

// one workgroup: the pivot (the lowest member of J), n and the pivot's vector
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_pivot_kernel(MomArgs m) {
    __shared__ int sh[2 * (kEkfBlock / 64)];
    int first = INT_MAX, cnt = 0;
    for (int b = threadIdx.x; b < m.members; b += kEkfBlock)
        if (m.flag[b]) {
            first = min(first, b);
            cnt++;
        }
    mom_first_count(first, cnt, sh);
    if (threadIdx.x == 0) {
        m.info[0] = cnt ? first : -1;
        m.info[1] = cnt;
    }
    for (int c = threadIdx.x; c < m.Dp; c += kEkfBlock) m.pivot[c] = cnt && c < m.D ? (double) m.x[(size_t) first * m.ld + c] : 0.0;
}

// Gram pass, grid (tiles, groups of kMomGroup block pairs): d_ext = (v - pivot, 1) of SUB members at a time in LDS, rows of ldl
// doubles (an odd multiple of 16: the four members of an instruction never share banks), zero outside J and in the padding; each wave
// four block pairs, A[m = lane & 15][k = lane >> 4] = d[row block + m], B[k][n = lane & 15] = d[column block + n] of member k.
// Lane tid stages member tid & (SUB - 1) of the sub-tile, columns tid / SUB + (256 / SUB) k, k < NP.  The members' floats of DEPTH
// sub-tiles are fetched into registers at once, unconditionally (past the tile's end and past column D the last valid one again, never
// used).  A tile is a chain of sub-tiles, each two barriers and a few LDS round trips long, and the kernel's time is that chain's: SUB is
// 16 wherever 16 rows of d_ext fit in LDS (43 KB at 320 columns), 4 beyond.  NP, DEPTH and SUB are compiled in so that the fetched floats
// are registers; the heading's deviation, the one remainder, is taken once per member before the loop
template <int NP, int DEPTH, int SUB>
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_gram_kernel(MomArgs m) {
#pragma clang fp contract(off)
    extern __shared__ double mom_lds[];  // d_ext [SUB][ldl] | pivot [Dp]
    __shared__ int sh_flag[kMomTile];
    __shared__ double sh_u[kMomTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ldl = (m.Dp & 16) ? m.Dp : m.Dp + 16;
    double *sh_d = mom_lds, *sh_p = mom_lds + SUB * ldl;
    const int b0 = blockIdx.x * kMomTile;
    {
        const int f = b0 + tid < m.members ? m.flag[b0 + tid] : 0;
        sh_flag[tid] = f;
        sh_u[tid] = f ? remainder((double) m.x[(size_t) (b0 + tid) * m.ld + 2] - m.pivot[2], kMomTwoPi) : 0.0;
    }
    for (int c = tid; c < m.Dp; c += kEkfBlock) sh_p[c] = m.pivot[c];
    for (int e = tid; e < SUB * ldl; e += kEkfBlock) sh_d[e] = 0.0;  // (the padding columns stay zero)
    __syncthreads();
    int rb[4], cb[4];
    bool bv[4];
    mom_d4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int bpl = blockIdx.y * kMomGroup + wave * 4 + b;
        bv[b] = bpl < m.count;
        const int bp = m.first + bpl;
        int R = 0;
        while ((R + 1) * (R + 2) / 2 <= bp) R++;
        rb[b] = bv[b] ? R * 16 : 0;
        cb[b] = bv[b] ? (bp - R * (R + 1) / 2) * 16 : 0;
        acc[b] = mom_d4{0.0, 0.0, 0.0, 0.0};
    }
    const int nsub = (min(kMomTile, m.members - b0) + SUB - 1) / SUB;
    const int p = tid & (SUB - 1), c0 = tid / SUB;
    constexpr int kStep = kEkfBlock / SUB;
    for (int s0 = 0; s0 < nsub; s0 += DEPTH) {
        float xv[DEPTH][NP];
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            const float *xb = m.x + (size_t) min(b0 + (s0 + d) * SUB + p, m.members - 1) * m.ld;
#pragma unroll
            for (int k = 0; k < NP; k++) xv[d][k] = xb[min(c0 + kStep * k, m.D - 1)];
        }
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            const int st = s0 + d;
            if (st < nsub) {  // (uniform)
                const int q = st * SUB + p;
                const bool in = q < kMomTile && sh_flag[q] != 0;
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    const int c = c0 + kStep * k;
                    if (c <= m.D) {
                        double v = 0.0;
                        if (in) v = c == m.D ? 1.0 : c == 2 ? sh_u[q] : (double) xv[d][k] - sh_p[c];
                        sh_d[p * ldl + c] = v;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < SUB / 4; kk++) {  // four members per instruction, in ascending order
                    const double *rw = sh_d + (kk * 4 + (lane >> 4)) * ldl + (lane & 15);
#pragma unroll
                    for (int b = 0; b < 4; b++)  // (a wave with fewer than four block pairs computes block pair (0, 0) in their place and drops it: a
                        acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(rw[rb[b]], rw[cb[b]], acc[b], 0, 0, 0);  // test here costs the accumulators their registers)
                }
                __syncthreads();
            }
        }
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (bv[b]) {
            const int bpl = blockIdx.y * kMomGroup + wave * 4 + b;
            double *o = m.part + ((size_t) blockIdx.x * (size_t) m.count + (size_t) bpl) * 256;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) o[((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[b][reg];
        }
    }
}

// the tiles' partials of one block pair, added in ascending order
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_reduce_kernel(MomArgs m) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int t = 0; t < m.tiles; t++) s = s + m.part[((size_t) t * (size_t) m.count + blockIdx.x) * 256 + threadIdx.x];
    m.sums[(size_t) (m.first + blockIdx.x) * 256 + threadIdx.x] = s;
}

// entry (r, c), c <= r, of sum d_ext d_ext^T
__device__ __forceinline__ double mom_sum(const MomArgs &m, int r, int c) {
    const int R = r >> 4;
    return m.sums[(size_t) (R * (R + 1) / 2 + (c >> 4)) * 256 + (r & 15) * 16 + (c & 15)];
}

// mean and C, a thread per output: e < D the mean's components, then the lower triangle of C (both halves written)
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_finish_kernel(MomArgs m) {
#pragma clang fp contract(off)
    const int D = m.D, T = m.C ? D * (D + 1) / 2 : 0;
    const int e = blockIdx.x * kEkfBlock + threadIdx.x;
    if (e >= D + T) return;
    const int cnt = m.info[1];
    const double n = (double) cnt, nan = __longlong_as_double(0x7ff8000000000000ll);
    if (e < D) {
        double v = nan;
        if (cnt) {
            v = m.pivot[e] + mom_sum(m, D, e) / n;
            if (e == 2) {  // the heading into (-pi, pi], as slamhost_joint_dense wraps
                v = remainder(v, kMomTwoPi);
                if (v <= -kMomTwoPi / 2) v += kMomTwoPi;
            }
        }
        m.mean[e] = v;
        return;
    }
    const int t = e - D;
    int r = (int) ((sqrt(8.0 * (double) t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) r--;
    while ((r + 1) * (r + 2) / 2 <= t) r++;
    const int c = t - r * (r + 1) / 2;
    double v = nan;
    if (cnt) {
        const double dr = mom_sum(m, D, r) / n, dc = mom_sum(m, D, c) / n;
        v = mom_sum(m, r, c) / n - dr * dc;
    }
    m.C[(size_t) r * D + c] = v;
    m.C[(size_t) c * D + r] = v;
}

// mean of P, grid (row blocks of the chunk, tiles): the block's rows are one stretch of `rows` ld floats of a member's slab, a lane
// four columns of it at a time (16-byte loads), the tile's members in ascending order, in double; members outside J are skipped by a
// test of the tile's flag bits that is uniform across the workgroup.  Only the float4s that reach into the lower triangle
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_pbar_kernel(MomArgs m) {
#pragma clang fp contract(off)
    __shared__ uint32_t sh_mask[kMomTile / 32];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int b0 = t * kMomTile;
    {
        const unsigned long long bal = __ballot(b0 + tid < m.members && m.flag[b0 + tid] != 0);
        if ((tid & 63) == 0) {
            sh_mask[2 * (tid >> 6)] = (uint32_t) bal;
            sh_mask[2 * (tid >> 6) + 1] = (uint32_t) (bal >> 32);
        }
    }
    __syncthreads();
    const int cnt = min(kMomTile, m.members - b0);
    const int ld4 = m.ld / 4, r0 = (m.first + (int) blockIdx.x) * m.rows, nrow = min(m.rows, m.D - r0);
    const size_t slab4 = (size_t) m.cap_dim * ld4;
    double *o = m.part + ((size_t) t * (size_t) m.count + blockIdx.x) * ((size_t) m.rows * m.ld);
    for (int e = tid; e < nrow * ld4; e += kEkfBlock) {
        const int rl = e / ld4, c4 = e - rl * ld4;
        if (4 * c4 > r0 + rl) continue;
        const float4 *src = reinterpret_cast<const float4 *>(m.P) + (size_t) b0 * slab4 + (size_t) (r0 + rl) * ld4 + c4;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int q0 = 0; q0 < cnt; q0 += kMomBatch) {
            const uint32_t bits = (uint32_t) __builtin_amdgcn_readfirstlane((int) sh_mask[q0 >> 5]);
            static_assert(kMomBatch == 32, "a batch is one word of the flag bits");
            if (!bits) continue;  // (nobody of this batch is in J)
            // every load of the batch is issued before the first sum waits for one: the loads are NOT under the flag's test (a load inside
            // a branch made the compiler wait for each before the next: the pass ran at one load's latency per member), only the sums
            // are; a member outside J costs its bytes, nothing else.  Past the tile's end the last member is read again and not added
            float4 v[kMomBatch];
#pragma unroll
            for (int j = 0; j < kMomBatch; j++) v[j] = src[(size_t) min(q0 + j, cnt - 1) * slab4];
#pragma unroll
            for (int j = 0; j < kMomBatch; j++)
                if (bits >> j & 1u) {
                    a0 = a0 + (double) v[j].x;
                    a1 = a1 + (double) v[j].y;
                    a2 = a2 + (double) v[j].z;
                    a3 = a3 + (double) v[j].w;
                }
        }
        double *oe = o + (size_t) rl * m.ld + 4 * c4;
        oe[0] = a0;
        oe[1] = a1;
        oe[2] = a2;
        oe[3] = a3;
    }
}

// ... and its finish, a thread per entry (row of the chunk, column < D): the tiles in ascending order, over n, mirrored
__global__ void __launch_bounds__(kEkfBlock) ekf_ens_mom_pbar_finish_kernel(MomArgs m) {
#pragma clang fp contract(off)
    const int D = m.D, r0 = m.first * m.rows, nrow = min(m.count * m.rows, D - r0);
    const int e = blockIdx.x * kEkfBlock + threadIdx.x;
    if (e >= nrow * D) return;
    const int ra = e / D, c = e - ra * D, r = r0 + ra;
    if (c > r) return;
    const int rbl = ra / m.rows, rl = ra - rbl * m.rows;
    const int cnt = m.info[1];
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (cnt) {
        const size_t block = (size_t) m.rows * m.ld;
        double s = 0.0;
        for (int t = 0; t < m.tiles; t++) s = s + m.part[((size_t) t * (size_t) m.count + rbl) * block + (size_t) rl * m.ld + c];
        v = s / (double) cnt;
    }
    m.Pbar[(size_t) r * D + c] = v;
    m.Pbar[(size_t) c * D + r] = v;
}

}  // namespace

struct slamgpu_ekf_ens {
    slamgpu_ekf_ens_config cfg{};
    EkfStream stream;
    int B = 0, ld = 0, cap_dim = 0;
    DevBuf<float> P, x, PHt, work, io;
    DevBuf<int32_t> dim, status, iw;
    DevBuf<double> acc, pose_dev;
    int nzcap = 0;
    int last_nz = -1;  // the observations of the last step's packet (-1: no step yet)
    // the step's packet on its way down: two pinned slots used in turn, so that a step does not wait for the copy of the previous one
    PinBuf<char> pin;
    size_t slot_bytes = 0;
    SlotRing<2> slots;
    EkfIdTable table;  // association_known (ONE table: every member has the same dimension)
    int nf_known = 0;  // ... and the features it has handed out
    // slamgpu_ens_run_noise: the launch's tape in device memory (EnsTapeRec [K] | per step lab [nz] | z_true [nz][2]) and the members'
    // own draws of the steps before the last, [B][3 + 2 zstride]
    DevBuf<char> tape;
    DevBuf<float> draws;
    // the trace: records [cap][6] and tags [cap] in device memory, the counters on the host; the scratch of one launch, grow-only
    Ring ring;
    DevBuf<double> tr_rec;
    DevBuf<uint32_t> tr_rtag;
    // slamgpu_ens_moments: its workspace, nothing until the first call, grow-only
    DevBuf<char> mom;
};

namespace {

int ens_check(slamgpu_ekf_ens *e) {
    if (!e) return fail(SLAMGPU_ERR_INVALID, "null EKF ensemble handle");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return 0;
}

void ens_release(slamgpu_ekf_ens *e) {
    e->P.release();
    e->x.release();
    e->PHt.release();
    e->work.release();
    e->io.release();
    e->dim.release();
    e->status.release();
    e->iw.release();
    e->acc.release();
    e->pose_dev.release();
    e->tape.release();
    e->draws.release();
    e->tr_rec.release();
    e->tr_rtag.release();
    e->mom.release();
    e->pin.release();
    e->slots.release();
    e->stream.release();
    delete e;
}

int ens_reserve(slamgpu_ekf_ens *e) {
    if (int rc = e->stream.create()) return rc;
    const size_t B = (size_t) e->B, ld = (size_t) e->ld;
    if (int rc = e->P.reserve_zeroed(B * ld * e->cap_dim, "EKF ensemble covariances P")) return rc;
    if (int rc = e->x.reserve_zeroed(B * ld, "EKF ensemble states x")) return rc;
    if (int rc = e->PHt.reserve_zeroed(B * ld * kKMax, "EKF ensemble P H^T")) return rc;
    if (int rc = e->work.reserve_zeroed(B * kWork, "EKF ensemble work area")) return rc;
    if (int rc = e->dim.reserve_zeroed(B, "EKF ensemble dimensions")) return rc;
    if (int rc = e->status.reserve_zeroed(B, "EKF ensemble status")) return rc;
    if (int rc = e->acc.reserve_zeroed(6 * B, "EKF ensemble accumulators")) return rc;
    if (int rc = e->pose_dev.reserve_zeroed(12 * B, "EKF ensemble poses")) return rc;
    const std::vector<int32_t> three(B, 3);
    HIP_TRY(hipMemcpy(e->dim, three.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice));
    e->slot_bytes = 4096;
    if (int rc = e->pin.reserve(2 * e->slot_bytes, "EKF ensemble staging")) return rc;
    return e->slots.create();
}

// what a launch needs room for: steps of at most nz observations, a packet of `bytes` in a pinned slot; a K-step launch also its tape and
// the members' draws, a traced one nq rows of the trace scratch
struct EnsNeeds {
    int32_t nz = 0;
    size_t bytes = 0, tape_bytes = 0, draw_floats = 0, nq = 0;
};

// A buffer that has to grow is grown with the stream idle (one synchronisation, whichever buffers grow; those that fit are left alone)
int ens_room(slamgpu_ekf_ens *e, const EnsNeeds &n) {
    const size_t B = (size_t) e->B;
    const int32_t nz = n.nz;
    const size_t bytes = n.bytes, tape_bytes = n.tape_bytes, draw_floats = n.draw_floats, nq = n.nq;
    const size_t io_floats = 3 * (size_t) nz + 3 * B + 2 * B * (size_t) nz;
    if (nz > e->nzcap || io_floats > e->io.cap || bytes > e->slot_bytes || tape_bytes > e->tape.cap || draw_floats > e->draws.cap ||
        6 * B * (1 + nq) > e->acc.cap) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (int rc = e->tape.reserve(tape_bytes, "EKF ensemble tape")) return rc;
        if (int rc = e->draws.reserve_zeroed(draw_floats, "EKF ensemble draws")) return rc;
        if (6 * B * (1 + nq) > e->acc.cap) {  // the trace's scratch lies behind the accumulators, which move with it
            DevBuf<double> grown;
            if (int rc = grown.reserve_zeroed(6 * B * (1 + nq), "EKF ensemble accumulators and trace scratch")) return rc;
            HIP_TRY(hipMemcpy(grown.p, e->acc.p, sizeof(double) * 6 * B, hipMemcpyDeviceToDevice));
            std::swap(grown, e->acc);
            grown.release();
        }
        const int cap = std::max(nz, std::max(e->nzcap, 64));
        if (int rc = e->iw.reserve_zeroed(B * (4 + 3 * (size_t) cap), "EKF ensemble labels")) return rc;
        e->nzcap = cap;
        if (int rc = e->io.reserve_zeroed(3 * (size_t) cap + 3 * B + 2 * B * (size_t) cap, "EKF ensemble inputs")) return rc;
        if (bytes > e->slot_bytes) {
            const size_t want = (std::max(bytes, (size_t) 4096) + 255) / 256 * 256;
            e->slots.reset();
            if (int rc = e->pin.reserve(2 * want, "EKF ensemble staging")) return rc;
            e->slot_bytes = want;
        }
    }
    return 0;
}

// the shared labels of the known association, as slamgpu_ekf_sim's table makes them, WITHOUT touching the table: `idn` are the ids that
// are new, in observation order (distinct: ens_step has refused a repeated unseen id); they take the features nf_known ... when the step
// fits.  When it does not, the return value is true and every member refuses the step (SLAMGPU_EKF_STATUS_CAPACITY)
bool ens_known_labels(const EkfIdTable &table, int nf_known, int max_landmarks, const int32_t *ids, int32_t nz, int32_t *lab, std::vector<int32_t> &idn) {
    for (int32_t i = 0; i < nz; i++) {
        const int32_t f = table.lookup(ids[i]);
        lab[i] = f >= 0 ? f : SLAMGPU_ASSOC_NEW;
        if (f < 0) idn.push_back(ids[i]);
    }
    return nf_known + (int) idn.size() > max_landmarks;
}

// a step's ids against the table's rules: inside [0, 2^20), an id not seen before at most once
int ens_check_ids(const EkfIdTable &table, const int32_t *ids, int32_t nz) {
    std::vector<int32_t> unseen;
    for (int32_t i = 0; i < nz; i++) {
        if (ids[i] < 0 || ids[i] >= kMaxId) return fail(SLAMGPU_ERR_INVALID, "ids[%d] = %d outside [0, %d)", i, ids[i], kMaxId);
        if (table.lookup(ids[i]) < 0) unseen.push_back(ids[i]);
    }
    std::sort(unseen.begin(), unseen.end());
    if (std::adjacent_find(unseen.begin(), unseen.end()) != unseen.end())
        return fail(SLAMGPU_ERR_INVALID, "an id not seen before appears twice in one step (it would be appended twice)");
    return 0;
}

// the noise flags and, where control noise is drawn, the lower Cholesky factor of Q, once, in float: L = L00, L10, L11
int ens_check_noise(const float Q[4], bool draw, uint32_t noise, float L[3]) {
    L[0] = L[1] = L[2] = 0.0f;
    if (draw && (noise & SLAMGPU_EKF_ENS_NOISE_CONTROL)) {
        if (!(Q[0] > 0.0f)) return fail(SLAMGPU_ERR_INVALID, "control noise: Q is not positive definite");
        L[0] = std::sqrt(Q[0]);
        L[1] = Q[2] / L[0];
        const float d = Q[3] - L[1] * L[1];
        if (!(d > 0.0f)) return fail(SLAMGPU_ERR_INVALID, "control noise: Q is not positive definite");
        L[2] = std::sqrt(d);
    }
    if (draw && (noise & ~7u)) return fail(SLAMGPU_ERR_INVALID, "noise flags %u", noise);
    return 0;
}

// the row stride of a step's innovation covariance in LDS, and the launch's dynamic LDS in floats: the heading stage's two columns or the
// chunk's innovation covariance, whichever is larger (at most 64 KB: np <= 128, ld <= 1056)
int ens_np(int32_t nz) {
    int np = 2;
    while (np < 2 * std::min(nz, kChunk)) np *= 2;
    return np;
}
size_t ens_lds_floats(const slamgpu_ekf_ens *e, int32_t observe, int32_t nz, int np) {
    size_t lds_floats = observe && e->cfg.batch_update && nz > 0 ? (size_t) np * np : 4;
    if (e->cfg.use_heading) lds_floats = std::max(lds_floats, 2 * (size_t) e->ld);
    return lds_floats;
}

// what every step of a launch shares: the handle's buffers and settings, the noise matrices, the Philox key
void ens_shared_args(const slamgpu_ekf_ens *e, EnsArgs &a, const float *Q, const float *Re, const float *R, const float L[3], bool draw, uint32_t noise) {
    a.P = e->P; a.x = e->x; a.dim = e->dim; a.status = e->status; a.acc = e->acc; a.PHt = e->PHt; a.work = e->work; a.iw = e->iw; a.io = e->io;
    a.members = e->B; a.ld = e->ld; a.cap_dim = e->cap_dim; a.max_landmarks = e->cfg.max_landmarks; a.nzcap = e->nzcap;
    a.use_heading = e->cfg.use_heading != 0; a.batch_update = e->cfg.batch_update != 0; a.known = e->cfg.association_known != 0;
    a.draw = draw; a.noise = noise; a.k0 = (uint32_t) e->cfg.seed; a.k1 = (uint32_t) (e->cfg.seed >> 32);
    a.wheel_base = e->cfg.wheel_base; a.sigma_phi = e->cfg.sigma_phi;
    a.r_phi = (float) std::pow((double) e->cfg.sigma_phi, 2);
    a.gate_reject = e->cfg.gate_reject; a.gate_augment = e->cfg.gate_augment;
    for (int q = 0; q < 4; q++) {
        a.Q[q] = Q[q];
        a.Re[q] = Re ? Re[q] : 0.0f;
        a.R[q] = R ? R[q] : 0.0f;
    }
    a.L00 = L[0]; a.L10 = L[1]; a.L11 = L[2];
    a.sr0 = R ? std::sqrt(R[0]) : 0.0f; a.sr1 = R ? std::sqrt(R[3]) : 0.0f;
}

// the records of a launch's nq traced steps, from the scratch into the ring's slots next, next + 1, ...
int ens_trace_launch(slamgpu_ekf_ens *e, int nq, const EnsTapeRec *tape, int K, uint32_t tag) {
    if (nq <= 0) return 0;
    ekf_ens_trace_kernel<<<nq, kEkfBlock, 0, e->stream>>>(e->acc.p + 6 * (size_t) e->B, tape, K, tag, e->B, e->tr_rec, e->tr_rtag, (long long) e->ring.next,
                                                          e->ring.cap);
    if (int rc = ekf_launched("ekf_ens_trace_kernel")) return rc;
    e->ring.advance(nq);
    return 0;
}

struct EnsStep {
    const float *VG = nullptr, *phi = nullptr, *z = nullptr;  // sim: per member
    float V = 0, G = 0, phi_true = 0;                         // sim_noise: shared
    const float *z_true = nullptr, *Qe = nullptr;             // Qe: the filter's control noise where it differs from the drawn one
    bool draw = false;
    uint32_t step = 0, noise = 0;
};

int ens_step(slamgpu_ekf_ens *e, const EnsStep &s, const int32_t *ids, int32_t nz, const float Q[4], const float Re[4], const float R[4], float dt,
             int32_t observe, const float *truth) {
    if (!Q) return fail(SLAMGPU_ERR_INVALID, "null Q");
    const bool known = e->cfg.association_known != 0;
    if (!observe) nz = 0;
    if (nz < 0 || nz > kMaxNz) return fail(SLAMGPU_ERR_INVALID, "nz %d outside [0, %d]", nz, kMaxNz);
    if (observe && (!Re || !R || (nz > 0 && (!(s.draw ? s.z_true : s.z) || (known && !ids))))) return fail(SLAMGPU_ERR_INVALID, "bad observation arguments");
    if (!s.draw && (!s.VG || !s.phi)) return fail(SLAMGPU_ERR_INVALID, "null VG or phi");
    if (observe && known)
        if (int rc = ens_check_ids(e->table, ids, nz)) return rc;
    float L[3];
    if (int rc = ens_check_noise(Q, s.draw, s.noise, L)) return rc;
    const size_t B = (size_t) e->B;
    const size_t bytes = sizeof(float) * (s.draw ? 3 * (size_t) nz : 3 * (size_t) nz + 3 * B + 2 * B * (size_t) nz);
    const bool traced = e->ring.cap > 0 && truth;  // (one record always fits: the capacity is at least 1)
    EnsNeeds needs;
    needs.nz = nz;
    needs.bytes = bytes;
    needs.nq = traced ? 1 : 0;
    if (int rc = ens_room(e, needs)) return rc;
    // the packet: lab | z_true | VG | phi | z in the layout of THIS step's nz; sim_noise sends the first two only
    const int k = e->slots.take();
    if (int rc = e->slots.wait(k)) return rc;
    char *h = e->pin.p + (size_t) k * e->slot_bytes;
    int32_t *lab = reinterpret_cast<int32_t *>(h);
    float *hf = reinterpret_cast<float *>(h);
    std::vector<int32_t> idn;
    bool refuse = false;
    if (observe && known) refuse = ens_known_labels(e->table, e->nf_known, e->cfg.max_landmarks, ids, nz, lab, idn);
    else std::fill(lab, lab + nz, SLAMGPU_ASSOC_DISCARD);
    if (s.draw) {
        if (nz > 0) memcpy(hf + nz, s.z_true, 8 * (size_t) nz);
    } else {
        std::fill(hf + nz, hf + 3 * (size_t) nz, 0.0f);
        memcpy(hf + 3 * (size_t) nz, s.VG, 8 * B);
        memcpy(hf + 3 * (size_t) nz + 2 * B, s.phi, 4 * B);
        if (nz > 0) memcpy(hf + 3 * (size_t) nz + 3 * B, s.z, 8 * B * (size_t) nz);
    }
    if (bytes > 0) HIP_TRY(hipMemcpyAsync(e->io, h, bytes, hipMemcpyHostToDevice, e->stream));
    if (int rc = e->slots.record(k, e->stream)) return rc;

    EnsArgs a{};
    ens_shared_args(e, a, s.Qe ? s.Qe : Q, Re, R, L, s.draw, s.noise);
    a.st.nz = nz;
    a.st.np = ens_np(nz);
    a.st.observe = observe != 0; a.st.has_truth = truth != nullptr; a.st.refuse = refuse;
    a.st.q = traced ? 0 : -1;
    a.st.step = s.step;
    a.st.V = s.V; a.st.G = s.G; a.st.phi_true = s.phi_true; a.st.dt = dt;
    for (int q = 0; q < 3; q++) a.st.truth[q] = truth ? truth[q] : 0.0f;
    const size_t lds_bytes = sizeof(float) * ens_lds_floats(e, observe, nz, a.st.np);
    if (traced) ekf_ens_kernel<true><<<e->B, kEkfBlock, lds_bytes, e->stream>>>(a);
    else ekf_ens_kernel<false><<<e->B, kEkfBlock, lds_bytes, e->stream>>>(a);
    if (int rc = ekf_launched("ekf_ens_kernel")) return rc;
    if (traced)
        if (int rc = ens_trace_launch(e, 1, nullptr, 0, s.step)) return rc;
    e->last_nz = nz;
    if (!refuse) {  // the step is on its way: only now does the table learn the new ids
        e->table.learn(idn, e->nf_known);
        e->nf_known += (int) idn.size();
    }
    return 0;
}

// slamgpu_ens_run_noise: the whole tape is checked first, against a COPY of the id table that learns step by step as K single calls would
// teach the table; then one copy through a pinned slot, one launch (and the trace's), and only then the copy replaces the table
int ens_run(slamgpu_ekf_ens *e, const slamgpu_ens_tape_step *steps, int32_t K, const float *z_true, const int32_t *ids, int32_t total, const float Q[4],
            const float Qe[4], const float Re[4], const float R[4], uint32_t noise) {
    if (K < 0 || K > kMaxRun) return fail(SLAMGPU_ERR_INVALID, "K %d outside [0, %d]", K, kMaxRun);
    if (K == 0) return 0;
    if (!steps || !Q || total < 0) return fail(SLAMGPU_ERR_INVALID, "null steps or Q, or a negative total");
    float L[3];
    if (int rc = ens_check_noise(Q, true, noise, L)) return rc;
    const bool known = e->cfg.association_known != 0;
    struct Plan {
        int32_t nz, refuse;
        size_t off;
        std::vector<int32_t> lab;
    };
    std::vector<Plan> plan((size_t) K);
    EkfIdTable table;
    if (known) table = e->table;
    int nf_known = e->nf_known;
    size_t floats = 0, lds_floats = 4;
    int32_t nzmax = 0, nq = 0;
    for (int32_t k = 0; k < K; k++) {
        const slamgpu_ens_tape_step &t = steps[k];
        Plan &p = plan[(size_t) k];
        p.nz = t.observe ? t.nz : 0;
        if (p.nz < 0 || p.nz > kMaxNz) return fail(SLAMGPU_ERR_INVALID, "step %d of the tape: nz %d outside [0, %d]", k, p.nz, kMaxNz);
        if (t.observe && (!Re || !R)) return fail(SLAMGPU_ERR_INVALID, "step %d of the tape observes: null Re or R", k);
        if (t.first < 0 || t.first > total) return fail(SLAMGPU_ERR_INVALID, "step %d of the tape: first %d outside [0, %d]", k, t.first, total);
        if (p.nz > 0) {
            if (p.nz > total - t.first)
                return fail(SLAMGPU_ERR_INVALID, "step %d of the tape: observations [%d, %d + %d) outside [0, %d)", k, t.first, t.first, p.nz, total);
            if (!z_true || (known && !ids)) return fail(SLAMGPU_ERR_INVALID, "step %d of the tape: bad observation arguments", k);
        }
        p.refuse = 0;
        p.lab.assign((size_t) p.nz, SLAMGPU_ASSOC_DISCARD);
        if (t.observe && known) {
            if (int rc = ens_check_ids(table, ids + t.first, p.nz)) return rc;
            std::vector<int32_t> idn;
            p.refuse = ens_known_labels(table, nf_known, e->cfg.max_landmarks, ids + t.first, p.nz, p.lab.data(), idn);
            if (!p.refuse) {
                table.learn(idn, nf_known);
                nf_known += (int) idn.size();
            }
        }
        p.off = floats;
        floats += 3 * (size_t) p.nz;
        nzmax = std::max(nzmax, p.nz);
        lds_floats = std::max(lds_floats, ens_lds_floats(e, t.observe, p.nz, ens_np(p.nz)));
        nq += e->ring.cap > 0 && t.has_truth;
    }
    if (nq > e->ring.cap && e->ring.cap > 0)
        return fail(SLAMGPU_ERR_CAPACITY, "the tape has %d steps with a truth, the trace retains %d records", nq, e->ring.cap);
    const size_t B = (size_t) e->B;
    const size_t bytes = sizeof(EnsTapeRec) * (size_t) K + sizeof(float) * floats;
    EnsNeeds needs;
    needs.nz = nzmax;
    needs.bytes = needs.tape_bytes = bytes;
    needs.draw_floats = B * (3 + 2 * (size_t) nzmax);
    needs.nq = (size_t) nq;
    if (int rc = ens_room(e, needs)) return rc;
    const int slot = e->slots.take();
    if (int rc = e->slots.wait(slot)) return rc;
    char *h = e->pin.p + (size_t) slot * e->slot_bytes;
    EnsTapeRec *rec = reinterpret_cast<EnsTapeRec *>(h);
    float *pk = reinterpret_cast<float *>(h + sizeof(EnsTapeRec) * (size_t) K);
    int32_t q = 0;
    for (int32_t k = 0; k < K; k++) {
        const slamgpu_ens_tape_step &t = steps[k];
        const Plan &p = plan[(size_t) k];
        EnsTapeRec &r = rec[k];
        r.V = t.V; r.G = t.G; r.phi_true = t.phi_true; r.dt = t.dt;
        for (int c = 0; c < 3; c++) r.truth[c] = t.has_truth ? t.truth[c] : 0.0f;
        r.has_truth = t.has_truth != 0; r.observe = t.observe != 0; r.nz = p.nz; r.off = (int32_t) p.off; r.refuse = p.refuse; r.np = ens_np(p.nz);
        r.q = e->ring.cap > 0 && t.has_truth ? q++ : -1;
        r.step = t.step;
        r.pad = 0;
        if (p.nz > 0) {
            memcpy(pk + p.off, p.lab.data(), 4 * (size_t) p.nz);
            memcpy(pk + p.off + p.nz, z_true + 2 * (size_t) t.first, 8 * (size_t) p.nz);
        }
    }
    HIP_TRY(hipMemcpyAsync(e->tape, h, bytes, hipMemcpyHostToDevice, e->stream));
    if (int rc = e->slots.record(slot, e->stream)) return rc;

    EnsArgs a{};
    ens_shared_args(e, a, Qe ? Qe : Q, Re, R, L, true, noise);
    const EnsTapeRec *tape = reinterpret_cast<const EnsTapeRec *>(e->tape.p);
    const float *packet = reinterpret_cast<const float *>(e->tape.p + sizeof(EnsTapeRec) * (size_t) K);
    ekf_ens_run_kernel<<<e->B, kEkfBlock, sizeof(float) * lds_floats, e->stream>>>(a, tape, packet, e->draws, K, nzmax);
    if (int rc = ekf_launched("ekf_ens_run_kernel")) return rc;
    if (int rc = ens_trace_launch(e, nq, tape, K, 0)) return rc;
    e->last_nz = plan[(size_t) K - 1].nz;
    if (known) {  // the launch is on its way: only now does the table learn what the tape's steps taught the copy
        e->table = std::move(table);
        e->nf_known = nf_known;
    }
    return 0;
}

// slamgpu_ens_moments: how many of `items` (block pairs of the Gram matrix, row blocks of P) go through the table of per-tile partials at
// a time: at most kMomPartBytes of it, at least one.  SLAMGPU_ENS_MOMENTS_CHUNK, read at the call, forces fewer (the tests reach the
// chunked path at small sizes with it).  With the sums of the block pairs (4.4 MB at D = 1027), the outputs' staging (mean, C and Pbar in
// double: 16.9 MB at D = 1027), the flags (4 bytes a member, at most 65 535 of them) and the pivot, the workspace stays under 40 MiB
// whatever the ensemble's size
constexpr size_t kMomPartBytes = (size_t) 16 << 20;
int mom_chunk(size_t bytes_per_item, int items) {
    int fit = (int) std::max<size_t>(1, kMomPartBytes / bytes_per_item);
    if (const char *s = getenv("SLAMGPU_ENS_MOMENTS_CHUNK")) fit = std::min(fit, std::max(1, atoi(s)));
    return std::min(fit, items);
}

int ens_moments(slamgpu_ekf_ens *e, int32_t D, uint32_t exclude_status, double *mean, double *C, double *Pbar, int32_t *counted, int32_t *left_out,
                int32_t *pivot) {
    if (!mean) return fail(SLAMGPU_ERR_INVALID, "null mean");
    if (D < 3 || D > e->cap_dim || !(D & 1)) return fail(SLAMGPU_ERR_INVALID, "D %d: odd, 3 .. %d", D, e->cap_dim);
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int B = e->B, T = (B + kMomTile - 1) / kMomTile, Dp = (D + 1 + 15) / 16 * 16, nb = Dp / 16, nbp = nb * (nb + 1) / 2;
    const int bp_lo = C ? 0 : nb * (nb - 1) / 2;  // without C only the block row of the column of ones: sum d and n
    const int bp_chunk = mom_chunk(sizeof(double) * 256 * (size_t) T, nbp - bp_lo);
    const int rows = std::max(1, 512 / e->ld), nrb = (D + rows - 1) / rows;  // a row block: about 128 float4s (more workgroups, not fuller ones)
    const size_t rb_doubles = (size_t) T * rows * e->ld;
    const int rb_chunk = Pbar ? mom_chunk(sizeof(double) * rb_doubles, nrb) : 0;
    const size_t DD = (size_t) D * D;
    Layout L;  // what goes up first, in one stretch
    const auto info = L.take<int32_t>(4, 8);
    const auto mean_d = L.take<double>((size_t) D, 8), C_d = L.take<double>(C ? DD : 0, 8), P_d = L.take<double>(Pbar ? DD : 0, 8);
    const size_t up = L.total();
    const auto flag = L.take<int32_t>((size_t) B, 8);
    const auto piv = L.take<double>((size_t) Dp, 8), sums = L.take<double>(256 * (size_t) nbp, 8);
    const auto part = L.take<double>(std::max(256 * (size_t) T * bp_chunk, rb_doubles * rb_chunk), 8);
    if (int rc = e->mom.reserve(L.total(), "EKF ensemble moments workspace")) return rc;
    MomArgs m{};
    m.P = e->P; m.x = e->x; m.dim = e->dim; m.status = e->status;
    m.members = B; m.ld = e->ld; m.cap_dim = e->cap_dim; m.D = D; m.Dp = Dp; m.tiles = T; m.rows = rows;
    m.exclude = exclude_status;
    m.flag = flag.at(e->mom); m.info = info.at(e->mom);
    m.pivot = piv.at(e->mom); m.sums = sums.at(e->mom); m.part = part.at(e->mom);
    m.mean = mean_d.at(e->mom); m.C = C ? C_d.at(e->mom) : nullptr; m.Pbar = Pbar ? P_d.at(e->mom) : nullptr;
    ekf_ens_mom_select_kernel<<<(B * kMomSelLanes + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(m);
    if (int rc = ekf_launched("ekf_ens_mom_select_kernel")) return rc;
    ekf_ens_mom_pivot_kernel<<<1, kEkfBlock, 0, e->stream>>>(m);
    if (int rc = ekf_launched("ekf_ens_mom_pivot_kernel")) return rc;
    const int ldl = (Dp & 16) ? Dp : Dp + 16;
    const int sub = D + 1 <= 320 ? kMomSubMax : 4;
    const size_t lds_bytes = sizeof(double) * ((size_t) sub * ldl + Dp);  // at most 45 568 bytes (D = 319: 16 rows of 336), 42 112 at D = 1027
    for (int at = bp_lo; at < nbp; at += bp_chunk) {
        m.first = at;
        m.count = std::min(bp_chunk, nbp - at);
        const dim3 grid(T, (m.count + kMomGroup - 1) / kMomGroup);  // ((256 / SUB) NP columns cover d_ext's D + 1; NP x DEPTH about 32 registers)
        if (D + 1 <= 128) ekf_ens_mom_gram_kernel<8, 4, 16><<<grid, kEkfBlock, lds_bytes, e->stream>>>(m);
        else if (D + 1 <= 320) ekf_ens_mom_gram_kernel<20, 2, 16><<<grid, kEkfBlock, lds_bytes, e->stream>>>(m);
        else ekf_ens_mom_gram_kernel<17, 2, 4><<<grid, kEkfBlock, lds_bytes, e->stream>>>(m);
        if (int rc = ekf_launched("ekf_ens_mom_gram_kernel")) return rc;
        ekf_ens_mom_reduce_kernel<<<m.count, kEkfBlock, 0, e->stream>>>(m);
        if (int rc = ekf_launched("ekf_ens_mom_reduce_kernel")) return rc;
    }
    const int outs = D + (C ? D * (D + 1) / 2 : 0);
    ekf_ens_mom_finish_kernel<<<(outs + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(m);
    if (int rc = ekf_launched("ekf_ens_mom_finish_kernel")) return rc;
    for (int at = 0; Pbar && at < nrb; at += rb_chunk) {
        m.first = at;
        m.count = std::min(rb_chunk, nrb - at);
        ekf_ens_mom_pbar_kernel<<<dim3(m.count, T), kEkfBlock, 0, e->stream>>>(m);
        if (int rc = ekf_launched("ekf_ens_mom_pbar_kernel")) return rc;
        const int entries = std::min(m.count * rows, D - at * rows) * D;
        ekf_ens_mom_pbar_finish_kernel<<<(entries + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(m);
        if (int rc = ekf_launched("ekf_ens_mom_pbar_finish_kernel")) return rc;
    }
    std::vector<char> h(up);
    HIP_TRY(hipMemcpyAsync(h.data(), e->mom.p, up, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int32_t *hi = reinterpret_cast<const int32_t *>(h.data() + info.off);
    memcpy(mean, h.data() + mean_d.off, sizeof(double) * (size_t) D);
    if (C) memcpy(C, h.data() + C_d.off, sizeof(double) * DD);
    if (Pbar) memcpy(Pbar, h.data() + P_d.off, sizeof(double) * DD);
    if (pivot) *pivot = hi[0];
    if (counted) *counted = hi[1];
    if (left_out) *left_out = B - hi[1];
    return 0;
}

int ens_member(slamgpu_ekf_ens *e, int32_t b) {
    if (b < 0 || b >= e->B) return fail(SLAMGPU_ERR_INVALID, "member %d outside [0, %d)", b, e->B);
    return 0;
}

}  // namespace

extern "C" {

int slamgpu_ens_create(const slamgpu_ekf_ens_config *cfg, slamgpu_ekf_ens **out) {
    if (!cfg || !out) return fail(SLAMGPU_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(slamgpu_ekf_ens_config))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_ekf_ens_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(slamgpu_ekf_ens_config));
    if (cfg->members < 1 || cfg->members > 65535) return fail(SLAMGPU_ERR_INVALID, "members %d outside [1, 65535]", cfg->members);
    if (int rc = ekf_check_config(cfg, 512)) return rc;
    slamgpu_ekf_ens *e = new slamgpu_ekf_ens();
    e->cfg = *cfg;
    e->B = cfg->members;
    e->cap_dim = ekf_cap_dim(cfg->max_landmarks);
    e->ld = ekf_ld(e->cap_dim);
    e->stream.adopt(cfg->external_stream);
    if (int rc = ens_reserve(e)) {
        ens_release(e);
        return rc;
    }
    *out = e;
    return 0;
}

void slamgpu_ens_destroy(slamgpu_ekf_ens *e) {
    if (!e) return;
    (void) hipSetDevice(e->cfg.device);
    if (e->stream) (void) hipStreamSynchronize(e->stream);
    ens_release(e);
}

int slamgpu_ens_sync(slamgpu_ekf_ens *e) {
    if (int rc = ens_check(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

int slamgpu_ens_sim(slamgpu_ekf_ens *e, const float *VG, const float *phi, const float *z, const int32_t *ids, int32_t nz, const float Q[4],
                        const float Re[4], const float R[4], float dt, int32_t observe, const float *truth) {
    if (int rc = ens_check(e)) return rc;
    EnsStep s;
    s.VG = VG;
    s.phi = phi;
    s.z = z;
    s.step = UINT32_MAX;  // (no Philox word: the trace's tag of such a step)
    return ens_step(e, s, ids, nz, Q, Re, R, dt, observe, truth);
}

int slamgpu_ens_sim_noise(slamgpu_ekf_ens *e, float V, float G, float phi_true, const float *z_true, const int32_t *ids, int32_t nz, uint32_t step,
                              const float Q[4], const float Qe[4], const float Re[4], const float R[4], float dt, int32_t observe, const float *truth,
                              uint32_t noise) {
    if (int rc = ens_check(e)) return rc;
    EnsStep s;
    s.V = V;
    s.G = G;
    s.phi_true = phi_true;
    s.z_true = z_true;
    s.draw = true;
    s.step = step;
    s.noise = noise;
    s.Qe = Qe;
    return ens_step(e, s, ids, nz, Q, Re, R, dt, observe, truth);
}

int slamgpu_ens_run_noise(slamgpu_ekf_ens *e, const slamgpu_ens_tape_step *steps, int32_t K, const float *z_true, const int32_t *ids, int32_t total,
                          const float Q[4], const float Qe[4], const float Re[4], const float R[4], uint32_t noise) {
    if (int rc = ens_check(e)) return rc;
    return ens_run(e, steps, K, z_true, ids, total, Q, Qe, Re, R, noise);
}

int slamgpu_ens_trace_enable(slamgpu_ekf_ens *e, int32_t capacity) {
    if (int rc = ens_check(e)) return rc;
    if (capacity < 0 || capacity > kMaxTrace) return fail(SLAMGPU_ERR_INVALID, "trace capacity %d outside [0, %d]", capacity, kMaxTrace);
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ring.reset(0);
    e->tr_rec.release();
    e->tr_rtag.release();
    if (capacity == 0) return 0;
    if (int rc = e->tr_rec.reserve_zeroed(6 * (size_t) capacity, "EKF ensemble trace records")) return rc;
    if (int rc = e->tr_rtag.reserve_zeroed((size_t) capacity, "EKF ensemble trace tags")) return rc;
    e->ring.reset(capacity);
    return 0;
}

int slamgpu_ens_trace_info(slamgpu_ekf_ens *e, int64_t *first, int64_t *next, int32_t *capacity) {
    if (int rc = ens_check(e)) return rc;
    if (first) *first = e->ring.first;
    if (next) *next = e->ring.next;
    if (capacity) *capacity = e->ring.cap;
    return 0;
}

int slamgpu_ens_trace_fetch(slamgpu_ekf_ens *e, int64_t first, int32_t count, double *out, uint32_t *step) {
    if (int rc = ens_check(e)) return rc;
    if (!e->ring.cap) return fail(SLAMGPU_ERR_INVALID, "the trace is off (slamgpu_ens_trace_enable)");
    if (!e->ring.check(first, count))
        return fail(SLAMGPU_ERR_INVALID, "trace records [%lld, %lld) are not retained: [%lld, %lld) are", (long long) first, (long long) first + count,
                    (long long) e->ring.first, (long long) e->ring.next);
    HIP_TRY(hipStreamSynchronize(e->stream));
    const Ring::Runs r = e->ring.stretches(first, count);
    if (out && r.n0 > 0) HIP_TRY(hipMemcpy(out, e->tr_rec.p + 6 * r.at, sizeof(double) * 6 * (size_t) r.n0, hipMemcpyDeviceToHost));
    if (out && r.n1 > 0) HIP_TRY(hipMemcpy(out + 6 * r.n0, e->tr_rec.p, sizeof(double) * 6 * (size_t) r.n1, hipMemcpyDeviceToHost));
    if (step && r.n0 > 0) HIP_TRY(hipMemcpy(step, e->tr_rtag.p + r.at, sizeof(uint32_t) * (size_t) r.n0, hipMemcpyDeviceToHost));
    if (step && r.n1 > 0) HIP_TRY(hipMemcpy(step + r.n0, e->tr_rtag.p, sizeof(uint32_t) * (size_t) r.n1, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ens_last_inputs(slamgpu_ekf_ens *e, float *VG, float *phi, float *z) {
    if (int rc = ens_check(e)) return rc;
    if (e->last_nz < 0) return fail(SLAMGPU_ERR_INVALID, "no step yet");
    const size_t B = (size_t) e->B, nz = (size_t) e->last_nz;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (VG) HIP_TRY(hipMemcpy(VG, e->io.p + 3 * nz, 8 * B, hipMemcpyDeviceToHost));
    if (phi) HIP_TRY(hipMemcpy(phi, e->io.p + 3 * nz + 2 * B, 4 * B, hipMemcpyDeviceToHost));
    if (z && nz > 0) HIP_TRY(hipMemcpy(z, e->io.p + 3 * nz + 3 * B, 8 * B * nz, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ens_dims(slamgpu_ekf_ens *e, int32_t *dim_out) {
    if (int rc = ens_check(e)) return rc;
    if (!dim_out) return fail(SLAMGPU_ERR_INVALID, "null output");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(dim_out, e->dim, sizeof(int32_t) * (size_t) e->B, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ens_poses(slamgpu_ekf_ens *e, double *out) {
    if (int rc = ens_check(e)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "null output");
    ekf_ens_pose_kernel<<<(12 * e->B + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(e->P, e->x, e->ld, e->cap_dim, e->B, e->pose_dev);
    if (int rc = ekf_launched("ekf_ens_pose_kernel")) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, e->pose_dev, sizeof(double) * 12 * (size_t) e->B, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ens_state(slamgpu_ekf_ens *e, int32_t b, float *x, float *P, int32_t ld_out) {
    if (int rc = ens_check(e)) return rc;
    if (int rc = ens_member(e, b)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    int32_t dim = 0;
    HIP_TRY(hipMemcpy(&dim, e->dim.p + b, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (P && ld_out < dim) return fail(SLAMGPU_ERR_INVALID, "ld_out %d < dim %d", ld_out, dim);
    const size_t ld = (size_t) e->ld;
    if (int rc = ekf_state_out(e->x.p + b * ld, e->P.p + (size_t) b * e->cap_dim * ld, e->ld, dim, x, P, ld_out)) return rc;
    return dim;
}

int slamgpu_ens_slab(slamgpu_ekf_ens *e, int32_t b, float *x, float *P) {
    if (int rc = ens_check(e)) return rc;
    if (int rc = ens_member(e, b)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t ld = (size_t) e->ld;
    if (x) HIP_TRY(hipMemcpy(x, e->x.p + b * ld, sizeof(float) * ld, hipMemcpyDeviceToHost));
    if (P) HIP_TRY(hipMemcpy(P, e->P.p + (size_t) b * e->cap_dim * ld, sizeof(float) * ld * e->cap_dim, hipMemcpyDeviceToHost));
    return e->ld;
}

int slamgpu_ens_upload(slamgpu_ekf_ens *e, int32_t b, int32_t dim, const float *x, const float *P, int32_t ld_in) {
    if (int rc = ens_check(e)) return rc;
    if (int rc = ens_member(e, b)) return rc;
    const size_t ld = (size_t) e->ld;
    if (int rc = ekf_state_in(e->stream, e->x.p + b * ld, e->P.p + (size_t) b * e->cap_dim * ld, e->ld, e->cap_dim, dim, x, P, ld_in)) return rc;
    HIP_TRY(hipMemcpy(e->dim.p + b, &dim, sizeof(int32_t), hipMemcpyHostToDevice));
    e->nf_known = (dim - 3) / 2;
    e->table.identity(e->nf_known);
    return 0;
}

int slamgpu_ens_status(slamgpu_ekf_ens *e, int32_t *status_out) {
    if (int rc = ens_check(e)) return rc;
    if (!status_out) return fail(SLAMGPU_ERR_INVALID, "null output");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(status_out, e->status, sizeof(int32_t) * (size_t) e->B, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ens_consistency(slamgpu_ekf_ens *e, double *out) {
    if (int rc = ens_check(e)) return rc;
    if (!out) return fail(SLAMGPU_ERR_INVALID, "null output");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, e->acc, sizeof(double) * 6 * (size_t) e->B, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ens_moments(slamgpu_ekf_ens *e, int32_t D, uint32_t exclude_status, double *mean, double *C, double *Pbar, int32_t *counted,
                        int32_t *left_out, int32_t *pivot) {
    if (int rc = ens_check(e)) return rc;
    return ens_moments(e, D, exclude_status, mean, C, Pbar, counted, left_out, pivot);
}

int slamgpu_ens_consistency_reset(slamgpu_ekf_ens *e) {
    if (int rc = ens_check(e)) return rc;
    HIP_TRY(hipMemsetAsync(e->acc, 0, sizeof(double) * 6 * (size_t) e->B, e->stream));
    return 0;
}

}  // extern "C"
