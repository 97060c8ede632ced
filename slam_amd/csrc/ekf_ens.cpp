// EKF-SLAM ensemble on the device (include/slamgpu.h: slamgpu_ens_*): B independent filters, member-major slabs resident in
// device memory, ONE launch per EKFSLAM::sim of all of them.  Kernels and host side in one unit.  Workgroup b owns member b from
// predict to augment, __syncthreads() between the stages: no grid-wide meeting, no spin, no atomics.  The arithmetic is ekf.cpp's
// stage by stage (itself the restatement of slam_amd/csrc/host/ekfslam.cpp); where the order of a sum differs, the stage says so.
#include "slamgpu_ctx.h"
#define SLAM_KNS slam_ekf_ens
#include "device_math.h"  // philox4x32, u01, box_muller3, as they are
#include "ekf_helpers.h"

namespace {

using slam_ekf_ens::box_muller3;
using slam_ekf_ens::philox4x32;
using slam_ekf_ens::U4;
using slam_ekf_ens::u01;

constexpr int kEnsBlock = 256;
constexpr int kChunk = 64;         // observations per chunk of the batch update
constexpr int kKMax = 2 * kChunk;  // rows of a chunk's innovation
constexpr int kWork = 10 * kChunk + 2 * kKMax;  // floats of a member's small work area: H5 [kChunk][10] | v [kKMax] | t [kKMax]
constexpr int kMaxNz = 4096;
constexpr int kMaxId = 1 << 20;  // known association: ids index the host's table
constexpr double kChi2_3_95 = 7.8147;

// one step of every member, by value.  io is the step's packet in device memory: lab [nz] int32 (known association: feature or
// SLAMGPU_ASSOC_NEW per observation, shared) | z_true [nz][2] (sim_noise, shared) | VG [B][2] | phi [B] | z [B][nz][2]; the last
// three are what the members used (the host's for sim, the members' own draws for sim_noise): slamgpu_ens_last_inputs
struct EnsArgs {
    float *P;         // [B][cap_dim][ld]
    float *x;         // [B][ld]
    int32_t *dim;     // [B]
    int32_t *status;  // [B] sticky
    double *acc;      // [B][6]
    float *PHt;       // [B][kKMax][ld]: P H^T of a chunk, k-major, then W1 in its place
    float *work;      // [B][kWork]
    int32_t *iw;      // [B][4 + 3 nzcap]: m, n_new, -, - | labels | observations matched | observations new
    float *io;
    int32_t members, ld, cap_dim, max_landmarks, nz, nzcap, np;  // np: the row stride of the innovation covariance in LDS, a power of two >= 2 min(nz, kChunk)
    int32_t use_heading, batch_update, known, observe, draw, has_truth;
    int32_t refuse;  // known association: the shared table has no room for the step's new ids, so NO member applies its update or augment
    uint32_t noise, step, k0, k1;
    float V, G, phi_true, dt, wheel_base, sigma_phi, r_phi, gate_reject, gate_augment;
    float Q[4], Re[4], R[4];
    float L00, L10, L11, sr0, sr1;  // the lower Cholesky factor of Q; sqrt(R00), sqrt(R11)
    float truth[3];
};

// EKFSLAM::dataAssociate for one (observation, feature) pair as ekf_gate_kernel evaluates it, operation by operation
__device__ __forceinline__ void ens_gate_pair(const float *P, int ld, const float *x, const float Pvv[3][3], const float R[4], float z0, float z1, int j,
                                     float *nis_out, float *nd_out) {
#pragma clang fp contract(off)
    float M[5][5];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) M[a][b] = Pvv[a][b];
    float zp[2], H5[10];
    ekf_observe_model(x, j, true, zp, H5);
    const float v0 = z0 - zp[0];
    const float v1 = ekf_trig_offset(z1 - zp[1]);
    const int f = 3 + 2 * j;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int q = 0; q < 2; q++) M[a][3 + q] = M[3 + q][a] = P[(size_t) a * ld + f + q];
    M[3][3] = P[(size_t) f * ld + f];
    M[3][4] = M[4][3] = P[(size_t) f * ld + f + 1];
    M[4][4] = P[(size_t) (f + 1) * ld + f + 1];
    float HP[2][5];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 5; k++) acc = acc + H5[5 * r + k] * M[k][c];
            HP[r][c] = acc;
        }
    float S[4];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 5; k++) acc = acc + HP[r][k] * H5[5 * c + k];
            S[2 * r + c] = acc + R[2 * r + c];
        }
    float Si[4], det;
    ekf_inverse2(S, Si, &det);
    const float t0 = v0 * Si[0] + v1 * Si[2], t1 = v0 * Si[1] + v1 * Si[3];
    const float nis = t0 * v0 + t1 * v1;
    *nis_out = nis;
    *nd_out = nis + logf(det);
}

__global__ void __launch_bounds__(kEnsBlock) ekf_ens_kernel(EnsArgs a) {
    extern __shared__ float lds[];  // heading: column 2 of P and the gain, [2][ld]; update: the innovation covariance, [np][np]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ld = a.ld, nz = a.nz;
    float *P = a.P + (size_t) b * a.cap_dim * ld;
    float *x = a.x + (size_t) b * ld;
    float *PHt = a.PHt + (size_t) b * kKMax * ld;
    float *H5g = a.work + (size_t) b * kWork, *vg = H5g + 10 * kChunk, *tg = vg + kKMax;
    int32_t *cnt = a.iw + (size_t) b * (4 + 3 * (size_t) a.nzcap), *lab = cnt + 4, *mi = lab + a.nzcap, *ni = mi + a.nzcap;
    const int32_t *lab_known = reinterpret_cast<const int32_t *>(a.io);
    const float *z_true = a.io + nz;
    float *vg_in = a.io + 3 * (size_t) nz + 2 * (size_t) b;
    float *phi_in = a.io + 3 * (size_t) nz + 2 * (size_t) a.members + b;
    float *z_in = a.io + 3 * (size_t) nz + 3 * (size_t) a.members + 2 * (size_t) nz * b;
    int dim = a.dim[b];

    // ---- the member's own inputs (sim_noise): Philox stream 5, counter (member, step, 5, q) ------------------------------------
    if (a.draw) {
        if (tid == 0) {
            float V = a.V, G = a.G, phi = a.phi_true;
            if (a.noise & SLAMGPU_EKF_ENS_NOISE_CONTROL) {  // multivariate_gauss2: x + chol(Q) g
                float g0, g1, g2;
                box_muller3(philox4x32((uint32_t) b, a.step, 5u, 0u, a.k0, a.k1), g0, g1, g2);
                V = a.V + a.L00 * g0;
                G = a.G + a.L10 * g0 + a.L11 * g1;
            }
            if (a.noise & SLAMGPU_EKF_ENS_NOISE_HEADING)  // (uncentred, as the reference's unifRand(): ekfslamwrapper.cpp:81)
                phi = a.phi_true + a.sigma_phi * u01(philox4x32((uint32_t) b, a.step, 5u, 1u, a.k0, a.k1).x);
            vg_in[0] = V;
            vg_in[1] = G;
            *phi_in = phi;
        }
        for (int i = tid; i < nz; i += kEnsBlock) {
            float zr = z_true[2 * i], zb = z_true[2 * i + 1];
            if (a.noise & SLAMGPU_EKF_ENS_NOISE_SENSOR) {  // Simulator::observe
                float g0, g1, g2;
                box_muller3(philox4x32((uint32_t) b, a.step, 5u, 2u + (uint32_t) i, a.k0, a.k1), g0, g1, g2);
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
        const float s = sinf(G + th), c = cosf(G + th);
        const float vts = V * a.dt * s, vtc = V * a.dt * c;
        float Pvv[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) Pvv[i][k] = P[(size_t) i * ld + k];
        __syncthreads();
        for (int j = 3 + tid; j < dim; j += kEnsBlock) {
            const float p0 = P[j], p1 = P[(size_t) ld + j], p2 = P[2 * (size_t) ld + j];
            const float n0 = p0 + (-vts) * p2, n1 = p1 + vtc * p2;  // Gv = [1 0 -vts; 0 1 vtc; 0 0 1]: row 2 stays
            P[j] = n0;
            P[(size_t) ld + j] = n1;
            P[(size_t) j * ld] = n0;
            P[(size_t) j * ld + 1] = n1;
        }
        if (tid == 0) {
            const float Gv[3][3] = {{1, 0, -vts}, {0, 1, vtc}, {0, 0, 1}};
            const float Gu[3][2] = {{a.dt * c, -vts}, {a.dt * s, vtc}, {a.dt * sinf(G) / a.wheel_base, V * a.dt * cosf(G) / a.wheel_base}};
            float T[3][3], U[3][2];
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    float acc = 0.0f;
#pragma unroll
                    for (int q = 0; q < 3; q++) acc = acc + Gv[i][q] * Pvv[q][k];
                    T[i][k] = acc;
                }
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    float acc = 0.0f;
#pragma unroll
                    for (int q = 0; q < 2; q++) acc = acc + Gu[i][q] * a.Q[2 * q + k];
                    U[i][k] = acc;
                }
            }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int k = 0; k <= i; k++) {  // the lower triangle, mirrored, as ekf_predict_kernel does
                    float p = 0.0f, q2 = 0.0f;
#pragma unroll
                    for (int q = 0; q < 3; q++) p = p + T[i][q] * Gv[k][q];
#pragma unroll
                    for (int q = 0; q < 2; q++) q2 = q2 + U[i][q] * Gu[k][q];
                    P[(size_t) i * ld + k] = p + q2;
                    P[(size_t) k * ld + i] = p + q2;
                }
            x[0] = x0 + vtc;
            x[1] = x1 + vts;
            x[2] = ekf_trig_offset(th + V * a.dt * sinf(G) / a.wheel_base);
        }
        __syncthreads();
    }

    // ---- EkfSlam::observe_heading: the single filter's one-pass form, every product and sum rounded on its own ------------------
    if (a.use_heading) {
        float *c2 = lds, *Wh = lds + ld;
        const float S = P[2 * (size_t) ld + 2] + a.r_phi;
        const float Si = 1.0f / S;
        const float hv = ekf_trig_offset(phi - x[2]);
        for (int i = tid; i < dim; i += kEnsBlock) {
            const float c = P[2 * (size_t) ld + i];  // row 2 = column 2: P is symmetric bit for bit
            c2[i] = c;
            Wh[i] = c * Si;
        }
        __syncthreads();
        const float eps = (float) 2.2204e-16;
        for (int j = tid; j < dim; j += kEnsBlock) {
            const float wj = Wh[j], cj = c2[j];
            x[j] = x[j] + wj * hv;
            for (int i = 0; i < dim; i++) {
                const float wi = Wh[i], ci = c2[i];
                const float pa = __fmul_rn(wi, cj), pb = __fmul_rn(ci, wj);
                const float q = __fmul_rn(__fmul_rn(wi, wj), S);
                float p = __fadd_rn(__fsub_rn(P[(size_t) i * ld + j], __fadd_rn(pa, pb)), q);
                if (i == j) p = __fadd_rn(p, eps);
                P[(size_t) i * ld + j] = p;
            }
        }
        __syncthreads();
    }

    if (a.observe) {
        const int nf = (dim - 3) / 2;
        // ---- labels: the shared table's, or the gates over (observation, feature) pairs against the state as it stands --------------
        if (a.known) {
            for (int i = tid; i < nz; i += kEnsBlock) {
                const int l = lab_known[i];
                lab[i] = l >= nf ? SLAMGPU_ASSOC_DISCARD : l;  // (a member that lacks the feature ignores the observation)
            }
        } else {
            // a wave per observation, its lanes over the features; a lane keeps the first minimum of its own features and between
            // lanes the lower feature wins a tie: the first minimum of all
            const int wave = tid >> 6, lane = tid & 63;
            float Pvv[3][3];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int k = 0; k < 3; k++) Pvv[i][k] = P[(size_t) i * ld + k];
            const float inf = __builtin_huge_valf();
            for (int i = wave; i < nz; i += kEnsBlock / 64) {
                const float z0 = z_in[2 * i], z1 = z_in[2 * i + 1];
                float nbest = inf, outer = inf;
                int jbest = -1;
                for (int j = lane; j < nf; j += 64) {
                    float nis, nd;
                    ens_gate_pair(P, ld, x, Pvv, a.Re, z0, z1, j, &nis, &nd);
                    if (nis < a.gate_reject && nd < nbest) {
                        nbest = nd;
                        jbest = j;
                    } else if (nis < outer) {
                        outer = nis;
                    }
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const float nb = __shfl_xor(nbest, s, 64), ob = __shfl_xor(outer, s, 64);
                    const int jb = __shfl_xor(jbest, s, 64);
                    if (jb >= 0 && (jbest < 0 || nb < nbest || (nb == nbest && jb < jbest))) {
                        nbest = nb;
                        jbest = jb;
                    }
                    if (ob < outer) outer = ob;
                }
                if (lane == 0) lab[i] = jbest >= 0 ? jbest : (outer > a.gate_augment ? SLAMGPU_ASSOC_NEW : SLAMGPU_ASSOC_DISCARD);
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
            if (nf + nn > a.max_landmarks || a.refuse) {  // the step does not fit: neither its update nor its augment is applied
                a.status[b] |= SLAMGPU_EKF_STATUS_CAPACITY;
                m = nn = 0;
            }
            cnt[0] = a.batch_update ? m : 0;
            cnt[1] = nn;
        }
        __syncthreads();
        const int m = cnt[0], nn = cnt[1];
        const int np = a.np;
#define AT(i, j) lds[(i) * np + (((i) + (j)) & (np - 1))]  // ekf_chol_kernel's rotated rows

        // ---- EkfSlam::batch_update, chunk by chunk ----------------------------------------------------------------------------------
        for (int at = 0; at < m; at += kChunk) {
            const int mc = min(kChunk, m - at), n = 2 * mc;
            if (tid < mc) {  // H5 and the innovation of observation at + tid
                const int o = mi[at + tid];
                float zp[2], H5[10];
                ekf_observe_model(x, lab[o], true, zp, H5);
#pragma unroll
                for (int k = 0; k < 10; k++) H5g[10 * tid + k] = H5[k];
                vg[2 * tid] = z_in[2 * o] - zp[0];
                vg[2 * tid + 1] = ekf_trig_offset(z_in[2 * o + 1] - zp[1]);
            }
            __syncthreads();
            // PHt[2i + a][r] = sum_k H5_i[a][k] P[cols_i[k]][r], k ascending as the host's mulT(P, H); rows of P, coalesced along r
            for (int r = tid; r < dim; r += kEnsBlock) {
                const float p0 = P[r], p1 = P[(size_t) ld + r], p2 = P[2 * (size_t) ld + r];
                for (int i = 0; i < mc; i++) {
                    const size_t f = 3 + 2 * (size_t) lab[mi[at + i]];
                    const float p3 = P[f * ld + r], p4 = P[(f + 1) * ld + r];
                    const float *h = H5g + 10 * i;
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        float acc = 0.0f;
                        acc = acc + p0 * h[5 * q];
                        acc = acc + p1 * h[5 * q + 1];
                        acc = acc + p2 * h[5 * q + 2];
                        acc = acc + p3 * h[5 * q + 3];
                        acc = acc + p4 * h[5 * q + 4];
                        PHt[(size_t) (2 * i + q) * ld + r] = acc;
                    }
                }
            }
            __syncthreads();
            // S = H PHt + R, the host's in-place symmetrisation, llt_lower, upper_inverse and t = U^-T v: ekf_chol_kernel's, in LDS
            for (int e = tid; e < n * n; e += kEnsBlock) {
                const int ra = e / n, cb = e - ra * n;
                const float *h = H5g + 10 * (ra >> 1) + 5 * (ra & 1);
                const size_t f = 3 + 2 * (size_t) lab[mi[at + (ra >> 1)]];
                const float *row = PHt + (size_t) cb * ld;
                float acc = 0.0f;
                acc = acc + h[0] * row[0];
                acc = acc + h[1] * row[1];
                acc = acc + h[2] * row[2];
                acc = acc + h[3] * row[f];
                acc = acc + h[4] * row[f + 1];
                AT(ra, cb) = acc + (((ra >> 1) == (cb >> 1)) ? a.R[2 * (ra & 1) + (cb & 1)] : 0.0f);
            }
            __syncthreads();
            for (int e = tid; e < n * n; e += kEnsBlock) {
                const int ra = e / n, cb = e - ra * n;
                if (ra > cb) {
                    AT(ra, cb) = (AT(ra, cb) + AT(cb, ra)) * 0.5f;
                    AT(cb, ra) = 0.0f;
                }
            }
            __syncthreads();
            bool bad = false;
            for (int k = 0; k < n; k++) {
                float acc = 0.0f;
                if (tid == k) {
                    float xk = AT(k, k);
                    if (k > 0) {
                        float sq = AT(k, 0) * AT(k, 0);
                        for (int j = 1; j < k; j++) sq = sq + AT(k, j) * AT(k, j);
                        xk = xk - sq;
                    }
                    AT(k, k) = xk > 0.0f ? sqrtf(xk) : -1.0f;  // (NaN fails the test too)
                } else if (tid > k && tid < n) {
                    acc = AT(tid, k);
                    for (int j = 0; j < k; j++) acc = acc + AT(tid, j) * (-1.0f * AT(k, j));
                }
                __syncthreads();
                const float dk = AT(k, k);
                bad = dk < 0.0f;
                if (bad) break;
                if (tid > k && tid < n) AT(tid, k) = acc * (1.0f / dk);
                __syncthreads();
            }
            if (bad) {  // the chunk is skipped: neither x nor P changes (every lane read the same pivot: the branch is uniform)
                if (tid == 0) a.status[b] |= SLAMGPU_EKF_STATUS_NOT_PD;
                __syncthreads();
                continue;
            }
            if (tid < n) {  // upper_inverse: column j of X = U^-1 belongs to lane j alone; the lower triangle keeps L
                const int j = tid;
                for (int i = n - 1; i >= 0; i--) {
                    if (j < i) continue;
                    const float d = 1.0f / AT(i, i);
                    const float bj = j == i ? d : AT(i, j) * d;
                    if (j > i) AT(i, j) = bj;
                    for (int r = 0; r < i; r++) AT(r, j) = AT(r, j) - bj * AT(i, r);
                }
                float acc = 0.0f;
                for (int k = 0; k <= j; k++) {
                    const float xkj = k == j ? 1.0f / AT(j, j) : AT(k, j);
                    acc = acc + xkj * vg[k];
                }
                tg[j] = acc;
            }
            __syncthreads();
            if (tid < n) AT(tid, tid) = 1.0f / AT(tid, tid);  // the diagonal of U^-1 in its place: AT(k, c), k <= c, is now X(k, c)
            __syncthreads();
            // W1 = PHt U^-1 (k ascending, as the host's mul) IN PLACE of PHt: column c needs the columns k <= c only, so c runs
            // downwards; and x += W1 t (the host forms W = W1 U^-T and W v: the same sum, associated the other way)
            for (int r = tid; r < dim; r += kEnsBlock) {
                float xacc = 0.0f;
                for (int c = n - 1; c >= 0; c--) {
                    float acc = 0.0f;
                    for (int k = 0; k <= c; k++) acc = acc + PHt[(size_t) k * ld + r] * AT(k, c);
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
                for (int i0 = 4 * wave; i0 < dim; i0 += 4 * (kEnsBlock / 64))
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
#undef AT

        // ---- EkfSlam::augment, one feature after another: each one's rows start from the pose rows, which the previous one left alone
        for (int q = 0; q < nn; q++) {
            const int o = ni[q], len = dim;
            const float r = z_in[2 * o], bb = z_in[2 * o + 1];
            const float s = sinf(x[2] + bb), c = cosf(x[2] + bb);
            const float g02 = -r * s, g12 = r * c;
            for (int j = tid; j < len; j += kEnsBlock) {
                const float p0 = P[j], p1 = P[(size_t) ld + j], p2 = P[2 * (size_t) ld + j];
                const float d0 = p0 + g02 * p2, d1 = p1 + g12 * p2;
                P[(size_t) len * ld + j] = d0;
                P[(size_t) (len + 1) * ld + j] = d1;
                P[(size_t) j * ld + len] = d0;
                P[(size_t) j * ld + len + 1] = d1;
            }
            if (tid == 0) {
                x[len] = x[0] + r * c;
                x[len + 1] = x[1] + r * s;
                const float Gv[2][3] = {{1, 0, g02}, {0, 1, g12}};
                const float Gz[2][2] = {{c, g02}, {s, g12}};
                float T[2][3], U[2][2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        float acc = 0.0f;
#pragma unroll
                        for (int t = 0; t < 3; t++) acc = acc + Gv[i][t] * P[(size_t) t * ld + k];
                        T[i][k] = acc;
                    }
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        float acc = 0.0f;
#pragma unroll
                        for (int t = 0; t < 2; t++) acc = acc + Gz[i][t] * a.Re[2 * t + k];
                        U[i][k] = acc;
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int k = 0; k <= i; k++) {  // (the lower triangle, mirrored, as in the predict stage)
                        float a2 = 0.0f, b2 = 0.0f;
#pragma unroll
                        for (int t = 0; t < 3; t++) a2 = a2 + T[i][t] * Gv[k][t];
#pragma unroll
                        for (int t = 0; t < 2; t++) b2 = b2 + U[i][t] * Gz[k][t];
                        P[(size_t) (len + i) * ld + len + k] = a2 + b2;
                        P[(size_t) (len + k) * ld + len + i] = a2 + b2;
                    }
            }
            dim += 2;
            __syncthreads();
        }
    }

    if (tid != 0) return;
    a.dim[b] = dim;
    if (!a.has_truth) return;
    // ---- consistency: the member's own row, one lane, in double (slamhost_pose_nees's definitions), every operation rounded on its
    // own: the float64 model of the tests evaluates the same formulas in the same order
    {
#pragma clang fp contract(off)
    double *A6 = a.acc + 6 * (size_t) b;
    const double ex = (double) x[0] - (double) a.truth[0], ey = (double) x[1] - (double) a.truth[1];
    const double et = remainder((double) x[2] - (double) a.truth[2], 2.0 * 3.14159265358979323846);
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
        return;
    }
    A6[0] += 1.0;
    A6[2] += nees;
    if (nees <= kChi2_3_95) A6[3] += 1.0;
    A6[4] += ex * ex + ey * ey;
    A6[5] += et * et;
    }
}

// slamgpu_ens_poses: out[b][12] = x, y, theta, Pvv row-major
__global__ void __launch_bounds__(kEnsBlock) ekf_ens_pose_kernel(const float *__restrict__ P, const float *__restrict__ x, int ld, int cap_dim, int members,
                                                                  double *__restrict__ out) {
    const int e = blockIdx.x * kEnsBlock + threadIdx.x;
    if (e >= 12 * members) return;
    const int b = e / 12, q = e - 12 * b;
    out[e] = q < 3 ? (double) x[(size_t) b * ld + q] : (double) P[(size_t) b * cap_dim * ld + (size_t) ((q - 3) / 3) * ld + (q - 3) % 3];
}

}  // namespace

struct slamgpu_ekf_ens {
    slamgpu_ekf_ens_config cfg{};
    hipStream_t stream = nullptr;
    bool own_stream = true;
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
    std::vector<int32_t> table;  // association_known: id -> feature, -1 not seen yet (ONE table: every member has the same dimension)
    int nf_known = 0;            // ... and the features it has handed out
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
    e->pin.release();
    e->slots.release();
    if (e->own_stream && e->stream) (void) hipStreamDestroy(e->stream);
    delete e;
}

int ens_reserve(slamgpu_ekf_ens *e) {
    if (e->own_stream) HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
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

// room for a step of nz observations whose packet is `bytes` long.  A buffer that has to grow is grown with the stream idle
int ens_room(slamgpu_ekf_ens *e, int32_t nz, size_t bytes) {
    const size_t B = (size_t) e->B;
    const size_t io_floats = 3 * (size_t) nz + 3 * B + 2 * B * (size_t) nz;
    if (nz > e->nzcap || io_floats > e->io.cap || bytes > e->slot_bytes) {
        HIP_TRY(hipStreamSynchronize(e->stream));
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
inline int32_t ens_lookup(const slamgpu_ekf_ens *e, int32_t id) { return (size_t) id < e->table.size() ? e->table[id] : -1; }
bool ens_known_labels(const slamgpu_ekf_ens *e, const int32_t *ids, int32_t nz, int32_t *lab, std::vector<int32_t> &idn) {
    for (int32_t i = 0; i < nz; i++) {
        const int32_t f = ens_lookup(e, ids[i]);
        lab[i] = f >= 0 ? f : SLAMGPU_ASSOC_NEW;
        if (f < 0) idn.push_back(ids[i]);
    }
    return e->nf_known + (int) idn.size() > e->cfg.max_landmarks;
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
    if (observe && known) {
        std::vector<int32_t> unseen;
        for (int32_t i = 0; i < nz; i++) {
            if (ids[i] < 0 || ids[i] >= kMaxId) return fail(SLAMGPU_ERR_INVALID, "ids[%d] = %d outside [0, %d)", i, ids[i], kMaxId);
            if (ens_lookup(e, ids[i]) < 0) unseen.push_back(ids[i]);
        }
        std::sort(unseen.begin(), unseen.end());
        if (std::adjacent_find(unseen.begin(), unseen.end()) != unseen.end())
            return fail(SLAMGPU_ERR_INVALID, "an id not seen before appears twice in one step (it would be appended twice)");
    }
    float L00 = 0, L10 = 0, L11 = 0;
    if (s.draw && (s.noise & SLAMGPU_EKF_ENS_NOISE_CONTROL)) {  // the lower Cholesky factor of Q, once, in float
        if (!(Q[0] > 0.0f)) return fail(SLAMGPU_ERR_INVALID, "control noise: Q is not positive definite");
        L00 = std::sqrt(Q[0]);
        L10 = Q[2] / L00;
        const float d = Q[3] - L10 * L10;
        if (!(d > 0.0f)) return fail(SLAMGPU_ERR_INVALID, "control noise: Q is not positive definite");
        L11 = std::sqrt(d);
    }
    if (s.draw && (s.noise & ~7u)) return fail(SLAMGPU_ERR_INVALID, "noise flags %u", s.noise);
    const size_t B = (size_t) e->B;
    const size_t bytes = sizeof(float) * (s.draw ? 3 * (size_t) nz : 3 * (size_t) nz + 3 * B + 2 * B * (size_t) nz);
    if (int rc = ens_room(e, nz, bytes)) return rc;
    // the packet: lab | z_true | VG | phi | z in the layout of THIS step's nz; sim_noise sends the first two only
    const int k = e->slots.take();
    if (int rc = e->slots.wait(k)) return rc;
    char *h = e->pin.p + (size_t) k * e->slot_bytes;
    int32_t *lab = reinterpret_cast<int32_t *>(h);
    float *hf = reinterpret_cast<float *>(h);
    std::vector<int32_t> idn;
    bool refuse = false;
    if (observe && known) refuse = ens_known_labels(e, ids, nz, lab, idn);
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
    a.P = e->P; a.x = e->x; a.dim = e->dim; a.status = e->status; a.acc = e->acc; a.PHt = e->PHt; a.work = e->work; a.iw = e->iw; a.io = e->io;
    a.members = e->B; a.ld = e->ld; a.cap_dim = e->cap_dim; a.max_landmarks = e->cfg.max_landmarks; a.nz = nz; a.nzcap = e->nzcap;
    int np = 2;
    while (np < 2 * std::min(nz, kChunk)) np *= 2;
    a.np = np;
    a.use_heading = e->cfg.use_heading != 0; a.batch_update = e->cfg.batch_update != 0; a.known = known; a.observe = observe != 0;
    a.draw = s.draw; a.has_truth = truth != nullptr; a.refuse = refuse;
    a.noise = s.noise; a.step = s.step; a.k0 = (uint32_t) e->cfg.seed; a.k1 = (uint32_t) (e->cfg.seed >> 32);
    a.V = s.V; a.G = s.G; a.phi_true = s.phi_true; a.dt = dt; a.wheel_base = e->cfg.wheel_base; a.sigma_phi = e->cfg.sigma_phi;
    a.r_phi = (float) std::pow((double) e->cfg.sigma_phi, 2);
    a.gate_reject = e->cfg.gate_reject; a.gate_augment = e->cfg.gate_augment;
    for (int q = 0; q < 4; q++) {
        a.Q[q] = s.Qe ? s.Qe[q] : Q[q];
        a.Re[q] = Re ? Re[q] : 0.0f;
        a.R[q] = R ? R[q] : 0.0f;
    }
    a.L00 = L00; a.L10 = L10; a.L11 = L11;
    a.sr0 = R ? std::sqrt(R[0]) : 0.0f; a.sr1 = R ? std::sqrt(R[3]) : 0.0f;
    for (int q = 0; q < 3; q++) a.truth[q] = truth ? truth[q] : 0.0f;
    // LDS: the heading stage's two columns or the chunk's innovation covariance, whichever is larger (at most 64 KB: np <= 128, ld <= 1056)
    size_t lds_floats = observe && e->cfg.batch_update && nz > 0 ? (size_t) np * np : 4;
    if (e->cfg.use_heading) lds_floats = std::max(lds_floats, 2 * (size_t) e->ld);
    ekf_ens_kernel<<<e->B, kEnsBlock, sizeof(float) * lds_floats, e->stream>>>(a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(SLAMGPU_ERR_HIP, "ekf_ens_kernel launch: %s", hipGetErrorString(err));
    e->last_nz = nz;
    if (!refuse) {  // the step is on its way: only now does the table learn the new ids
        for (size_t i = 0; i < idn.size(); i++) {
            if ((size_t) idn[i] >= e->table.size()) e->table.resize((size_t) idn[i] + 1, -1);
            e->table[idn[i]] = e->nf_known + (int32_t) i;
        }
        e->nf_known += (int) idn.size();
    }
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
    if (cfg->max_landmarks < 0 || cfg->max_landmarks > 512) return fail(SLAMGPU_ERR_INVALID, "max_landmarks %d outside [0, 512]", cfg->max_landmarks);
    if (!(cfg->wheel_base > 0.0f) || !(cfg->sigma_phi >= 0.0f) || !(cfg->gate_reject >= 0.0f) || !(cfg->gate_augment >= 0.0f))
        return fail(SLAMGPU_ERR_INVALID, "wheel_base must be positive, sigma_phi and the gates non-negative");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SLAMGPU_ERR_NO_DEVICE, "no HIP device: libslamgpu has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SLAMGPU_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    slamgpu_ekf_ens *e = new slamgpu_ekf_ens();
    e->cfg = *cfg;
    e->B = cfg->members;
    e->cap_dim = 3 + 2 * cfg->max_landmarks;
    e->ld = (e->cap_dim + 31) / 32 * 32;
    if (cfg->external_stream) {
        e->stream = reinterpret_cast<hipStream_t>(cfg->external_stream);
        e->own_stream = false;
    }
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
    ekf_ens_pose_kernel<<<(12 * e->B + kEnsBlock - 1) / kEnsBlock, kEnsBlock, 0, e->stream>>>(e->P, e->x, e->ld, e->cap_dim, e->B, e->pose_dev);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(SLAMGPU_ERR_HIP, "ekf_ens_pose_kernel launch: %s", hipGetErrorString(err));
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
    if (x) HIP_TRY(hipMemcpy(x, e->x.p + b * ld, sizeof(float) * (size_t) dim, hipMemcpyDeviceToHost));
    if (P)
        HIP_TRY(hipMemcpy2D(P, sizeof(float) * (size_t) ld_out, e->P.p + (size_t) b * e->cap_dim * ld, sizeof(float) * ld, sizeof(float) * (size_t) dim,
                            (size_t) dim, hipMemcpyDeviceToHost));
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
    if (dim < 3 || dim > e->cap_dim || ((dim - 3) & 1) || !x || !P || ld_in < dim)
        return fail(SLAMGPU_ERR_INVALID, "bad upload: dim %d (3 + 2 nf up to %d), ld_in %d", dim, e->cap_dim, ld_in);
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t ld = (size_t) e->ld;
    HIP_TRY(hipMemcpy(e->x.p + b * ld, x, sizeof(float) * (size_t) dim, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy2D(e->P.p + (size_t) b * e->cap_dim * ld, sizeof(float) * ld, P, sizeof(float) * (size_t) ld_in, sizeof(float) * (size_t) dim,
                        (size_t) dim, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->dim.p + b, &dim, sizeof(int32_t), hipMemcpyHostToDevice));
    e->nf_known = (dim - 3) / 2;
    e->table.assign((size_t) e->nf_known, 0);
    for (int f = 0; f < e->nf_known; f++) e->table[f] = f;
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

int slamgpu_ens_consistency_reset(slamgpu_ekf_ens *e) {
    if (int rc = ens_check(e)) return rc;
    HIP_TRY(hipMemsetAsync(e->acc, 0, sizeof(double) * 6 * (size_t) e->B, e->stream));
    return 0;
}

}  // extern "C"
