// What the device EKF (ekf.cpp) and the EKF ensemble (ekf_ens.cpp) evaluate alike, ONCE: the stages of EKFSLAM::sim as device
// functions -- the gate of a pair, predict, the heading update, the small algebra of the batch update, augment -- operation by
// operation as the host's (slam_amd/csrc/host/ekfslam.cpp), and the host pieces both handles are made of.  The units keep what
// differs by design: how a stage is spread over lanes and workgroups, the rank update, the gain.  Both are compiled
// -ffp-contract=on: a product fuses with a sum where the SOURCE writes them in one expression, so an expression here rounds the
// same in every kernel it is inlined into.  Private to the including unit, after slamgpu_ctx.h.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kEkfBlock = 256;     // lanes of a workgroup, every kernel of both units
constexpr int kChunk = 64;         // observations per chunk of the batch update
constexpr int kKMax = 2 * kChunk;  // rows of a chunk's innovation: the K extent of the rank update

__device__ inline float ekf_trig_offset(float ang) {  // core.cpp:460-477
    const double pi = 3.14159265358979323846;
    if (((double) ang < -2 * pi) || ((double) ang > 2 * pi)) {
        const int n = (int) floor((double) ang / (2 * pi));
        ang = (float) ((double) ang - n * (2 * pi));
    }
    if ((double) ang > pi) ang = (float) ((double) ang - (2 * pi));
    if ((double) ang < -pi) ang = (float) ((double) ang + (2 * pi));
    return ang;
}

// EkfSlam::observe_model: H restricted to its five non-zero columns {0, 1, 2, fpos, fpos + 1}
__device__ inline void ekf_observe_model(const float *__restrict__ x, int idf, bool want_zp, float zp[2], float H5[10]) {
#pragma clang fp contract(off)
    const int fpos = 3 + idf * 2;
    const float dx = x[fpos] - x[0], dy = x[fpos + 1] - x[1];
    const float d2 = dx * dx + dy * dy;
    const float d = sqrtf(d2);
    const float xd = dx / d, yd = dy / d, xd2 = dx / d2, yd2 = dy / d2;
    zp[0] = d;
    zp[1] = want_zp ? atan2f(dy, dx) - x[2] : 0.0f;
    H5[0] = -xd; H5[1] = -yd; H5[2] = 0; H5[3] = xd; H5[4] = yd;
    H5[5] = yd2; H5[6] = -xd2; H5[7] = -1; H5[8] = -yd2; H5[9] = xd2;
}

// 2x2 inverse / determinant through partial-pivot LU, as the host's inverse2
__device__ inline void ekf_inverse2(const float S[4], float X[4], float *det) {
#pragma clang fp contract(off)
    const bool swap = fabsf(S[2]) > fabsf(S[0]);
    const float u00 = swap ? S[2] : S[0], u01 = swap ? S[3] : S[1];
    float l10 = swap ? S[0] : S[2];
    const float r11 = swap ? S[1] : S[3];
    if (u00 != 0.0f) l10 = l10 * (1.0f / u00);
    const float u11 = r11 - l10 * u01;
    float b00 = swap ? 0.0f : 1.0f, b01 = swap ? 1.0f : 0.0f, b10 = swap ? 1.0f : 0.0f, b11 = swap ? 0.0f : 1.0f;
    b10 -= b00 * l10;
    b11 -= b01 * l10;
    float a = 1.0f / u11;
    b10 *= a;
    b11 *= a;
    b00 -= b10 * u01;
    b01 -= b11 * u01;
    a = 1.0f / u00;
    X[0] = b00 * a;
    X[1] = b01 * a;
    X[2] = b10;
    X[3] = b11;
    *det = (swap ? -1.0f : 1.0f) * (u00 * u11);
}

__device__ __forceinline__ void ekf_load_pose_block(const float *P, int ld, float Pvv[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) Pvv[i][k] = P[(size_t) i * ld + k];
}

// ---- gates: EKFSLAM::dataAssociate (ekfslam.cpp:151-189) as EkfSlam::associate evaluates it, operation by operation ----------------

// one (observation, feature) pair: the normalised innovation squared and the normalised distance
__device__ __forceinline__ void ekf_gate_pair(const float *P, int ld, const float *x, const float Pvv[3][3], const float R[4], float z0, float z1, int j,
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

// a lane's candidate over its own features, in ascending order: the first minimum of nd among the gated pairs, else the plain minimum
// of nis
__device__ __forceinline__ void ekf_gate_keep(float &nbest, float &outer, int &jbest, float nis, float nd, int j, float gate_reject) {
    if (nis < gate_reject && nd < nbest) {
        nbest = nd;
        jbest = j;
    } else if (nis < outer) {
        outer = nis;
    }
}

// ... another lane's candidate merged into this one: between lanes the lower feature wins a tie, so the result is the first minimum of all
__device__ __forceinline__ void ekf_gate_merge(float &nbest, float &outer, int &jbest, float nb, float ob, int jb) {
    if (jb >= 0 && (jbest < 0 || nb < nbest || (nb == nbest && jb < jbest))) {
        nbest = nb;
        jbest = jb;
    }
    if (ob < outer) outer = ob;
}

__device__ __forceinline__ int32_t ekf_gate_label(float outer, int jbest, float gate_augment) {
    return jbest >= 0 ? jbest : (outer > gate_augment ? SLAMGPU_ASSOC_NEW : SLAMGPU_ASSOC_DISCARD);
}

// ---- EkfSlam::predict ---------------------------------------------------------------------------------------------------------------

struct EkfMotion {
    float s, c, vts, vtc;
};

__device__ __forceinline__ EkfMotion ekf_motion(float V, float G, float th, float dt) {
    const float s = sinf(G + th), c = cosf(G + th);
    const float vts = V * dt * s, vtc = V * dt * c;
    return EkfMotion{s, c, vts, vtc};
}

// the pose rows Gv P[0:3, j] of a column j >= 3, with their mirror
__device__ __forceinline__ void ekf_predict_column(float *P, int ld, int j, float vts, float vtc) {
    const float p0 = P[j], p1 = P[(size_t) ld + j], p2 = P[2 * (size_t) ld + j];
    const float n0 = p0 + (-vts) * p2, n1 = p1 + vtc * p2;  // Gv = [1 0 -vts; 0 1 vtc; 0 0 1]: row 2 stays
    P[j] = n0;
    P[(size_t) ld + j] = n1;
    P[(size_t) j * ld] = n0;
    P[(size_t) j * ld + 1] = n1;
}

// the 3x3 pose block Gv Pvv Gv^T + Gu Q Gu^T and the pose, from the block and the pose as they were BEFORE the step (by value: the
// caller says when they were read)
__device__ __forceinline__ void ekf_predict_pose(float *P, int ld, float *x, const float Pvv[3][3], float x0, float x1, float th, EkfMotion mo, float V,
                                                 float G, float dt, float wheel_base, const float Q[4]) {
    const float s = mo.s, c = mo.c, vts = mo.vts, vtc = mo.vtc;
    const float Gv[3][3] = {{1, 0, -vts}, {0, 1, vtc}, {0, 0, 1}};
    const float Gu[3][2] = {{dt * c, -vts}, {dt * s, vtc}, {dt * sinf(G) / wheel_base, V * dt * cosf(G) / wheel_base}};
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
            for (int q = 0; q < 2; q++) acc = acc + Gu[i][q] * Q[2 * q + k];
            U[i][k] = acc;
        }
    }
    // (the host's dense products leave (i, k) and (k, i) an ulp apart; here the lower triangle is computed and mirrored: P == P^T)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k <= i; k++) {
            float a = 0.0f, b = 0.0f;
#pragma unroll
            for (int q = 0; q < 3; q++) a = a + T[i][q] * Gv[k][q];
#pragma unroll
            for (int q = 0; q < 2; q++) b = b + U[i][q] * Gu[k][q];
            P[(size_t) i * ld + k] = a + b;
            P[(size_t) k * ld + i] = a + b;
        }
    x[0] = x0 + vtc;
    x[1] = x1 + vts;
    x[2] = ekf_trig_offset(th + V * dt * sinf(G) / wheel_base);
}

// ---- EkfSlam::observe_heading: josephUpdate (core.cpp:294-317) with H = e_2^T --------------------------------------------------------

// entry i of the gain W = P[:, 2] / S and of the column it came from
__device__ __forceinline__ void ekf_heading_gain(const float *P, int ld, int i, float Si, float *c2, float *Wh) {
    const float c = P[2 * (size_t) ld + i];  // row 2 = column 2: P is symmetric bit for bit
    c2[i] = c;
    Wh[i] = c * Si;
}

// C = I - W H differs from I in column 2 only, so C P C^T + W R W^T + eps I = P - W P[2, :] - P[:, 2] W^T + W S W^T + eps I, ONE
// element-wise pass over P (the host forms the products densely).  Entry (i, j) and (j, i) evaluate the same expression on commuted
// operands -- every product and sum rounded on its own, no contraction -- so P stays symmetric bit for bit
__device__ __forceinline__ float ekf_heading_element(float p0, float wi, float ci, float wj, float cj, float S, bool diagonal) {
    const float eps = (float) 2.2204e-16;
    const float a = __fmul_rn(wi, cj), b = __fmul_rn(ci, wj);
    const float q = __fmul_rn(__fmul_rn(wi, wj), S);
    float p = __fadd_rn(__fsub_rn(p0, __fadd_rn(a, b)), q);
    if (diagonal) p = __fadd_rn(p, eps);
    return p;
}

// ---- EkfSlam::batch_update, a chunk: the small algebra --------------------------------------------------------------------------------

// H5 of feature idf into registers; a writer also stores it and the innovation v of observation i of the chunk
__device__ __forceinline__ void ekf_innovation(const float *__restrict__ x, int idf, bool writer, float z0, float z1, int i, float H5[10], float *H5g,
                                               float *v) {
    float zp[2];
    ekf_observe_model(x, idf, writer, zp, H5);
    if (writer) {
#pragma unroll
        for (int k = 0; k < 10; k++) H5g[10 * i + k] = H5[k];
        v[2 * i] = z0 - zp[0];
        v[2 * i + 1] = ekf_trig_offset(z1 - zp[1]);
    }
}

// PHt[2i + a][r] = sum_k H5_i[a][k] P[cols_i[k]][r], k ascending as the host's mulT(P, H); p: the five ROWS of P at column r (symmetry
// makes them the columns).  PHt is stored k-major, [kKMax][ld]
__device__ __forceinline__ void ekf_pht(const float p[5], const float *h, float *__restrict__ PHt, int ld, int i, int r) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 5; k++) acc = acc + p[k] * h[5 * a + k];
        PHt[(size_t) (2 * i + a) * ld + r] = acc;
    }
}

// The innovation covariance of a chunk lives in LDS, [n][n] with a row stride np (a power of two >= n).  Rows are rotated by their
// index so that neither a walk along a row nor one down a column meets a bank twice
__device__ __forceinline__ float &ekf_at(float *A, int np, int i, int j) { return A[i * np + ((i + j) & (np - 1))]; }

// S = H PHt + R with the host's in-place symmetrisation (the factorisation reads the lower triangle: the true average; the strictly
// upper one is cleared).  idf_of(i): the feature of observation i of the chunk.  The whole workgroup
template <class F>
__device__ __forceinline__ void ekf_innov_cov(float *A, int np, int n, const float *H5, const float *PHt, int ld, const float *R, F idf_of) {
    const int tid = threadIdx.x;
    for (int e = tid; e < n * n; e += kEkfBlock) {
        const int a = e / n, b = e - a * n;
        const float *h = H5 + 10 * (a >> 1) + 5 * (a & 1);
        const size_t f = 3 + 2 * (size_t) idf_of(a >> 1);
        const float *row = PHt + (size_t) b * ld;
        float acc = 0.0f;
        acc = acc + h[0] * row[0];
        acc = acc + h[1] * row[1];
        acc = acc + h[2] * row[2];
        acc = acc + h[3] * row[f];
        acc = acc + h[4] * row[f + 1];
        ekf_at(A, np, a, b) = acc + (((a >> 1) == (b >> 1)) ? R[2 * (a & 1) + (b & 1)] : 0.0f);
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += kEkfBlock) {
        const int a = e / n, b = e - a * n;
        if (a > b) {
            ekf_at(A, np, a, b) = (ekf_at(A, np, a, b) + ekf_at(A, np, b, a)) * 0.5f;
            ekf_at(A, np, b, a) = 0.0f;
        }
    }
    __syncthreads();
}

// the host's llt_lower, L in the lower triangle.  A pivot that is not positive travels in the diagonal itself (-1), every lane reads
// it after the barrier: the verdict (true: bad pivot, A is left half done) is uniform across the workgroup
__device__ __forceinline__ bool ekf_llt_lower(float *A, int np, int n) {
    const int tid = threadIdx.x;
    for (int k = 0; k < n; k++) {
        float acc = 0.0f;
        if (tid == k) {
            float xk = ekf_at(A, np, k, k);
            if (k > 0) {
                float sq = ekf_at(A, np, k, 0) * ekf_at(A, np, k, 0);
                for (int j = 1; j < k; j++) sq = sq + ekf_at(A, np, k, j) * ekf_at(A, np, k, j);
                xk = xk - sq;
            }
            ekf_at(A, np, k, k) = xk > 0.0f ? sqrtf(xk) : -1.0f;  // (NaN fails the test too)
        } else if (tid > k && tid < n) {
            acc = ekf_at(A, np, tid, k);
            for (int j = 0; j < k; j++) acc = acc + ekf_at(A, np, tid, j) * (-1.0f * ekf_at(A, np, k, j));
        }
        __syncthreads();
        const float dk = ekf_at(A, np, k, k);
        if (dk < 0.0f) return true;
        if (tid > k && tid < n) ekf_at(A, np, tid, k) = acc * (1.0f / dk);
        __syncthreads();
    }
    return false;
}

// the host's upper_inverse and t = U^-T v.  The strictly upper triangle receives X = U^-1 (U = L^T; upper triangular itself), the
// diagonal keeps L's: X(j, j) = 1 / A(j, j).  Column j of X belongs to lane j alone, no barrier inside
__device__ __forceinline__ void ekf_upper_inverse(float *A, int np, int n, const float *v, float *t) {
    const int j = threadIdx.x;
    if (j >= n) return;
    for (int i = n - 1; i >= 0; i--) {
        if (j < i) continue;  // (X(i, j) is an exact zero there: the host multiplies and subtracts zeros)
        const float a = 1.0f / ekf_at(A, np, i, i);
        const float b = j == i ? a : ekf_at(A, np, i, j) * a;
        if (j > i) ekf_at(A, np, i, j) = b;
        for (int r = 0; r < i; r++) ekf_at(A, np, r, j) = ekf_at(A, np, r, j) - b * ekf_at(A, np, i, r);
    }
    float acc = 0.0f;
    for (int k = 0; k <= j; k++) {
        const float xkj = k == j ? 1.0f / ekf_at(A, np, j, j) : ekf_at(A, np, k, j);
        acc = acc + xkj * v[k];
    }
    t[j] = acc;
}

// ---- EkfSlam::augment, one feature appended at len: Gv = [1 0 -r s; 0 1 r c] ---------------------------------------------------------

struct EkfBearing {
    float s, c, g02, g12;
};

__device__ __forceinline__ EkfBearing ekf_bearing(const float *x, float r, float b) {
    const float s = sinf(x[2] + b), c = cosf(x[2] + b);
    const float g02 = -r * s, g12 = r * c;
    return EkfBearing{s, c, g02, g12};
}

// the two new rows and columns Gv P[0:3, j] of a column j < len
__device__ __forceinline__ void ekf_augment_column(float *P, int ld, int len, int j, float g02, float g12) {
    const float p0 = P[j], p1 = P[(size_t) ld + j], p2 = P[2 * (size_t) ld + j];
    const float d0 = p0 + g02 * p2, d1 = p1 + g12 * p2;
    P[(size_t) len * ld + j] = d0;
    P[(size_t) (len + 1) * ld + j] = d1;
    P[(size_t) j * ld + len] = d0;
    P[(size_t) j * ld + len + 1] = d1;
}

// the new feature and its 2x2 block Gv Pvv Gv^T + Gz Re Gz^T (one lane)
__device__ __forceinline__ void ekf_augment_block(float *P, int ld, int len, float *x, float r, EkfBearing g, const float Re[4]) {
    const float s = g.s, c = g.c, g02 = g.g02, g12 = g.g12;
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
            for (int q = 0; q < 3; q++) acc = acc + Gv[i][q] * P[(size_t) q * ld + k];
            T[i][k] = acc;
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 2; q++) acc = acc + Gz[i][q] * Re[2 * q + k];
            U[i][k] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int k = 0; k <= i; k++) {  // (the lower triangle, mirrored, as in the predict stage)
            float a2 = 0.0f, b2 = 0.0f;
#pragma unroll
            for (int q = 0; q < 3; q++) a2 = a2 + T[i][q] * Gv[k][q];
#pragma unroll
            for (int q = 0; q < 2; q++) b2 = b2 + U[i][q] * Gz[k][q];
            P[(size_t) (len + i) * ld + len + k] = a2 + b2;
            P[(size_t) (len + k) * ld + len + i] = a2 + b2;
        }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------

inline int ekf_launched(const char *what) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(SLAMGPU_ERR_HIP, "%s launch: %s", what, hipGetErrorString(err));
    return 0;
}

// what both configs are checked for after their struct_size (and the ensemble's members), and the device made current
template <class Cfg>
int ekf_check_config(const Cfg *cfg, int most_landmarks) {
    if (cfg->max_landmarks < 0 || cfg->max_landmarks > most_landmarks)
        return fail(SLAMGPU_ERR_INVALID, "max_landmarks %d outside [0, %d]", cfg->max_landmarks, most_landmarks);
    if (!(cfg->wheel_base > 0.0f) || !(cfg->sigma_phi >= 0.0f) || !(cfg->gate_reject >= 0.0f) || !(cfg->gate_augment >= 0.0f))
        return fail(SLAMGPU_ERR_INVALID, "wheel_base must be positive, sigma_phi and the gates non-negative");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SLAMGPU_ERR_NO_DEVICE, "no HIP device: libslamgpu has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SLAMGPU_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    return 0;
}

inline int ekf_cap_dim(int max_landmarks) { return 3 + 2 * max_landmarks; }
inline int ekf_ld(int cap_dim) { return (cap_dim + 31) / 32 * 32; }

// the handle's stream: the caller's (slamgpu_*_config.external_stream), or one of its own
struct EkfStream {
    hipStream_t s = nullptr;
    bool own = true;
    operator hipStream_t() const { return s; }
    void adopt(uint64_t external) {
        if (external) {
            s = reinterpret_cast<hipStream_t>(external);
            own = false;
        }
    }
    int create() {
        if (own) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return 0;
    }
    void release() {
        if (own && s) (void) hipStreamDestroy(s);
    }
};

// association_known: id -> feature, -1 not seen yet.  What a handle does with a step that does not fit is the handle's policy
struct EkfIdTable {
    std::vector<int32_t> map;
    int32_t lookup(int32_t id) const { return (size_t) id < map.size() ? map[id] : -1; }
    // the step's new ids, in observation order, take the features base, base + 1, ...
    void learn(const std::vector<int32_t> &idn, int32_t base) {
        for (size_t i = 0; i < idn.size(); i++) {
            if ((size_t) idn[i] >= map.size()) map.resize((size_t) idn[i] + 1, -1);
            map[idn[i]] = base + (int32_t) i;
        }
    }
    // after an upload of nf features: feature f has id f
    void identity(int nf) {
        map.assign((size_t) nf, 0);
        for (int f = 0; f < nf; f++) map[f] = f;
    }
    // after the removal of features[k] (ascending and distinct): their ids have not been seen, the others follow their features
    void remove(const int32_t *features, int32_t k) {
        for (int32_t &f : map) {
            if (f < 0) continue;
            const int32_t *at = std::lower_bound(features, features + k, f);
            f = (at != features + k && *at == f) ? -1 : f - (int32_t) (at - features);
        }
    }
};

// x[dim] and P[dim][dim] of a filter at (xd, Pd, row stride ld) to the caller's arrays, either may be null; the stream is idle
inline int ekf_state_out(const float *xd, const float *Pd, int ld, int dim, float *x, float *P, int32_t ld_out) {
    if (x) HIP_TRY(hipMemcpy(x, xd, sizeof(float) * (size_t) dim, hipMemcpyDeviceToHost));
    if (P)
        HIP_TRY(hipMemcpy2D(P, sizeof(float) * (size_t) ld_out, Pd, sizeof(float) * (size_t) ld, sizeof(float) * (size_t) dim, (size_t) dim,
                            hipMemcpyDeviceToHost));
    return 0;
}

// ... and the caller's state into the filter, checked first; waits for the stream
inline int ekf_state_in(hipStream_t stream, float *xd, float *Pd, int ld, int cap_dim, int32_t dim, const float *x, const float *P, int32_t ld_in) {
    if (dim < 3 || dim > cap_dim || ((dim - 3) & 1) || !x || !P || ld_in < dim)
        return fail(SLAMGPU_ERR_INVALID, "bad upload: dim %d (3 + 2 nf up to %d), ld_in %d", dim, cap_dim, ld_in);
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(xd, x, sizeof(float) * (size_t) dim, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy2D(Pd, sizeof(float) * (size_t) ld, P, sizeof(float) * (size_t) ld_in, sizeof(float) * (size_t) dim, (size_t) dim,
                        hipMemcpyHostToDevice));
    return 0;
}

}  // namespace
