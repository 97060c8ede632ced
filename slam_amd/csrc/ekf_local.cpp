// Local periods of the device EKF (include/slamgpu.h: slamgpu_ekf_local_*): the compressed EKF of Guivant and Nebot (IEEE Trans.
// Robotics and Automation 17(3), 2001) on the filter of ekf.cpp.  Between begin and end the stages run on the pose and the chosen
// features only -- the active set A0, na0 = 3 + 2 k state entries -- and what they do to the rest of the map (the passive set B) is
// carried in three small matrices and applied to P in one pass by end.  With Y = P[A0, B] as it stands at begin, every stage touches
// P[A, B] by a row transform only, P[A, B] = phi Y, so the stages run on the extended symmetric matrix and state
//
//     M = [ P_AA   phi ]      s = [ x_A   ]      at begin: phi = I (na0 x na0), psi = 0, theta = 0
//         [ phi^T -psi ]          [ theta ]
//
// whose na0 extra ("carried") entries no observation refers to, and end commits
//
//     P[A, B] = phi Y (and its mirror)      P[B, B] -= Y^T psi Y      x_B += Y^T theta      P[A, A], x_A scattered back.
//
// The same filter, not an approximation.  M's layout (ekf_handle.h: EkfLocal) keeps what lies between the active
// state and the carried entries zero, so the stages are ekf.cpp's own kernels on M, bit for bit the arithmetic of the full filter;
// this unit holds what is new: begin's gather, the carried columns of an augment, psi's float64 copy and the commit's products on the
// matrix cores.  The entries of psi are thousands of times those of Y^T psi Y (psi is information: 1 / R and 1 / sigma_phi^2 enter
// it), so the commit takes psi from a float64 copy summed from the float32 factors of every chunk (G1 G1^T) and heading update, not
// from M's float32 block, and forms Y^T (psi Y) in float64 (v_mfma_f64_16x16x4_f64), rounded once into P: with the float32 block the
// passive part of P comes out 9 to 36 times further from the float64 filter than the full device filter leaves it, with the float64
// copy 0.4 to 1.5 times (profiles/ekf_local.txt).  P[A, B] = phi Y is float32 (v_mfma_f32_32x32x2_f32).  The heading update's
// eps I is left out of the passive part: h eps for h heading updates, eight orders below float32 rounding of P.
#include "ekf_handle.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// begin: row a of the active state, gathered from row gmap[a] of P, coalesced along the row: an active column goes to M, a passive
// one to the panel Y [na0][ldY].  The lane of column 0 also sets phi's row (the identity), its mirror and x_A
__global__ void __launch_bounds__(kEkfBlock) ekf_local_gather_kernel(const float *__restrict__ P, int ldP, int dim0, const float *__restrict__ x,
                                                                      const int32_t *__restrict__ gmap, const int32_t *__restrict__ cmap,
                                                                      float *__restrict__ M, int ld, int off, float *__restrict__ xl,
                                                                      float *__restrict__ Y, int ldY) {
    const int a = blockIdx.y, c = blockIdx.x * kEkfBlock + threadIdx.x;
    if (c >= dim0) return;
    const int g = gmap[a];
    const float v = P[(size_t) g * ldP + c];
    const int l = cmap[c];
    if (l >= 0)
        M[(size_t) a * ld + l] = v;
    else
        Y[(size_t) a * ldY + (-l - 1)] = v;
    if (c == 0) {
        M[(size_t) a * ld + off + a] = 1.0f;
        M[(size_t) (off + a) * ld + a] = 1.0f;
        xl[a] = x[g];
    }
}

// augment, one feature appended at len: its rows Gv phi[pose rows] over the carried columns [off, off + nx), with their mirror
// (ekf_augment_kernel covers the columns below len)
__global__ void __launch_bounds__(kEkfBlock) ekf_local_augment_kernel(float *__restrict__ M, int ld, int len, const float *__restrict__ x, float r, float b,
                                                                       int off, int nx) {
    const EkfBearing g = ekf_bearing(x, r, b);
    const int j = blockIdx.x * kEkfBlock + threadIdx.x;
    if (j < nx) ekf_augment_column(M, ld, len, off + j, g.g02, g.g12);
}

// psi's float64 copy.  A chunk: psi += G1 G1^T, G1 = the carried rows of the chunk's W1 (k ascending; (a, c) and (c, a) are the same
// chain on commuted products).  A 32 x 32 tile of psi per workgroup, its two panels of G1 staged in LDS (read along k, as W1 is stored)
__global__ void __launch_bounds__(kEkfBlock) ekf_local_psi_chunk_kernel(const float *__restrict__ W1, int off, int na0, int n,
                                                                         const int32_t *__restrict__ flag, double *__restrict__ psi) {
    if (!flag[0]) return;
    __shared__ float Ga[32][kKMax + 1], Gc[32][kKMax + 1];
    const int tid = threadIdx.x, a0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int e = tid; e < 32 * kKMax; e += kEkfBlock) {
        const int r = e / kKMax, k = e % kKMax;
        Ga[r][k] = a0 + r < na0 && k < n ? W1[(size_t) (off + a0 + r) * kKMax + k] : 0.0f;
        Gc[r][k] = c0 + r < na0 && k < n ? W1[(size_t) (off + c0 + r) * kKMax + k] : 0.0f;
    }
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    if (c0 + tx >= na0) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int a = ty + 8 * i;
        if (a0 + a >= na0) continue;
        double acc = 0.0;
        for (int k = 0; k < n; k++) acc = acc + (double) Ga[a][k] * (double) Gc[tx][k];
        psi[(size_t) (a0 + a) * na0 + c0 + tx] += acc;
    }
}

// ... a heading update: what ekf_heading_element does to M's -psi block, negated, from the update's float32 gain w and column c:
// psi += w c^T + c w^T - w w^T S
__global__ void __launch_bounds__(kEkfBlock) ekf_local_psi_heading_kernel(EkfWork w, int off, int na0, double *__restrict__ psi) {
    const int a = blockIdx.y, c = blockIdx.x * kEkfBlock + threadIdx.x;
    if (c >= na0) return;
    const double S = w.hv[1], wa = w.Wh[off + a], ca = w.c2[off + a], wc = w.Wh[off + c], cc = w.c2[off + c];
    psi[(size_t) a * na0 + c] += (wa * cc + ca * wc) - (wa * wc) * S;
}

// The commit, T = psi Y in float64: kTRows rows of T per workgroup (Y is read once for all of them), a lane per passive column, c ascending
constexpr int kTRows = 16;
__global__ void __launch_bounds__(kEkfBlock) ekf_local_t_kernel(const double *__restrict__ psi, int na0, const float *__restrict__ Y, int ldY, int nB,
                                                                 double *__restrict__ T) {
    const int a0 = blockIdx.y * kTRows, b = blockIdx.x * kEkfBlock + threadIdx.x;
    if (b >= nB) return;
    double acc[kTRows];
#pragma unroll
    for (int r = 0; r < kTRows; r++) acc[r] = 0.0;
    for (int c = 0; c < na0; c++) {
        const double y = (double) Y[(size_t) c * ldY + b];
#pragma unroll
        for (int r = 0; r < kTRows; r++) acc[r] = acc[r] + psi[(size_t) min(a0 + r, na0 - 1) * na0 + c] * y;
    }
#pragma unroll
    for (int r = 0; r < kTRows; r++)
        if (a0 + r < na0) T[(size_t) (a0 + r) * ldY + b] = acc[r];
}

// ... P[B, B] -= Y^T T on the float64 MFMA (v_mfma_f64_16x16x4_f64), the hot path of the commit.  A 64 x 64 tile of P[B, B] per
// workgroup, 32 x 32 per wave = 2 x 2 accumulators of 4 doubles; the panels Y (converted) and T are k-major in memory and staged in
// LDS kK64 rows of k at a time, zeros beyond K and nB.  Only tiles on or below the diagonal, and in a diagonal tile only i >= j, are
// computed -- (i, j) and (j, i) are different chains here -- each element rounded ONCE into float32 and written with its mirror:
// P == P^T bit for bit.  Lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; its result register r is row
// (l >> 4) + 4 r, column l & 15 of the 16 x 16 tile
constexpr int kTile64 = 64, kK64 = 16;
__global__ void __launch_bounds__(kEkfBlock) ekf_local_bb_kernel(const float *__restrict__ Y, const double *__restrict__ T, int ldY, int K, int nB,
                                                                  float *__restrict__ P, int ldP, const int32_t *__restrict__ bidx) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    __shared__ double As[kK64][kTile64 + 2], Bs[kK64][kTile64 + 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wi = wave >> 1, wj = wave & 1, c16 = lane & 15, q = lane >> 4;
    const int I0 = bi * kTile64, J0 = bj * kTile64;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[a][b][r] = 0.0;
    for (int kc = 0; kc < K; kc += kK64) {
#pragma unroll
        for (int s = 0; s < kK64 * kTile64 / kEkfBlock; s++) {
            const int idx = tid + kEkfBlock * s, kk = idx / kTile64, c = idx % kTile64;
            const bool kin = kc + kk < K;
            As[kk][c] = kin && I0 + c < nB ? (double) Y[(size_t) (kc + kk) * ldY + I0 + c] : 0.0;
            Bs[kk][c] = kin && J0 + c < nB ? T[(size_t) (kc + kk) * ldY + J0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kK64; kk += 4) {
            const double a0 = As[kk + q][wi * 32 + c16], a1 = As[kk + q][wi * 32 + 16 + c16];
            const double b0 = Bs[kk + q][wj * 32 + c16], b1 = Bs[kk + q][wj * 32 + 16 + c16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int col = J0 + wj * 32 + b * 16 + c16;
            if (col >= nB) continue;
            const size_t gc = (size_t) bidx[col];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = I0 + wi * 32 + a * 16 + q + 4 * r;
                if (row >= nB || row < col) continue;
                const size_t gr = (size_t) bidx[row];
                const float p = (float) ((double) P[gr * ldP + gc] - acc[a][b][r]);
                P[gr * ldP + gc] = p;
                P[gc * ldP + gr] = p;
            }
        }
}

// ... and P[A, B] = phi Y with its mirror, on the exact-float32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered f32 fma chain per element)
// with ekf_syrk_kernel's tiling: a 128 x 128 tile per workgroup, 64 x 64 per wave = 2 x 2 accumulators of 16 registers.
// out(i, j) = sum_k L[k][i] R[k][j] over k < K: both panels k-major in memory (L: the carried ROWS of M, phi^T, by M's symmetry; R: Y)
// and staged in LDS kKStep rows of k at a time, zeros beyond K, nI, nJ.  Stored at P[imap[i]][jmap[j]] and mirrored
__global__ void __launch_bounds__(kEkfBlock) ekf_local_ab_kernel(const float *__restrict__ L, int ldL, const float *__restrict__ R, int ldR, int K, int nI,
                                                                  int nJ, float *__restrict__ out, int ldo, const int32_t *__restrict__ imap,
                                                                  const int32_t *__restrict__ jmap) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    __shared__ float As[kKStep][kTile + 4], Bs[kKStep][kTile + 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wi = wave >> 1, wj = wave & 1, li = lane & 31, h = lane >> 5;
    const int I0 = bi * kTile, J0 = bj * kTile;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[a][b][g] = 0.0f;
    for (int kc = 0; kc < K; kc += kKStep) {
#pragma unroll
        for (int q = 0; q < kKStep * kTile / kEkfBlock; q++) {
            const int idx = tid + kEkfBlock * q, kk = idx / kTile, c = idx % kTile;
            const bool kin = kc + kk < K;
            As[kk][c] = kin && I0 + c < nI ? L[(size_t) (kc + kk) * ldL + I0 + c] : 0.0f;
            Bs[kk][c] = kin && J0 + c < nJ ? R[(size_t) (kc + kk) * ldR + J0 + c] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kKStep; kk += 2) {
            const float a0 = As[kk + h][wi * 64 + li], a1 = As[kk + h][wi * 64 + 32 + li];
            const float b0 = Bs[kk + h][wj * 64 + li], b1 = Bs[kk + h][wj * 64 + 32 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // accumulator register g of lane (li, h): row (g & 3) + 8 (g >> 2) + 4 h, column li of its 32 x 32 tile
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int col = J0 + wj * 64 + b * 32 + li;
            if (col >= nJ) continue;
            const size_t gc = (size_t) jmap[col];
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const int row = I0 + wi * 64 + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
                if (row >= nI) continue;
                const size_t gr = (size_t) imap[row];
                out[gr * ldo + gc] = acc[a][b][g];
                out[gc * ldo + gr] = acc[a][b][g];
            }
        }
}

// the commit's x_B += Y^T theta, a lane per passive entry, a ascending
__global__ void __launch_bounds__(kEkfBlock) ekf_local_xb_kernel(const float *__restrict__ Y, int ldY, int na0, int nB, const float *__restrict__ theta,
                                                                  const int32_t *__restrict__ bidx, float *__restrict__ x) {
    const int b = blockIdx.x * kEkfBlock + threadIdx.x;
    if (b >= nB) return;
    float acc = 0.0f;
    for (int a = 0; a < na0; a++) acc = acc + Y[(size_t) a * ldY + b] * theta[a];
    x[bidx[b]] = x[bidx[b]] + acc;
}

// ... and P[A, A], x_A back to where the full filter keeps them: row blockIdx.y of the active state, a lane per column
__global__ void __launch_bounds__(kEkfBlock) ekf_local_scatter_kernel(const float *__restrict__ M, int ld, int dimA, const float *__restrict__ xl,
                                                                       const int32_t *__restrict__ gmap, float *__restrict__ P, int ldP,
                                                                       float *__restrict__ x) {
    const int i = blockIdx.y, j = blockIdx.x * kEkfBlock + threadIdx.x;
    if (j >= dimA) return;
    const size_t gi = (size_t) gmap[i];
    P[gi * ldP + gmap[j]] = M[(size_t) i * ld + j];
    if (j == 0) x[gi] = xl[i];
}

inline size_t round_up(size_t n, size_t to) { return (n + to - 1) / to * to; }

}  // namespace

EkfMat ekf_local_mat(slamgpu_ekf *e) {
    const EkfLocal &l = e->loc;
    return EkfMat{l.M, l.x, l.PHt, l.W1, l.ld, l.off + l.na0, l.k + l.n_new, l.dimA(), l.w};
}

int ekf_local_features(slamgpu_ekf *e, const int32_t *idf, int32_t m, std::vector<int32_t> &local) {
    const EkfLocal &l = e->loc;
    const int nf0 = (l.dim0 - 3) / 2;
    local.resize((size_t) m);
    for (int32_t i = 0; i < m; i++) {
        const int32_t f = idf[i];
        const int32_t at = f < 0 ? -1 : f < nf0 ? l.g2l[f] : f - nf0 < l.n_new ? l.k + (f - nf0) : -1;
        if (at < 0) return fail(SLAMGPU_ERR_INVALID, "idf[%d] = %d is not active in the open local period", i, f);
        local[i] = at;
    }
    return 0;
}

void ekf_local_labels(slamgpu_ekf *e, int32_t *labels, int32_t nz) {
    const EkfLocal &l = e->loc;
    const int nf0 = (l.dim0 - 3) / 2;
    for (int32_t i = 0; i < nz; i++)
        if (labels[i] >= 0) labels[i] = labels[i] < l.k ? l.feat[labels[i]] : nf0 + (labels[i] - l.k);
}

int ekf_local_augment_carried(slamgpu_ekf *e, float r, float b) {
    const EkfLocal &l = e->loc;
    ekf_local_augment_kernel<<<(l.na0 + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(l.M, l.ld, l.dimA(), l.x, r, b, l.off, l.na0);
    return ekf_launched("ekf_local_augment_kernel");
}

int ekf_local_chunk(slamgpu_ekf *e, int n) {
    const EkfLocal &l = e->loc;
    ekf_local_psi_chunk_kernel<<<dim3((l.na0 + 31) / 32, (l.na0 + 31) / 32), kEkfBlock, 0, e->stream>>>(l.W1, l.off, l.na0, n, e->flag, l.psi);
    return ekf_launched("ekf_local_psi_chunk_kernel");
}

int ekf_local_heading(slamgpu_ekf *e) {
    const EkfLocal &l = e->loc;
    ekf_local_psi_heading_kernel<<<dim3((l.na0 + kEkfBlock - 1) / kEkfBlock, l.na0), kEkfBlock, 0, e->stream>>>(l.w, l.off, l.na0, l.psi);
    return ekf_launched("ekf_local_psi_heading_kernel");
}

void ekf_local_release(slamgpu_ekf *e) {
    EkfLocal &l = e->loc;
    l.M.release();
    l.x.release();
    l.Y.release();
    l.T.release();
    l.psi.release();
    l.PHt.release();
    l.W1.release();
    l.cw.release();
    l.idx.release();
    l.idx_host.release();
    if (l.idx_ev) (void) hipEventDestroy(l.idx_ev);
    l.idx_ev = nullptr;
    l.open = false;
}

extern "C" {

int slamgpu_ekf_local_begin(slamgpu_ekf *e, const int32_t *features, int32_t k, int32_t max_new) {
    if (int rc = ekf_check(e)) return rc;
    EkfLocal &l = e->loc;
    if (l.open) return fail(SLAMGPU_ERR_INVALID, "a local period is already open");
    const int nf = (e->dim - 3) / 2;
    if (k < 0 || k > nf || max_new < 0 || (k > 0 && !features))
        return fail(SLAMGPU_ERR_INVALID, "bad local period: k %d (of %d features), max_new %d", k, nf, max_new);
    for (int32_t i = 0; i < k; i++)
        if (features[i] < 0 || features[i] >= nf || (i > 0 && features[i] <= features[i - 1]))
            return fail(SLAMGPU_ERR_INVALID, "features[%d] = %d: ascending, distinct, in [0, %d)", i, features[i], nf);
    const int room = std::min(max_new, e->cfg.max_landmarks - nf);  // (what max_landmarks leaves: ekf_room refuses the rest first)
    const int na0 = 3 + 2 * k, off = 3 + 2 * (k + room), nM = off + na0, ld = ekf_ld(nM), nB = e->dim - na0, ldY = ekf_ld(std::max(nB, 1));
    // grow-only buffers; M and x start a period all zero
    if (int rc = l.M.reserve((size_t) ld * nM, "EKF local matrix")) return rc;
    if (int rc = l.x.reserve((size_t) ld, "EKF local state")) return rc;
    if (int rc = l.Y.reserve((size_t) ldY * na0, "EKF local panel Y")) return rc;
    if (int rc = l.T.reserve((size_t) ldY * na0, "EKF local panel T")) return rc;
    if (int rc = l.psi.reserve((size_t) na0 * na0, "EKF local psi")) return rc;
    if (int rc = l.PHt.reserve((size_t) ld * kKMax, "EKF local P H^T")) return rc;
    if (int rc = l.W1.reserve_zeroed(round_up((size_t) nM, kTile) * kKMax, "EKF local W1")) return rc;
    if (int rc = l.cw.reserve(2 * (size_t) ld, "EKF local heading work")) return rc;
    const size_t n_idx = (size_t) off + (size_t) nB + (size_t) e->dim;
    if (int rc = l.idx.reserve(n_idx, "EKF local index maps")) return rc;
    if (int rc = l.idx_host.reserve(n_idx, "EKF local index staging")) return rc;
    if (!l.idx_ev) HIP_TRY(hipEventCreateWithFlags(&l.idx_ev, hipEventDisableTiming));
    if (l.idx_used) HIP_TRY(hipEventSynchronize(l.idx_ev));  // (the previous period's maps: taken long ago)
    int32_t *gmap = l.idx_host.p, *bidx = gmap + off, *cmap = bidx + nB;
    l.feat.assign(features, features + k);
    l.g2l.assign((size_t) nf, -1);
    for (int c = 0; c < e->dim; c++) cmap[c] = 0;
    for (int i = 0; i < 3; i++) gmap[i] = i;
    for (int32_t i = 0; i < k; i++) {
        l.g2l[features[i]] = i;
        gmap[3 + 2 * i] = 3 + 2 * features[i];
        gmap[4 + 2 * i] = 4 + 2 * features[i];
    }
    for (int i = na0; i < off; i++) gmap[i] = e->dim + (i - na0);  // features the period creates: where the full filter would put them
    for (int i = 0; i < na0; i++) cmap[gmap[i]] = i + 1;
    int nb = 0;
    for (int c = 0; c < e->dim; c++) {
        if (cmap[c] > 0) {
            cmap[c] -= 1;
        } else {
            bidx[nb] = c;
            cmap[c] = -(nb + 1);
            nb++;
        }
    }
    HIP_TRY(hipMemcpyAsync(l.idx, l.idx_host, sizeof(int32_t) * n_idx, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(l.idx_ev, e->stream));
    l.idx_used = true;
    HIP_TRY(hipMemsetAsync(l.M, 0, sizeof(float) * (size_t) ld * nM, e->stream));
    HIP_TRY(hipMemsetAsync(l.x, 0, sizeof(float) * (size_t) ld, e->stream));
    HIP_TRY(hipMemsetAsync(l.psi, 0, sizeof(double) * (size_t) na0 * na0, e->stream));
    ekf_local_gather_kernel<<<dim3((e->dim + kEkfBlock - 1) / kEkfBlock, na0), kEkfBlock, 0, e->stream>>>(e->P, e->ld, e->dim, e->x, l.idx, l.idx.p + off + nB,
                                                                                                           l.M, ld, off, l.x, l.Y, ldY);
    if (int rc = ekf_launched("ekf_local_gather_kernel")) return rc;
    l.k = k;
    l.max_new = max_new;
    l.n_new = 0;
    l.na0 = na0;
    l.off = off;
    l.ld = ld;
    l.dim0 = e->dim;
    l.nB = nB;
    l.ldY = ldY;
    l.calls = 0;
    l.w = e->w;
    l.w.c2 = l.cw.p;
    l.w.Wh = l.cw.p + ld;
    l.open = true;
    return 0;
}

int slamgpu_ekf_local_end(slamgpu_ekf *e) {
    if (int rc = ekf_check(e)) return rc;
    EkfLocal &l = e->loc;
    if (!l.open) return fail(SLAMGPU_ERR_INVALID, "no local period is open");
    const int dimA = l.dimA();
    const int32_t *gmap = l.idx.p, *bidx = l.idx.p + l.off;
    const float *carried = l.M.p + (size_t) l.off * l.ld;  // rows [off, off + na0) of M: phi^T (then the float32 -psi, not used)
    if (l.nB > 0) {
        ekf_local_t_kernel<<<dim3((l.nB + kEkfBlock - 1) / kEkfBlock, (l.na0 + kTRows - 1) / kTRows), kEkfBlock, 0, e->stream>>>(l.psi, l.na0, l.Y, l.ldY, l.nB, l.T);
        if (int rc = ekf_launched("ekf_local_t_kernel")) return rc;
        const int t64 = (l.nB + kTile64 - 1) / kTile64;
        ekf_local_bb_kernel<<<dim3(t64, t64), kEkfBlock, 0, e->stream>>>(l.Y, l.T, l.ldY, l.na0, l.nB, e->P, e->ld, bidx);
        if (int rc = ekf_launched("ekf_local_bb_kernel")) return rc;
        ekf_local_ab_kernel<<<dim3((l.nB + kTile - 1) / kTile, (dimA + kTile - 1) / kTile), kEkfBlock, 0, e->stream>>>(carried, l.ld, l.Y, l.ldY, l.na0, dimA,
                                                                                                                  l.nB, e->P, e->ld, gmap, bidx);
        if (int rc = ekf_launched("ekf_local_ab_kernel")) return rc;
        ekf_local_xb_kernel<<<(l.nB + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(l.Y, l.ldY, l.na0, l.nB, l.x.p + l.off, bidx, e->x);
        if (int rc = ekf_launched("ekf_local_xb_kernel")) return rc;
    }
    ekf_local_scatter_kernel<<<dim3((dimA + kEkfBlock - 1) / kEkfBlock, dimA), kEkfBlock, 0, e->stream>>>(l.M, l.ld, dimA, l.x, gmap, e->P, e->ld, e->x);
    if (int rc = ekf_launched("ekf_local_scatter_kernel")) return rc;
    l.open = false;
    l.commits++;
    return 0;
}

int slamgpu_ekf_local_info(slamgpu_ekf *e, int32_t out[6]) {
    if (!e || !out) return fail(SLAMGPU_ERR_INVALID, "null argument");
    const EkfLocal &l = e->loc;
    out[0] = l.open ? 1 : 0;
    out[1] = l.open ? l.k : 0;
    out[2] = l.open ? l.n_new : 0;
    out[3] = l.open ? l.max_new : 0;
    out[4] = l.open ? (int32_t) std::min<int64_t>(l.calls, INT32_MAX) : 0;
    out[5] = (int32_t) std::min<int64_t>(l.commits, INT32_MAX);
    return 0;
}

int slamgpu_ekf_lookup(slamgpu_ekf *e, const int32_t *ids, int32_t n, int32_t *features_out) {
    if (!e || n < 0 || (n > 0 && (!ids || !features_out))) return fail(SLAMGPU_ERR_INVALID, "bad lookup arguments");
    for (int32_t i = 0; i < n; i++) features_out[i] = ids[i] < 0 ? -1 : e->table.lookup(ids[i]);
    return 0;
}

}  // extern "C"
