// EKF-SLAM on the device (include/slamgpu.h: slamgpu_ekf_*): one joint filter, x and the dense P resident in device memory.
// Kernels and host side in one unit; the stages' arithmetic is in ekf_helpers.h, shared with the ensemble.  It restates host/ekfslam.cpp
// (itself the restatement of matzipan/slam algorithms/ekfslam.cpp:17-323 and core.cpp:275-317) stage by stage; where the order of a sum
// or the form of an update differs from the host's, the stage says so.  The host tracks dim (it knows the labels): none on the device.
// While a local period is open (ekf_local.cpp; the handle both units share: ekf_handle.h) the same kernels run on the period's
// extended matrix: the host functions below take what they work on from ekf_mat().
#include "ekf_handle.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // (one 16-byte access in the IR: a float4 is four floats there, and their stores get regrouped)

// a chunk of the batch update, by value
struct EkfObs {
    float z[2 * kChunk];
    int32_t idf[kChunk];
    float R[4];
    int32_t m;
};

// (the arithmetic of every stage but the gain and the rank update: ekf_helpers.h, shared with the ensemble)

// EkfSlam::predict.  One lane per column j >= 3; the workgroup that finishes last (a ticket) then writes the 3x3 pose block and the
// pose, which every workgroup has read by then
__global__ void __launch_bounds__(kEkfBlock) ekf_predict_kernel(float *__restrict__ P, int ld, int dim, float *__restrict__ x, float V, float G,
                                                                 float q00, float q01, float q10, float q11, float dt, float wheel_base,
                                                                 int32_t *ticket) {
    const float th = x[2];
    const EkfMotion mo = ekf_motion(V, G, th, dt);
    const int j = 3 + blockIdx.x * kEkfBlock + threadIdx.x;
    if (j < dim) ekf_predict_column(P, ld, j, mo.vts, mo.vtc);
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(ticket, 1) == (int) gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    *ticket = 0;
    const float Q[4] = {q00, q01, q10, q11};
    float Pvv[3][3];
    ekf_load_pose_block(P, ld, Pvv);
    ekf_predict_pose(P, ld, x, Pvv, x[0], x[1], th, mo, V, G, dt, wheel_base, Q);
}

// EkfSlam::observe_heading, first half: the gain W = P[:, 2] / (P22 + R), the column it came from and the innovation.  P and x stay
__global__ void __launch_bounds__(kEkfBlock) ekf_heading_gain_kernel(const float *__restrict__ P, int ld, int dim, const float *__restrict__ x,
                                                                      float phi, float R, EkfWork w) {
    const float S = P[2 * (size_t) ld + 2] + R;
    const float Si = 1.0f / S;
    const int i = blockIdx.x * kEkfBlock + threadIdx.x;
    if (i < dim) ekf_heading_gain(P, ld, i, Si, w.c2, w.Wh);
    if (i == 0) {
        w.hv[0] = ekf_trig_offset(phi - x[2]);
        w.hv[1] = S;
    }
}

// ... second half: the one-pass Joseph update of ekf_heading_element, a lane per column and gridDim.y rows at a time.  The workgroups
// of the first row also apply x += W v
__global__ void __launch_bounds__(kEkfBlock) ekf_heading_kernel(float *__restrict__ P, int ld, int dim, float *__restrict__ x, EkfWork w) {
    const int j = blockIdx.x * kEkfBlock + threadIdx.x;
    if (j >= dim) return;
    const float S = w.hv[1];
    const float wj = w.Wh[j], cj = w.c2[j];
    if (blockIdx.y == 0) x[j] = x[j] + wj * w.hv[0];
    for (int i = blockIdx.y; i < dim; i += gridDim.y)
        P[(size_t) i * ld + j] = ekf_heading_element(P[(size_t) i * ld + j], w.Wh[i], w.c2[i], wj, cj, S, i == j);
}

// The gates: one workgroup per observation, its lanes over the features, the lanes' candidates merged through LDS
__global__ void __launch_bounds__(kEkfBlock) ekf_gate_kernel(const float *__restrict__ P, int ld, int nf, const float *__restrict__ x,
                                                              const float *__restrict__ z, float r00, float r01, float r10, float r11,
                                                              float gate_reject, float gate_augment, int32_t *__restrict__ labels) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const float z0 = z[2 * i], z1 = z[2 * i + 1];
    const float R[4] = {r00, r01, r10, r11};
    float Pvv[3][3];
    ekf_load_pose_block(P, ld, Pvv);
    const float inf = __builtin_huge_valf();
    float nbest = inf, outer = inf;
    int jbest = -1;
    for (int j = tid; j < nf; j += kEkfBlock) {
        float nis, nd;
        ekf_gate_pair(P, ld, x, Pvv, R, z0, z1, j, &nis, &nd);
        ekf_gate_keep(nbest, outer, jbest, nis, nd, j, gate_reject);
    }
    __shared__ float s_nd[kEkfBlock], s_out[kEkfBlock];
    __shared__ int s_j[kEkfBlock];
    s_nd[tid] = nbest;
    s_out[tid] = outer;
    s_j[tid] = jbest;
    __syncthreads();
    for (int step = kEkfBlock / 2; step > 0; step >>= 1) {
        if (tid < step) ekf_gate_merge(s_nd[tid], s_out[tid], s_j[tid], s_nd[tid + step], s_out[tid + step], s_j[tid + step]);
        __syncthreads();
    }
    if (tid == 0) labels[i] = ekf_gate_label(s_out[0], s_j[0], gate_augment);
}

// EkfSlam::batch_update, a chunk: H5, the innovation v (workgroup column 0) and P H^T, observation blockIdx.y at the state rows of
// the workgroup's lanes.  Five ROWS of P per observation, coalesced along r
__global__ void __launch_bounds__(kEkfBlock) ekf_innov_kernel(const float *__restrict__ P, int ld, int dim, const float *__restrict__ x, EkfObs O,
                                                               float *__restrict__ PHt, EkfWork w) {
    const int i = blockIdx.y, r = blockIdx.x * kEkfBlock + threadIdx.x;
    const int idf = O.idf[i];
    float H5[10];
    ekf_innovation(x, idf, blockIdx.x == 0 && threadIdx.x == 0, O.z[2 * i], O.z[2 * i + 1], i, H5, w.H5, w.v);
    if (r >= dim) return;
    const size_t f = 3 + 2 * (size_t) idf;
    const float p[5] = {P[r], P[(size_t) ld + r], P[2 * (size_t) ld + r], P[f * ld + r], P[(f + 1) * ld + r]};
    ekf_pht(p, H5, PHt, ld, i, r);
}

// ... the innovation covariance, its factorisation, the inverse of the upper factor and t = U^-T v in ONE workgroup with S in LDS
// (ekf_helpers.h), then U^-1 copied out for ekf_gain_kernel.  A pivot that is not positive: flag[0] = 0 -- the chunk's gain and rank
// update do nothing -- and SLAMGPU_EKF_STATUS_NOT_PD
__global__ void __launch_bounds__(kEkfBlock) ekf_chol_kernel(const float *__restrict__ PHt, int ld, EkfObs O, EkfWork w) {
    __shared__ float A[kKMax * kKMax];  // (all of the 64 KB a workgroup may declare: the pivot's verdict travels in the diagonal itself)
    const int tid = threadIdx.x, n = 2 * O.m;
    ekf_innov_cov(A, kKMax, n, w.H5, PHt, ld, O.R, [&](int i) { return O.idf[i]; });
    if (ekf_llt_lower(A, kKMax, n)) {
        if (tid == 0) {
            w.flag[0] = 0;
            atomicOr(&w.flag[1], SLAMGPU_EKF_STATUS_NOT_PD);
        }
        return;
    }
    ekf_upper_inverse(A, kKMax, n, w.v, w.t);
    if (tid < n) {  // (column tid is the lane's own: no barrier)
        for (int k = 0; k < tid; k++) w.Ui[k * kKMax + tid] = ekf_at(A, kKMax, k, tid);
        w.Ui[tid * kKMax + tid] = 1.0f / ekf_at(A, kKMax, tid, tid);
        for (int k = tid + 1; k < n; k++) w.Ui[k * kKMax + tid] = 0.0f;
    }
    if (tid == 0) w.flag[0] = 1;
}

// ... W1 = PHt U^-1 (k ascending, as the host's mul) and x += W1 t (the host forms W = W1 U^-T and W v: the same sum, associated
// the other way).  32 state rows per workgroup; W1 is stored [rows][kKMax], zero in columns n .. npad - 1
__global__ void __launch_bounds__(kEkfBlock) ekf_gain_kernel(const float *__restrict__ PHt, int ld, int dim, float *__restrict__ x, int n, int npad,
                                                              float *__restrict__ W1, EkfWork w) {
    if (!w.flag[0]) return;
    __shared__ float Ps[kKMax][32];
    __shared__ float Ws[32][kKMax + 1];
    const int tid = threadIdx.x, lr = tid & 31, q = tid >> 5;
    const int r0 = blockIdx.x * 32, r = r0 + lr;
    for (int k = q; k < n; k += 8) Ps[k][lr] = r < dim ? PHt[(size_t) k * ld + r] : 0.0f;
    __syncthreads();
    for (int c = q; c < npad; c += 8) {
        float acc = 0.0f;
        if (c < n)
            for (int k = 0; k <= c; k++) acc = acc + Ps[k][lr] * w.Ui[k * kKMax + c];
        Ws[lr][c] = acc;
    }
    __syncthreads();
    for (int e = tid; e < 32 * npad; e += kEkfBlock) {
        const int row = e / npad, c = e - row * npad;
        if (r0 + row < dim) W1[(size_t) (r0 + row) * kKMax + c] = Ws[row][c];
    }
    if (q == 0 && r < dim) {
        float acc = 0.0f;
        for (int c = 0; c < n; c++) acc = acc + Ws[lr][c] * w.t[c];
        x[r] = x[r] + acc;
    }
}

// ... P -= W1 W1^T on the exact-float32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered f32 fma chain per element).  A 128 x 128 tile of P
// per workgroup, 64 x 64 per wave = 2 x 2 accumulators of 16 registers; the two W1 panels are staged in LDS kKStep k columns at a
// time, k-major, so that a lane's operand is one conflict-free read.  Only tiles on or below the diagonal are computed; an
// off-diagonal tile is written twice, the second time transposed, and inside a diagonal tile (i, j) and (j, i) are the same chain
// on commuted products: P == P^T bit for bit.  Rows and columns >= dim of P are neither read nor written; W1's rows there
// (allocated, never data) only reach accumulators that are not stored
__global__ void __launch_bounds__(kEkfBlock) ekf_syrk_kernel(float *__restrict__ P, int ld, int dim, const float *__restrict__ W1, int npad,
                                                              const int32_t *__restrict__ flag) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi || !flag[0]) return;
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
    for (int kc = 0; kc < npad; kc += kKStep) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int idx = tid + kEkfBlock * q, row = idx >> 3, k4 = (idx & 7) * 4;
            const float4 a = *reinterpret_cast<const float4 *>(W1 + (size_t) (I0 + row) * kKMax + kc + k4);
            const float4 b = *reinterpret_cast<const float4 *>(W1 + (size_t) (J0 + row) * kKMax + kc + k4);
            As[k4][row] = a.x; As[k4 + 1][row] = a.y; As[k4 + 2][row] = a.z; As[k4 + 3][row] = a.w;
            Bs[k4][row] = b.x; Bs[k4 + 1][row] = b.y; Bs[k4 + 2][row] = b.z; Bs[k4 + 3][row] = b.w;
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
            if (col >= dim) continue;
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const int row0 = I0 + wi * 64 + a * 32 + 8 * g4 + 4 * h;
                float p[4];
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (row0 + e < dim) {
                        p[e] = P[(size_t) (row0 + e) * ld + col] - acc[a][b][4 * g4 + e];
                        P[(size_t) (row0 + e) * ld + col] = p[e];
                    }
                if (bi == bj) continue;
                if (row0 + 3 < dim) {
                    *reinterpret_cast<float4 *>(P + (size_t) col * ld + row0) = make_float4(p[0], p[1], p[2], p[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (row0 + e < dim) P[(size_t) col * ld + row0 + e] = p[e];
                }
            }
        }
}

// EkfSlam::augment, one feature appended at len: a lane per column, lane 0 of the grid the 2x2 block and the feature itself
__global__ void __launch_bounds__(kEkfBlock) ekf_augment_kernel(float *__restrict__ P, int ld, int len, float *__restrict__ x, float r, float b,
                                                                 float re00, float re01, float re10, float re11) {
    const EkfBearing g = ekf_bearing(x, r, b);
    const int j = blockIdx.x * kEkfBlock + threadIdx.x;
    if (j < len) ekf_augment_column(P, ld, len, j, g.g02, g.g12);
    if (j != 0) return;
    const float Re[4] = {re00, re01, re10, re11};
    ekf_augment_block(P, ld, len, x, r, g, Re);
}

// slamgpu_ekf_block: out[a][b] = P[idx[a]][idx[b]]
__global__ void __launch_bounds__(kEkfBlock) ekf_block_kernel(const float *__restrict__ P, int ld, const int32_t *__restrict__ idx, int k,
                                                               float *__restrict__ out) {
    const size_t e = (size_t) blockIdx.x * kEkfBlock + threadIdx.x;
    if (e >= (size_t) k * k) return;
    const int a = (int) (e / k), b = (int) (e - (size_t) a * k);
    out[e] = P[(size_t) idx[a] * ld + idx[b]];
}

// slamgpu_ekf_remove: P'[i][j] = P[src[max(i, j)]][src[min(i, j)]] IN PLACE, n = dim' rows, nothing below s0 moves.  Two transposing
// copies of kRmTile x kRmTile tiles through LDS, the second launched after the first:
//   gather: reads the strict LOWER triangle of the old P, writes the strict UPPER triangle of the new one at columns >= s0
//   mirror: reads that upper triangle, writes the strict lower triangle at rows >= s0
// In both the entries read and the entries written are disjoint sets, so the workgroups of a launch need no order among themselves.
// The diagonal and x, which would be read and written in the same triangle, wait in the heading update's scratch vectors in between.
constexpr int kRmTile = 64;

// a lane's place in a tile pass: four consecutive columns c, c + 1, c + 2, c + 3 of row r0 (+ 16 per pass).  A 32-lane half holds 8
// quads x 4 rows, so that with the row stride kRmTile + 1 its 32 reads t[c + e][r] (bank c + e + r mod 32) and its 32 writes
// t[r][c + e] (bank r + c + e mod 32) each fall on 32 different banks
struct RmLane {
    int c, r0;
    __device__ explicit RmLane(int tid) : c(4 * ((tid & 7) + 8 * ((tid >> 5) & 1))), r0(((tid & 31) >> 3) + 4 * (tid >> 6)) {}
};

// the entries of the new P a phase writes: the gather (i, j) with i < j and s0 <= j < n, the mirror (i, j) with j < i and s0 <= i < n
template <bool kUpper>
__device__ inline bool rm_writes(int i, int j, int s0, int n) {
    return kUpper ? (i < j && j >= s0 && j < n) : (j < i && i >= s0 && i < n);
}

// ... and the tiles every entry of which is one: strictly off the diagonal and wholly inside [s0, n) on the side that counts.  Their
// workgroups take the paths without a test, where all of a lane's loads are in flight together
template <bool kUpper>
__device__ inline bool rm_full_tile(int bi, int bj, int s0, int n) {
    const int b = kUpper ? bj : bi;
    return bi != bj && b * kRmTile >= s0 && (b + 1) * kRmTile <= n;
}

// the tile in LDS, t[a][b] = what belongs at row I0 + b, column J0 + a, out to P along its rows: 16 bytes per lane where the four
// entries are all the phase's (J0 is a multiple of 4 and so is ld)
template <bool kUpper>
__device__ inline void rm_store_tile(float *__restrict__ P, int ld, const float (*t)[kRmTile + 1], int I0, int J0, int s0, int n, int tid, bool full) {
    const RmLane L(tid);
    const int j = J0 + L.c;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int r = L.r0 + 16 * pass, i = I0 + r;
        const float v0 = t[L.c][r], v1 = t[L.c + 1][r], v2 = t[L.c + 2][r], v3 = t[L.c + 3][r];
        float *row = P + (size_t) i * ld + j;
        if (full || (rm_writes<kUpper>(i, j, s0, n) && rm_writes<kUpper>(i, j + 3, s0, n))) {
            *reinterpret_cast<f32x4 *>(row) = f32x4{v0, v1, v2, v3};
        } else {
            if (rm_writes<kUpper>(i, j, s0, n)) row[0] = v0;
            if (rm_writes<kUpper>(i, j + 1, s0, n)) row[1] = v1;
            if (rm_writes<kUpper>(i, j + 2, s0, n)) row[2] = v2;
            if (rm_writes<kUpper>(i, j + 3, s0, n)) row[3] = v3;
        }
    }
}

// ... the gather.  Tile (bi, bj) of the new upper triangle, column tiles from jb0 = s0 / kRmTile on: row src[j] of the old P at the
// columns src[I0 ..], a few contiguous runs, a lane per column.  The workgroups of the diagonal tiles also save the diagonal and x
__global__ void __launch_bounds__(kEkfBlock) ekf_remove_gather_kernel(float *__restrict__ P, int ld, int n, int s0, int jb0, const int32_t *__restrict__ src,
                                                                       const float *__restrict__ x, float *__restrict__ diag, float *__restrict__ xs) {
    const int bi = blockIdx.y, bj = jb0 + blockIdx.x;
    if (bi > bj) return;
    __shared__ float t[kRmTile][kRmTile + 1];
    const int tid = threadIdx.x, lane = tid & 63, I0 = bi * kRmTile, J0 = bj * kRmTile;
    const int i = I0 + lane;
    const int sc = i < n ? src[i] : 0;
    const bool full = rm_full_tile<true>(bi, bj, s0, n);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (the wave's rows src[j] are the same for its lanes: scalar loads)
    if (full) {
        float v[kRmTile / 4];
#pragma unroll
        for (int pass = 0; pass < kRmTile / 4; pass++) v[pass] = P[(size_t) src[J0 + wave + 4 * pass] * ld + sc];
#pragma unroll
        for (int pass = 0; pass < kRmTile / 4; pass++) t[wave + 4 * pass][lane] = v[pass];
    } else {
#pragma unroll
        for (int pass = 0; pass < kRmTile / 4; pass++) {
            const int a = wave + 4 * pass, j = J0 + a;
            if (rm_writes<true>(i, j, s0, n)) t[a][lane] = P[(size_t) src[j] * ld + sc];
        }
    }
    if (bi == bj && tid < kRmTile && i >= s0 && i < n) {
        diag[i] = P[(size_t) sc * ld + sc];
        xs[i] = x[sc];
    }
    __syncthreads();
    rm_store_tile<true>(P, ld, t, I0, J0, s0, n, tid, full);
}

// ... the mirror.  Tile (bi, bj) of the new lower triangle, row tiles from ib0 = s0 / kRmTile on: rows J0 .. of the upper triangle at
// the columns I0 .., 16 bytes per lane where the four entries are all the phase's.  The diagonal tiles put the diagonal and x back
__global__ void __launch_bounds__(kEkfBlock) ekf_remove_mirror_kernel(float *__restrict__ P, int ld, int n, int s0, int ib0, float *__restrict__ x,
                                                                       const float *__restrict__ diag, const float *__restrict__ xs) {
    const int bi = ib0 + blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    __shared__ float t[kRmTile][kRmTile + 1];
    const int tid = threadIdx.x, I0 = bi * kRmTile, J0 = bj * kRmTile;
    const RmLane L(tid);
    const int i = I0 + L.c;
    const bool full = rm_full_tile<false>(bi, bj, s0, n);
    if (full) {
        f32x4 v[4];
#pragma unroll
        for (int pass = 0; pass < 4; pass++) v[pass] = *reinterpret_cast<const f32x4 *>(P + (size_t) (J0 + L.r0 + 16 * pass) * ld + i);
#pragma unroll
        for (int pass = 0; pass < 4; pass++) {
            float *at = &t[L.r0 + 16 * pass][L.c];
            at[0] = v[pass].x;
            at[1] = v[pass].y;
            at[2] = v[pass].z;
            at[3] = v[pass].w;
        }
    }
#pragma unroll
    for (int pass = 0; pass < 4 && !full; pass++) {
        const int a = L.r0 + 16 * pass, j = J0 + a;
        const float *row = P + (size_t) j * ld + i;
        if (rm_writes<false>(i, j, s0, n) && i + 3 < n) {  // (i > j and i >= s0: so are i + 1 .. i + 3)
            const f32x4 v = *reinterpret_cast<const f32x4 *>(row);
            t[a][L.c] = v.x;
            t[a][L.c + 1] = v.y;
            t[a][L.c + 2] = v.z;
            t[a][L.c + 3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (rm_writes<false>(i + e, j, s0, n)) t[a][L.c + e] = row[e];
        }
    }
    __syncthreads();
    // t[a][b]: row I0 + b, column J0 + a of the lower triangle
    rm_store_tile<false>(P, ld, t, I0, J0, s0, n, tid, full);
    const int d = I0 + tid;
    if (bi == bj && tid < kRmTile && d >= s0 && d < n) {
        P[(size_t) d * ld + d] = diag[d];
        x[d] = xs[d];
    }
}

// ... the vacated strip: rows [n, dim) over the columns [0, dim), columns [n, dim) of the rows [0, n), and x[n, dim)
__global__ void __launch_bounds__(kEkfBlock) ekf_remove_zero_kernel(float *__restrict__ P, int ld, int n, int dim, float *__restrict__ x) {
    const size_t g = (size_t) blockIdx.x * kEkfBlock + threadIdx.x;
    const size_t w = (size_t) (dim - n), below = w * (size_t) dim;
    if (g < w) x[n + g] = 0.0f;
    if (g < below) {
        P[(n + g / dim) * ld + g % dim] = 0.0f;
    } else if (g - below < w * (size_t) n) {
        const size_t q = g - below;
        P[(q / w) * ld + n + q % w] = 0.0f;
    }
}

}  // namespace

int ekf_check(slamgpu_ekf *e) {
    if (!e) return fail(SLAMGPU_ERR_INVALID, "null EKF handle");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return 0;
}

namespace {

inline int nf_of(const slamgpu_ekf *e) { return (e->dim - 3) / 2; }

// what the stages work on: P and x, or an open local period's extended matrix
inline EkfMat ekf_mat(slamgpu_ekf *e) {
    if (e->loc.open) return ekf_local_mat(e);
    return EkfMat{e->P, e->x, e->PHt, e->W1, e->ld, e->dim, nf_of(e), e->dim, e->w};
}

inline int ekf_closed(const slamgpu_ekf *e, const char *what) {
    return e->loc.open ? fail(SLAMGPU_ERR_INVALID, "%s while a local period is open (the passive part of P is stale until slamgpu_ekf_local_end)", what) : 0;
}

// a stage entry point's tail: the period counts the calls that succeeded
inline int ekf_counted(slamgpu_ekf *e, int rc) {
    if (rc == 0 && e->loc.open) e->loc.calls++;
    return rc;
}

int ekf_predict(slamgpu_ekf *e, float V, float G, const float Q[4], float dt) {
    const EkfMat m = ekf_mat(e);
    const int nb = std::max(1, (m.n - 3 + kEkfBlock - 1) / kEkfBlock);
    ekf_predict_kernel<<<nb, kEkfBlock, 0, e->stream>>>(m.P, m.ld, m.n, m.x, V, G, Q[0], Q[1], Q[2], Q[3], dt, e->cfg.wheel_base, e->flag.p + 2);
    return ekf_launched("ekf_predict_kernel");
}

int ekf_heading(slamgpu_ekf *e, float phi) {
    const EkfMat m = ekf_mat(e);
    const float R = (float) std::pow((double) e->cfg.sigma_phi, 2);
    const int nb = (m.n + kEkfBlock - 1) / kEkfBlock;
    ekf_heading_gain_kernel<<<nb, kEkfBlock, 0, e->stream>>>(m.P, m.ld, m.n, m.x, phi, R, m.w);
    if (int rc = ekf_launched("ekf_heading_gain_kernel")) return rc;
    ekf_heading_kernel<<<dim3(nb, std::min(m.n, 16384)), kEkfBlock, 0, e->stream>>>(m.P, m.ld, m.n, m.x, m.w);
    if (int rc = ekf_launched("ekf_heading_kernel")) return rc;
    return e->loc.open ? ekf_local_heading(e) : 0;
}

// labels of the gates for z[nz] against the state as it stands: one synchronisation.  In a local period the gates see the active and
// the new features; the labels go out in global indices
int ekf_associate(slamgpu_ekf *e, const float *z, int32_t nz, const float Re[4], int32_t *labels) {
    if (nz == 0) return 0;
    const EkfMat m = ekf_mat(e);
    if (int rc = e->z_dev.reserve(2 * (size_t) nz, "EKF observations")) return rc;
    if (int rc = e->lab_dev.reserve((size_t) nz, "EKF labels")) return rc;
    if (int rc = e->pin.reserve(12 * (size_t) nz, "EKF association staging")) return rc;
    float *zh = reinterpret_cast<float *>(e->pin.p);
    int32_t *lh = reinterpret_cast<int32_t *>(e->pin.p + 8 * (size_t) nz);
    memcpy(zh, z, 8 * (size_t) nz);
    HIP_TRY(hipMemcpyAsync(e->z_dev, zh, 8 * (size_t) nz, hipMemcpyHostToDevice, e->stream));
    ekf_gate_kernel<<<nz, kEkfBlock, 0, e->stream>>>(m.P, m.ld, m.nf, m.x, e->z_dev, Re[0], Re[1], Re[2], Re[3], e->cfg.gate_reject,
                                                      e->cfg.gate_augment, e->lab_dev);
    if (int rc = ekf_launched("ekf_gate_kernel")) return rc;
    HIP_TRY(hipMemcpyAsync(lh, e->lab_dev, 4 * (size_t) nz, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    memcpy(labels, lh, 4 * (size_t) nz);
    if (e->loc.open) ekf_local_labels(e, labels, nz);
    return 0;
}

int ekf_update(slamgpu_ekf *e, const float *zf, const int32_t *idf, int32_t m, const float R[4]) {
    const int nf = nf_of(e);
    for (int32_t i = 0; i < m; i++)
        if (idf[i] < 0 || idf[i] >= nf) return fail(SLAMGPU_ERR_INVALID, "idf[%d] = %d outside [0, %d)", i, idf[i], nf);
    std::vector<int32_t> local;
    if (e->loc.open) {
        if (int rc = ekf_local_features(e, idf, m, local)) return rc;
        idf = local.data();
    }
    const EkfMat M = ekf_mat(e);
    for (int32_t at = 0; at < m; at += kChunk) {
        EkfObs O{};
        O.m = std::min(kChunk, m - at);
        memcpy(O.z, zf + 2 * (size_t) at, 8 * (size_t) O.m);
        memcpy(O.idf, idf + at, 4 * (size_t) O.m);
        memcpy(O.R, R, 16);
        const int n = 2 * O.m, npad = (n + kKStep - 1) / kKStep * kKStep;
        ekf_innov_kernel<<<dim3((M.n + kEkfBlock - 1) / kEkfBlock, O.m), kEkfBlock, 0, e->stream>>>(M.P, M.ld, M.n, M.x, O, M.PHt, M.w);
        if (int rc = ekf_launched("ekf_innov_kernel")) return rc;
        ekf_chol_kernel<<<1, kEkfBlock, 0, e->stream>>>(M.PHt, M.ld, O, M.w);
        if (int rc = ekf_launched("ekf_chol_kernel")) return rc;
        ekf_gain_kernel<<<(M.n + 31) / 32, kEkfBlock, 0, e->stream>>>(M.PHt, M.ld, M.n, M.x, n, npad, M.W1, M.w);
        if (int rc = ekf_launched("ekf_gain_kernel")) return rc;
        if (e->loc.open)
            if (int rc = ekf_local_chunk(e, n)) return rc;
        const int tiles = (M.n + kTile - 1) / kTile;
        ekf_syrk_kernel<<<dim3(tiles, tiles), kEkfBlock, 0, e->stream>>>(M.P, M.ld, M.n, M.W1, npad, e->flag);
        if (int rc = ekf_launched("ekf_syrk_kernel")) return rc;
    }
    return 0;
}

// how many features a call may still create: the handle's capacity and, in a local period, the period's
int ekf_room(slamgpu_ekf *e, int n, const char *note) {
    if (nf_of(e) + n > e->cfg.max_landmarks)
        return fail(SLAMGPU_ERR_CAPACITY, "%d features + %d new exceed max_landmarks %d%s", nf_of(e), n, e->cfg.max_landmarks, note);
    if (e->loc.open && e->loc.n_new + n > e->loc.max_new)
        return fail(SLAMGPU_ERR_CAPACITY, "%d features created in the local period + %d new exceed its max_new %d%s", e->loc.n_new, n, e->loc.max_new, note);
    return 0;
}

int ekf_augment(slamgpu_ekf *e, const float *zn, int32_t n, const float Re[4]) {
    if (int rc = ekf_room(e, n, "")) return rc;
    for (int32_t q = 0; q < n; q++) {  // serial by nature: each feature's rows start from the pose rows, which the previous one left alone
        const EkfMat m = ekf_mat(e);
        if (e->loc.open)
            if (int rc = ekf_local_augment_carried(e, zn[2 * q], zn[2 * q + 1])) return rc;
        ekf_augment_kernel<<<(m.len + kEkfBlock - 1) / kEkfBlock, kEkfBlock, 0, e->stream>>>(m.P, m.ld, m.len, m.x, zn[2 * q], zn[2 * q + 1], Re[0],
                                                                                             Re[1], Re[2], Re[3]);
        if (int rc = ekf_launched("ekf_augment_kernel")) return rc;
        e->dim += 2;
        if (e->loc.open) e->loc.n_new++;
    }
    return 0;
}

void ekf_release(slamgpu_ekf *e) {
    ekf_local_release(e);
    e->P.release();
    e->x.release();
    e->PHt.release();
    e->W1.release();
    e->work.release();
    e->z_dev.release();
    e->blk_dev.release();
    e->flag.release();
    e->lab_dev.release();
    e->idx_dev.release();
    e->rm_src.release();
    e->rm_host.release();
    if (e->rm_ev) (void) hipEventDestroy(e->rm_ev);
    e->pin.release();
    e->stream.release();
    delete e;
}

int ekf_reserve(slamgpu_ekf *e) {
    if (int rc = e->stream.create()) return rc;
    const size_t ld = (size_t) e->ld, rows = ((size_t) e->cap_dim + kTile - 1) / kTile * kTile;
    if (int rc = e->P.reserve_zeroed(ld * e->cap_dim, "EKF covariance P")) return rc;
    if (int rc = e->x.reserve_zeroed(ld, "EKF state x")) return rc;
    if (int rc = e->PHt.reserve_zeroed(ld * kKMax, "EKF P H^T")) return rc;
    if (int rc = e->W1.reserve_zeroed(rows * kKMax, "EKF W1")) return rc;
    Layout L;
    const auto H5 = L.take<float>(10 * kChunk), v = L.take<float>(kKMax), t = L.take<float>(kKMax), Ui = L.take<float>(kKMax * kKMax),
               hv = L.take<float>(2), c2 = L.take<float>(ld), Wh = L.take<float>(ld);
    if (int rc = e->work.reserve_zeroed(L.total() / sizeof(float), "EKF work area")) return rc;
    if (int rc = e->flag.reserve_zeroed(4, "EKF flags")) return rc;
    char *base = reinterpret_cast<char *>(e->work.p);
    auto at = [&](size_t off) { return reinterpret_cast<float *>(base + off); };
    e->w = EkfWork{at(H5.off), at(v.off), at(t.off), at(Ui.off), at(hv.off), at(c2.off), at(Wh.off), e->flag.p};
    if (int rc = e->pin.reserve(4096, "EKF staging")) return rc;
    return 0;
}

}  // namespace

extern "C" {

int slamgpu_ekf_create(const slamgpu_ekf_config *cfg, slamgpu_ekf **out) {
    if (!cfg || !out) return fail(SLAMGPU_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(slamgpu_ekf_config))
        return fail(SLAMGPU_ERR_INVALID, "slamgpu_ekf_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(slamgpu_ekf_config));
    if (int rc = ekf_check_config(cfg, 32000)) return rc;
    slamgpu_ekf *e = new slamgpu_ekf();
    e->cfg = *cfg;
    e->cap_dim = ekf_cap_dim(cfg->max_landmarks);
    e->ld = ekf_ld(e->cap_dim);
    e->stream.adopt(cfg->external_stream);
    if (int rc = ekf_reserve(e)) {
        ekf_release(e);
        return rc;
    }
    *out = e;
    return 0;
}

void slamgpu_ekf_destroy(slamgpu_ekf *e) {
    if (!e) return;
    (void) hipSetDevice(e->cfg.device);
    if (e->stream) (void) hipStreamSynchronize(e->stream);
    ekf_release(e);
}

int slamgpu_ekf_predict(slamgpu_ekf *e, float V, float G, const float Q[4], float dt) {
    if (int rc = ekf_check(e)) return rc;
    if (!Q) return fail(SLAMGPU_ERR_INVALID, "null Q");
    return ekf_counted(e, ekf_predict(e, V, G, Q, dt));
}

int slamgpu_ekf_observe_heading(slamgpu_ekf *e, float phi) {
    if (int rc = ekf_check(e)) return rc;
    return ekf_counted(e, ekf_heading(e, phi));
}

int slamgpu_ekf_associate(slamgpu_ekf *e, const float *z, int32_t nz, const float Re[4], int32_t *labels_out) {
    if (int rc = ekf_check(e)) return rc;
    if (nz < 0 || !Re || (nz > 0 && (!z || !labels_out))) return fail(SLAMGPU_ERR_INVALID, "bad association arguments");
    return ekf_counted(e, ekf_associate(e, z, nz, Re, labels_out));
}

int slamgpu_ekf_update(slamgpu_ekf *e, const float *zf, const int32_t *idf, int32_t m, const float R[4]) {
    if (int rc = ekf_check(e)) return rc;
    if (m < 0 || !R || (m > 0 && (!zf || !idf))) return fail(SLAMGPU_ERR_INVALID, "bad update arguments");
    const int rc = ekf_update(e, zf, idf, m, R);
    if (rc == 0) e->stats.observed(idf, m, ++e->stats.epoch);
    return ekf_counted(e, rc);
}

int slamgpu_ekf_augment(slamgpu_ekf *e, const float *zn, int32_t n, const float Re[4]) {
    if (int rc = ekf_check(e)) return rc;
    if (n < 0 || !Re || (n > 0 && !zn)) return fail(SLAMGPU_ERR_INVALID, "bad augment arguments");
    const int rc = ekf_augment(e, zn, n, Re);
    if (rc == 0) e->stats.append(n, e->stats.epoch);
    return ekf_counted(e, rc);
}

int slamgpu_ekf_sim(slamgpu_ekf *e, float V, float G, const float Q[4], float dt, float phi, const float *z, const int32_t *ids, int32_t nz,
                    const float Re[4], const float R[4], int32_t observe) {
    if (int rc = ekf_check(e)) return rc;
    if (!Q) return fail(SLAMGPU_ERR_INVALID, "null Q");
    const bool known = e->cfg.association_known != 0;
    if (observe && (nz < 0 || !Re || !R || (nz > 0 && (!z || (known && !ids))))) return fail(SLAMGPU_ERR_INVALID, "bad observation arguments");
    std::vector<float> zf, zn;
    std::vector<int32_t> idf, idn;
    if (observe && known) {  // EkfSlam::associate_known: it does not look at the state, so the capacity is checked before anything runs
        for (int32_t i = 0; i < nz; i++) {
            if (ids[i] < 0) return fail(SLAMGPU_ERR_INVALID, "ids[%d] = %d", i, ids[i]);
            const int32_t f = e->table.lookup(ids[i]);
            if (f < 0) {
                zn.insert(zn.end(), {z[2 * i], z[2 * i + 1]});
                idn.push_back(ids[i]);
            } else {
                zf.insert(zf.end(), {z[2 * i], z[2 * i + 1]});
                idf.push_back(f);
            }
        }
        if (int rc = ekf_room(e, (int) idn.size(), "")) return rc;
        if (e->loc.open) {  // an id on a passive feature: refused before anything runs
            std::vector<int32_t> local;
            if (int rc = ekf_local_features(e, idf.data(), (int32_t) idf.size(), local)) return rc;
        }
    }
    if (int rc = ekf_predict(e, V, G, Q, dt)) return rc;
    if (e->cfg.use_heading)
        if (int rc = ekf_heading(e, phi)) return rc;
    if (!observe) return ekf_counted(e, 0);
    if (!known) {
        std::vector<int32_t> lab((size_t) nz);
        if (int rc = ekf_associate(e, z, nz, Re, lab.data())) return rc;
        for (int32_t i = 0; i < nz; i++) {
            if (lab[i] >= 0) {
                zf.insert(zf.end(), {z[2 * i], z[2 * i + 1]});
                idf.push_back(lab[i]);
            } else if (lab[i] == SLAMGPU_ASSOC_NEW) {
                zn.insert(zn.end(), {z[2 * i], z[2 * i + 1]});
            }
        }
        if (int rc = ekf_room(e, (int) (zn.size() / 2), " (the predict and heading stages have been applied)")) return rc;
    }
    const int nf0 = nf_of(e);
    const int32_t epoch = e->stats.epoch + 1;  // this step's, once it has succeeded
    if (e->cfg.batch_update) {
        if (int rc = ekf_update(e, zf.data(), idf.data(), (int32_t) idf.size(), R)) return rc;
        e->stats.observed(idf.data(), (int32_t) idf.size(), epoch);
    }
    if (int rc = ekf_augment(e, zn.data(), (int32_t) (zn.size() / 2), Re)) return rc;
    e->stats.append((int) (zn.size() / 2), epoch);
    e->table.learn(idn, nf0);
    e->stats.epoch = epoch;
    return ekf_counted(e, 0);
}

int slamgpu_ekf_dim(slamgpu_ekf *e) {
    if (!e) return fail(SLAMGPU_ERR_INVALID, "null EKF handle");
    return e->dim;
}

int slamgpu_ekf_pose(slamgpu_ekf *e, double xyt[3], double Pvv[9]) {
    if (int rc = ekf_check(e)) return rc;
    if (!xyt && !Pvv) return fail(SLAMGPU_ERR_INVALID, "null outputs");
    float *h = reinterpret_cast<float *>(e->pin.p);
    const EkfMat m = ekf_mat(e);
    HIP_TRY(hipMemcpyAsync(h, m.x, 12, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpy2DAsync(h + 3, 12, m.P, sizeof(float) * (size_t) m.ld, 12, 3, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 3 && xyt; i++) xyt[i] = h[i];
    for (int i = 0; i < 9 && Pvv; i++) Pvv[i] = h[3 + i];
    return 0;
}

int slamgpu_ekf_state(slamgpu_ekf *e, float *x, float *P, int32_t ld_out) {
    if (int rc = ekf_check(e)) return rc;
    if (int rc = ekf_closed(e, "slamgpu_ekf_state")) return rc;
    if (P && ld_out < e->dim) return fail(SLAMGPU_ERR_INVALID, "ld_out %d < dim %d", ld_out, e->dim);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rc = ekf_state_out(e->x, e->P, e->ld, e->dim, x, P, ld_out)) return rc;
    return e->dim;
}

int slamgpu_ekf_block(slamgpu_ekf *e, const int32_t *idx, int32_t k, float *out) {
    if (int rc = ekf_check(e)) return rc;
    if (int rc = ekf_closed(e, "slamgpu_ekf_block")) return rc;
    if (k < 0 || (k > 0 && (!idx || !out))) return fail(SLAMGPU_ERR_INVALID, "bad block arguments");
    for (int32_t a = 0; a < k; a++)
        if (idx[a] < 0 || idx[a] >= e->cap_dim) return fail(SLAMGPU_ERR_INVALID, "idx[%d] = %d outside [0, %d)", a, idx[a], e->cap_dim);
    if (k == 0) return 0;
    const size_t kk = (size_t) k * k;
    if (int rc = e->idx_dev.reserve((size_t) k, "EKF block indices")) return rc;
    if (int rc = e->blk_dev.reserve(kk, "EKF block")) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->idx_dev, idx, sizeof(int32_t) * (size_t) k, hipMemcpyHostToDevice));
    ekf_block_kernel<<<(unsigned) ((kk + kEkfBlock - 1) / kEkfBlock), kEkfBlock, 0, e->stream>>>(e->P, e->ld, e->idx_dev, k, e->blk_dev);
    if (int rc = ekf_launched("ekf_block_kernel")) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, e->blk_dev, sizeof(float) * kk, hipMemcpyDeviceToHost));
    return 0;
}

int slamgpu_ekf_upload(slamgpu_ekf *e, int32_t dim, const float *x, const float *P, int32_t ld_in) {
    if (int rc = ekf_check(e)) return rc;
    if (int rc = ekf_closed(e, "slamgpu_ekf_upload")) return rc;
    if (int rc = ekf_state_in(e->stream, e->x, e->P, e->ld, e->cap_dim, dim, x, P, ld_in)) return rc;
    e->dim = dim;
    e->table.identity(nf_of(e));
    e->stats.uploaded(nf_of(e));
    return 0;
}

int slamgpu_ekf_remove(slamgpu_ekf *e, const int32_t *features, int32_t k) {
    if (int rc = ekf_check(e)) return rc;
    if (int rc = ekf_closed(e, "slamgpu_ekf_remove")) return rc;
    if (k < 0 || (k > 0 && !features)) return fail(SLAMGPU_ERR_INVALID, "bad remove arguments");
    const int nf = nf_of(e);
    for (int32_t q = 0; q < k; q++) {
        if (features[q] < 0 || features[q] >= nf) return fail(SLAMGPU_ERR_INVALID, "features[%d] = %d outside [0, %d)", q, features[q], nf);
        if (q > 0 && features[q] <= features[q - 1]) return fail(SLAMGPU_ERR_INVALID, "features[%d] = %d after %d: not ascending and distinct", q, features[q], features[q - 1]);
    }
    if (k == 0) return 0;
    const int dim = e->dim, n = dim - 2 * k, s0 = 3 + 2 * features[0];
    if (s0 < n) {  // something moves (otherwise the removed features are the last ones)
        if (int rc = e->rm_src.reserve((size_t) n, "EKF removal index map")) return rc;
        if (int rc = e->rm_host.reserve((size_t) n, "EKF removal index staging")) return rc;
        if (!e->rm_ev) HIP_TRY(hipEventCreateWithFlags(&e->rm_ev, hipEventDisableTiming));
        if (e->rm_used) HIP_TRY(hipEventSynchronize(e->rm_ev));  // (the previous removal's map: taken long ago)
        int32_t *src = e->rm_host.p;
        for (int i = 0; i < 3; i++) src[i] = i;
        for (int f = 0, q = 0, at = 3; f < nf; f++) {
            if (q < k && features[q] == f) {
                q++;
                continue;
            }
            src[at++] = 3 + 2 * f;
            src[at++] = 4 + 2 * f;
        }
        HIP_TRY(hipMemcpyAsync(e->rm_src, src, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipEventRecord(e->rm_ev, e->stream));
        e->rm_used = true;
        const int nt = (n + kRmTile - 1) / kRmTile, b0 = s0 / kRmTile;
        ekf_remove_gather_kernel<<<dim3(nt - b0, nt), kEkfBlock, 0, e->stream>>>(e->P, e->ld, n, s0, b0, e->rm_src, e->x, e->w.c2, e->w.Wh);
        if (int rc = ekf_launched("ekf_remove_gather_kernel")) return rc;
        ekf_remove_mirror_kernel<<<dim3(nt, nt - b0), kEkfBlock, 0, e->stream>>>(e->P, e->ld, n, s0, b0, e->x, e->w.c2, e->w.Wh);
        if (int rc = ekf_launched("ekf_remove_mirror_kernel")) return rc;
    }
    const size_t zeroed = (size_t) (dim - n) * ((size_t) dim + n);
    ekf_remove_zero_kernel<<<(unsigned) ((zeroed + kEkfBlock - 1) / kEkfBlock), kEkfBlock, 0, e->stream>>>(e->P, e->ld, n, dim, e->x);
    if (int rc = ekf_launched("ekf_remove_zero_kernel")) return rc;
    e->dim = n;
    e->table.remove(features, k);
    e->stats.remove(features, k);
    return 0;
}

int slamgpu_ekf_feature_stats(slamgpu_ekf *e, int32_t *hits, int32_t *born, int32_t *last, int32_t *epoch) {
    if (!e) return fail(SLAMGPU_ERR_INVALID, "null EKF handle");
    const EkfFeatureStats &s = e->stats;
    const size_t bytes = sizeof(int32_t) * s.hits.size();
    if (hits && bytes) memcpy(hits, s.hits.data(), bytes);
    if (born && bytes) memcpy(born, s.born.data(), bytes);
    if (last && bytes) memcpy(last, s.last.data(), bytes);
    if (epoch) *epoch = s.epoch;
    return (int) s.hits.size();
}

int slamgpu_ekf_status(slamgpu_ekf *e, int32_t *status) {
    if (int rc = ekf_check(e)) return rc;
    if (!status) return fail(SLAMGPU_ERR_INVALID, "null output");
    int32_t *h = reinterpret_cast<int32_t *>(e->pin.p);
    HIP_TRY(hipMemcpyAsync(h, e->flag.p + 1, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *status = *h;
    return 0;
}

int slamgpu_ekf_sync(slamgpu_ekf *e) {
    if (int rc = ekf_check(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
