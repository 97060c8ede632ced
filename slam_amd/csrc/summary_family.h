// The shared pieces of the posterior summaries (slamgpu_map_summary, _map_pairs, _innovation_*, _joint_summary, _pose_*, _path_summary):
// every summary takes the same particle set, the same weights and the same order of merging, and takes them from here.
// kernels.hip includes this file once, after block_scale and the genealogy helpers.  Plain function templates: each takes what it
// uses as arguments; the kernels own their __shared__ arrays and hand them in (summary_finish, a whole kernel body, declares its own).
#pragma once

namespace SLAM_KNS {

// the record of landmark l behind genealogy entry sl (single contexts: read_through_genealogy past its genealogy load, so that the
// slots of one genealogy row share that load)
SLAM_DEV void read_record(const Buffers &B, const int32_t *__restrict__ live, size_t S, int l, int sl, float4 &la, float &lb) {
    if (sl < 0) {
        const size_t at = (size_t) l * B.pool_cap + (sl & ~kPoolBit);
        la = B.poolA[at];
        lb = B.poolB[at];
    } else {
        const int b = live[l];
        la = B.lmkA[b][(size_t) l * S + sl];
        lb = B.lmkB[b][(size_t) l * S + sl];
    }
}
// whether that record is there (read_record's addresses, the x of its first half alone)
SLAM_DEV bool record_held(const Buffers &B, const int32_t *__restrict__ live, size_t S, int l, int sl) {
    const float x = sl < 0 ? B.poolA[(size_t) l * B.pool_cap + (sl & ~kPoolBit)].x : B.lmkA[live[l]][(size_t) l * S + sl].x;
    return x == x;
}

// one (W, mean, M2, sum w Pf, holders) summary and the pairwise update with the one that follows it in particle order
struct MapPart {
    double v[kMapFields];
};
SLAM_DEV void map_merge(MapPart &a, const MapPart &b) {
    a.v[kMapCnt] += b.v[kMapCnt];
    if (!(b.v[kMapW] != 0.0)) return;  // nothing of weight in b (its holders, if any, are counted)
    if (!(a.v[kMapW] != 0.0)) {
        const double cnt = a.v[kMapCnt];
        a = b;
        a.v[kMapCnt] = cnt;
        return;
    }
    const double W = a.v[kMapW] + b.v[kMapW], f = b.v[kMapW] / W, g = a.v[kMapW] * f;
    const double dx = b.v[kMapMx] - a.v[kMapMx], dy = b.v[kMapMy] - a.v[kMapMy];
    a.v[kMapMx] += dx * f;
    a.v[kMapMy] += dy * f;
    a.v[kMapXX] += b.v[kMapXX] + dx * dx * g;
    a.v[kMapXY] += b.v[kMapXY] + dx * dy * g;
    a.v[kMapYY] += b.v[kMapYY] + dy * dy * g;
    a.v[kMapP00] += b.v[kMapP00];
    a.v[kMapP10] += b.v[kMapP10];
    a.v[kMapP11] += b.v[kMapP11];
    a.v[kMapW] = W;
}

// This lane's T particles of tile blockIdx.x (particle t * kBlock + threadIdx.x of the tile): whether they exist, their ancestors
// (through ws.keep while a resample is pending) and their weights (resampled particles restart at 1/N, as in peek_kernel); mb: the
// lane's largest log-weight.  With pa, the ancestors' poses: weight and pose then come from one 16-byte load.
template <int T>
SLAM_DEV void summary_lanes(const Buffers &B, const WeightScratch &ws, const Ctrl *ctrl, int cur, bool pend, int logw, bool (&on)[T], int (&anc)[T],
                            float (&wf)[T], float &mb, float4 (*pa)[T] = nullptr) {
    mb = -INFINITY;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int i = blockIdx.x * (T * kBlock) + t * kBlock + threadIdx.x;
        on[t] = i < B.n;
        anc[t] = on[t] ? (pend ? ws.keep[B.slot][i] : i) : 0;
        if (pa) (*pa)[t] = on[t] ? B.poseA[cur][anc[t]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
        wf[t] = on[t] ? (pend ? ctrl->inv_n : pa ? (*pa)[t].w : B.poseA[cur][anc[t]].w) : 0.0f;
        if (on[t] && logw) mb = fmaxf(mb, wf[t]);
    }
}

// The weights the sums are taken with.  Log-weights: mb becomes M_t, the tile's largest, and w = exp(l - M_t); linear: mb = 0, w = wf.
// sh_m: kBlock / kWave floats of the workgroup's.
template <int T>
SLAM_DEV void tile_weights(int logw, const float (&wf)[T], const bool (&on)[T], float &mb, int lane, int wave, float *sh_m, double (&w)[T]) {
    constexpr int kWaves = kBlock / kWave;
    if (logw) {
        for (int d = kWave / 2; d > 0; d >>= 1) mb = fmaxf(mb, __shfl_xor(mb, d, kWave));
        if (lane == 0) sh_m[wave] = mb;
        __syncthreads();
        mb = sh_m[0];
        for (int v = 1; v < kWaves; v++) mb = fmaxf(mb, sh_m[v]);
#pragma unroll
        for (int t = 0; t < T; t++) w[t] = (on[t] && mb != -INFINITY) ? exp((double) wf[t] - (double) mb) : 0.0;
    } else {
        mb = 0.0f;
#pragma unroll
        for (int t = 0; t < T; t++) w[t] = (double) wf[t];
    }
}

// The tile's sum of weights and M_t into wpart[2 tile], [2 tile + 1]: every group of slots would find the same bits, the grid's first
// stores them.  sh_w: kBlock / kWave doubles of the workgroup's.
template <int T>
SLAM_DEV void tile_weight_sum(const double (&w)[T], float mb, int lane, int wave, double *sh_w, double *wpart) {
    constexpr int kWaves = kBlock / kWave;
    if (blockIdx.y != 0) return;
    double sw = 0.0;
#pragma unroll
    for (int t = 0; t < T; t++) sw += w[t];
    sw = wave_sum_d(sw);
    if (lane == 0) sh_w[wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = sh_w[0];
        for (int v = 1; v < kWaves; v++) tot += sh_w[v];
        wpart[2 * blockIdx.x] = tot;
        wpart[2 * blockIdx.x + 1] = (double) mb;
    }
}

// A wave's nine sums about its pivot (a: sum w | w dx, w dy | w dx^2, w dx dy, w dy^2 | the three plain weighted sums) and its
// number of holders, as the wave's MapPart o.  (W == 0: holders without weight are counted, and carry nothing else)
SLAM_DEV void moments_emit(double *o, const double *a, double px, double py, int cnt) {
    const double W = a[0];
    const bool any = W != 0.0;
    const double mx = any ? a[1] / W : 0.0, my = any ? a[2] / W : 0.0;
    o[kMapW] = W;
    o[kMapMx] = px + mx;
    o[kMapMy] = py + my;
    o[kMapXX] = a[3] - a[1] * mx;
    o[kMapXY] = a[4] - a[1] * my;
    o[kMapYY] = a[5] - a[2] * my;
    o[kMapP00] = a[6];
    o[kMapP10] = a[7];
    o[kMapP11] = a[8];
    o[kMapCnt] = (double) cnt;
}

// The end of a tile: thread s < sn merges the waves' MapParts of slot s0 + s in ascending order (wave v: lanes v * 64 .. of each of the
// tile's strides) and stores the tile's column of A.part.  FIELDS = kInnFields: the plain sum behind the MapPart is added up beside it.
template <int FIELDS>
SLAM_DEV void tile_merge_store(double (*sh)[kBlock / kWave][FIELDS], int sn, int s0, const MapSummaryArgs &A) {
    constexpr int kWaves = kBlock / kWave;
    __syncthreads();
    if ((int) threadIdx.x >= sn) return;
    const int s = threadIdx.x;
    MapPart m;
    for (int q = 0; q < kMapFields; q++) m.v[q] = sh[s][0][q];
    double extra = 0.0;
    if constexpr (FIELDS > kMapFields) extra = sh[s][0][kMapFields];
    for (int v = 1; v < kWaves; v++) {
        MapPart b;
        for (int q = 0; q < kMapFields; q++) b.v[q] = sh[s][v][q];
        map_merge(m, b);
        if constexpr (FIELDS > kMapFields) extra += sh[s][v][kMapFields];
    }
    double *p = A.part + (size_t) blockIdx.x * FIELDS * (size_t) A.count + (size_t) (s0 + s);
    for (int q = 0; q < kMapFields; q++) p[(size_t) q * A.count] = m.v[q];
    if constexpr (FIELDS > kMapFields) p[(size_t) kMapFields * A.count] = extra;
}

// The finishing pass of the summaries that reduce MapPart partials: the body of map_finish_kernel (slamgpu_map_summary and
// slamgpu_map_pairs) and of innovation_finish_kernel (INNOV, with I), so that the sum of all weights has one path.
// kMapFinParts threads per slot: each merges its stretch of the tiles' partials in ascending order (and adds up that stretch's
// weights), the slot's first thread merges the stretches in ascending order, normalises and writes the outputs.  INNOV: a partial has
// kInnFields fields, the last a plain weighted sum (sum w nis) that is scaled and added like sum w P, and the outputs go to the
// staging area or to the ring.
template <bool INNOV>
SLAM_DEV void summary_finish(const MapSummaryArgs &A, const InnovArgs *I) {
    constexpr int kFinFields = INNOV ? kInnFields : kMapFields;
    constexpr int kFinStride = INNOV ? kInnStride : kMapStride;
    constexpr int kSlots = kBlock / kMapFinParts;
    __shared__ double sh[kMapFinParts][kFinFields + 1][kSlots];
    __shared__ double sh_m[kBlock / kWave];
    const int sl = threadIdx.x % kSlots, part = threadIdx.x / kSlots;
    const int s = blockIdx.x * kSlots + sl;
    double M = -INFINITY;
    if (A.logw) {  // the largest log-weight of all tiles
        for (int t = threadIdx.x; t < A.tiles; t += kBlock) M = fmax(M, A.wpart[2 * t + 1]);
        for (int d = kWave / 2; d > 0; d >>= 1) M = fmax(M, __shfl_xor(M, d, kWave));
        if ((threadIdx.x & (kWave - 1)) == 0) sh_m[threadIdx.x / kWave] = M;
        __syncthreads();
        M = sh_m[0];
        for (int v = 1; v < kBlock / kWave; v++) M = fmax(M, sh_m[v]);
    }
    const int per = (A.tiles + kMapFinParts - 1) / kMapFinParts, t0 = part * per, t1 = min(A.tiles, t0 + per);
    MapPart m;
    for (int q = 0; q < kMapFields; q++) m.v[q] = 0.0;
    double nis = 0.0;
    double wsum = 0.0;
    for (int t = t0; t < t1; t++) {
        const double f = A.logw ? block_scale((float) A.wpart[2 * t + 1], M) : 1.0;
        wsum += A.wpart[2 * t] * f;
        if (s >= A.count) continue;
        const double *p = A.part + (size_t) t * kFinFields * (size_t) A.count + (size_t) s;
        MapPart b;
        for (int q = 0; q < kMapFields; q++) b.v[q] = p[(size_t) q * A.count];
        if (A.logw) {
            b.v[kMapW] *= f;
            for (int q = kMapXX; q <= kMapP11; q++) b.v[q] *= f;
        }
        map_merge(m, b);
        if constexpr (INNOV)
            if (b.v[kMapW] != 0.0) nis += p[(size_t) kInnNis * A.count] * f;  // (of the tiles map_merge takes sums from)
    }
    for (int q = 0; q < kMapFields; q++) sh[part][q][sl] = m.v[q];
    sh[part][kMapFields][sl] = wsum;
    if constexpr (INNOV) sh[part][kMapFields + 1][sl] = nis;
    __syncthreads();
    if (part != 0 || s >= A.count) return;
    double Wtot = wsum;
    for (int v = 1; v < kMapFinParts; v++) {
        MapPart b;
        for (int q = 0; q < kMapFields; q++) b.v[q] = sh[v][q][sl];
        map_merge(m, b);
        if constexpr (INNOV) nis += sh[v][kMapFields + 1][sl];
        Wtot += sh[v][kMapFields][sl];
    }
    size_t at = (size_t) s;
    if constexpr (INNOV) {
        if (I->ring_cap > 0) {  // entry ring_at + s of the ring, with its tags
            at = (size_t) ((I->ring_at + (int64_t) s) % (int64_t) I->ring_cap);
            I->tag[2 * at] = I->record;
            I->tag[2 * at + 1] = I->idf ? I->idf[s] : kInnSlotPerParticle;
        }
    }
    double *o = A.out + at * kFinStride;
    if (!INNOV || A.holders) A.holders[s] = (int32_t) m.v[kMapCnt];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!(Wtot > 0.0) || !(Wtot < INFINITY)) {  // the weights sum to zero or to nothing finite: SLAMGPU_STATUS_DEGENERATE's convention
        for (int q = 0; q < kFinStride; q++) o[q] = nan;
        return;
    }
    const double W = m.v[kMapW];
    o[0] = W / Wtot;
    const bool held = m.v[kMapCnt] != 0.0 && W != 0.0;
    o[1] = held ? m.v[kMapMx] : nan;
    o[2] = held ? m.v[kMapMy] : nan;
    for (int q = kMapXX; q <= kMapP11; q++) o[q] = held ? m.v[q] / W : nan;
    if constexpr (INNOV) o[9] = held ? nis / W : nan;
}

}  // namespace SLAM_KNS
