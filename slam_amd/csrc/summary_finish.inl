// The finishing pass of the summaries that reduce (W, mean, M2, sum w P, holders) partials: the one text of map_finish_kernel
// (SLAM_FINISH_INNOV 0: slamgpu_map_summary and slamgpu_map_pairs) and innovation_finish_kernel (SLAM_FINISH_INNOV 1), which
// kernels.hip includes as their bodies so that both compile the same statements and the sum of all weights has one path.
// kMapFinParts threads per slot: each merges its stretch of the tiles' partials in ascending order (and adds up that stretch's
// weights), the slot's first thread merges the stretches in ascending order, normalises and writes the outputs.
// Expects: A (MapSummaryArgs) and, with SLAM_FINISH_INNOV, I (InnovArgs): a partial then has kInnFields fields, the last a plain
// weighted sum (sum w nis) that is scaled and added like sum w P, and the outputs go to the staging area or to the ring.
#if SLAM_FINISH_INNOV
    constexpr int kFinFields = kInnFields;
#else
    constexpr int kFinFields = kMapFields;
#endif
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
#if SLAM_FINISH_INNOV
    double nis = 0.0;
#endif
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
#if SLAM_FINISH_INNOV
        if (b.v[kMapW] != 0.0) nis += p[(size_t) kInnNis * A.count] * f;  // (of the tiles map_merge takes sums from)
#endif
    }
    for (int q = 0; q < kMapFields; q++) sh[part][q][sl] = m.v[q];
    sh[part][kMapFields][sl] = wsum;
#if SLAM_FINISH_INNOV
    sh[part][kMapFields + 1][sl] = nis;
#endif
    __syncthreads();
    if (part != 0 || s >= A.count) return;
    double Wtot = wsum;
    for (int v = 1; v < kMapFinParts; v++) {
        MapPart b;
        for (int q = 0; q < kMapFields; q++) b.v[q] = sh[v][q][sl];
        map_merge(m, b);
#if SLAM_FINISH_INNOV
        nis += sh[v][kMapFields + 1][sl];
#endif
        Wtot += sh[v][kMapFields][sl];
    }
#if SLAM_FINISH_INNOV
    size_t at = (size_t) s;
    if (I.ring_cap > 0) {  // entry ring_at + s of the ring, with its tags
        at = (size_t) ((I.ring_at + (int64_t) s) % (int64_t) I.ring_cap);
        I.tag[2 * at] = I.record;
        I.tag[2 * at + 1] = I.idf[s];
    }
    double *o = A.out + at * kInnStride;
    if (A.holders) A.holders[s] = (int32_t) m.v[kMapCnt];
    constexpr int kFinStride = kInnStride;
#else
    double *o = A.out + (size_t) s * kMapStride;
    A.holders[s] = (int32_t) m.v[kMapCnt];
    constexpr int kFinStride = kMapStride;
#endif
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
#if SLAM_FINISH_INNOV
    o[9] = held ? nis / W : nan;
#endif
