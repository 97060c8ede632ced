// The weights of a lane's kMapT particles as slamgpu_map_summary takes them, and the tile's sum of them: the one text of
// map_summary_kernel, map_pairs_kernel and innovation_summary_kernel (kernels.hip includes it inside each, so that all of them compile
// the same statements).  Expects: A (MapSummaryArgs), wf[kMapT], on[kMapT], mb (the lane's largest log-weight), lane, wave, kWaves,
// __shared__ sh_w[kWaves], sh_m[kWaves].  Leaves: w[kMapT] (linear: w; log-weights: exp(l - M_t)), mb = M_t (linear: 0),
// A.wpart[2 tile], [2 tile + 1] written by the grid's first group.
    double w[kMapT];
    if (A.logw) {  // the tile's largest log-weight
        for (int d = kWave / 2; d > 0; d >>= 1) mb = fmaxf(mb, __shfl_xor(mb, d, kWave));
        if (lane == 0) sh_m[wave] = mb;
        __syncthreads();
        mb = sh_m[0];
        for (int v = 1; v < kWaves; v++) mb = fmaxf(mb, sh_m[v]);
#pragma unroll
        for (int t = 0; t < kMapT; t++) w[t] = (on[t] && mb != -INFINITY) ? exp((double) wf[t] - (double) mb) : 0.0;
    } else {
        mb = 0.0f;
#pragma unroll
        for (int t = 0; t < kMapT; t++) w[t] = (double) wf[t];
    }
    if (blockIdx.y == 0) {  // the tile's sum of weights (every group of slots would find the same bits: one of them stores it)
        double sw = 0.0;
#pragma unroll
        for (int t = 0; t < kMapT; t++) sw += w[t];
        sw = wave_sum_d(sw);
        if (lane == 0) sh_w[wave] = sw;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = sh_w[0];
            for (int v = 1; v < kWaves; v++) tot += sh_w[v];
            A.wpart[2 * blockIdx.x] = tot;
            A.wpart[2 * blockIdx.x + 1] = (double) mb;
        }
    }
