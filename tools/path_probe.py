"""Cost of the path posterior (slamgpu_path_*), in one process, example_webmap, FastSLAM 2, fast build, known association:

  (a) recording: slamgpu_run_observe over 200 observation steps with recording on against the same call with it off (fresh contexts
      of the same seed, the two arms taken in turn), at 10^5 particles and at 1 000 -- where the persistent one-launch loop is what
      recording gives up.  Wall time of the call + a synchronisation, per step; 2 runs of warm-up, the median of 7.
  (b) slamgpu_path_summary and slamgpu_path_trace over 200 and over 2 000 records at 10^5 particles, after that many steps of the
      course (the genealogy is the filter's own): the kernels' time between event pairs (slamgpu_profile / slamgpu_kernel_time), the
      whole call between two events, algorithmic bytes = records x N x bytes actually read per particle and record (the record's 16 B
      where the particle still has a descendant, the 12 B of descendants' weight and count everywhere) and that rate beside the copy
      rate this tree has measured on the part (profiles/copy_ceiling_r04.txt).

    python tools/path_probe.py [--out profiles/path.txt] [--steps 200 2000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import slam_amd  # noqa: E402
from particle_lists_probe import course  # noqa: E402

COPY = (4.9e12, 5.3e12)
WALK = ("path_seed", "path_push", "path_finish")


def known(c, N):
    s = slam_amd.SlamGpu(N, c["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         math_mode=slam_amd.MATH_FAST)
    s.set_map(c["lm"])
    return s


def run(s, c, a, b):
    s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)


def recording_cost(c, N, steps=200, reps=7, warm=2):
    us = {False: [], True: []}
    for rep in range(warm + reps):
        for on in (False, True):
            s = known(c, N)
            if on:
                s.path_enable(steps)
            run(s, c, 0, 8)  # (first launches, allocations)
            s.history_fetch()
            if on:
                s.path_enable(steps)
            s.sync()
            t0 = time.perf_counter()
            run(s, c, 8, 8 + steps)
            s.sync()
            dt = time.perf_counter() - t0
            if rep >= warm:
                us[on].append(1e6 * dt / steps)
            launches = s.persist_info()[0]
            s.close()
    off, on_ = statistics.median(us[False]), statistics.median(us[True])
    return ["  N = %d: recording off %.2f us per step (runs %s)%s" % (N, off, " ".join("%.2f" % x for x in us[False]),
                                                                  "" if N > 2048 else "  [the persistent loop: one launch per call]"),
            "  %s  recording on  %.2f us per step (runs %s)  [persistent launches of the last run: %d]" %
            (" " * len("N = %d:" % N), on_, " ".join("%.2f" % x for x in us[True]), launches),
            "  %s  -> +%.2f us per step, x %.2f" % (" " * len("N = %d:" % N), on_ - off, on_ / off)]


def walks(c, N, steps, reps=7, warm=2):
    s = known(c, N)
    s.path_enable(steps)
    for a in range(0, steps, 1000):
        run(s, c, a, min(steps, a + 1000))
        s.history_fetch()
    s.profile(True)
    ks, ws, kt, wt = [], [], [], []
    for rep in range(warm + reps):
        a = sum(s.kernel_time(k)[0] for k in WALK)
        s.timer_start()
        ps = s.path_summary()
        w = s.timer_stop()
        k = sum(s.kernel_time(k)[0] for k in WALK) - a
        a = s.kernel_time("path_trace")[0]
        s.timer_start()
        s.path_trace(-1)
        w2 = s.timer_stop()
        k2 = s.kernel_time("path_trace")[0] - a
        if rep >= warm:
            ks.append(k), ws.append(w), kt.append(k2), wt.append(w2)
    launches = [s.kernel_time(k)[1] // (warm + reps) for k in WALK]
    s.profile(False)
    s.close()
    d = ps["distinct"].astype(np.float64)
    b = 16.0 * d.sum() + 12.0 * N * steps
    km, wm, tm = statistics.median(ks), statistics.median(ws), statistics.median(kt)
    back = lambda q: int(d[-1 - q]) if q < len(d) else -1
    return ["  %d records: distinct ancestors 1 / 10 / 100 records back %d / %d / %d, at the oldest record %d (mean over the records %.0f of %d)" %
            (steps, back(1), back(10), back(100), int(d[0]), d.mean(), N),
            "    path_summary kernels (seed %d + push %d + finish %d launches)  %.3f ms  (calls %s)" %
            (launches[0], launches[1], launches[2], km, " ".join("%.3f" % x for x in ks)),
            "    path_summary whole call (launches, copies of the result, sync)  %.3f ms  (calls %s)" % (wm, " ".join("%.3f" % x for x in ws)),
            "    per record %.2f us; algorithmic bytes %.3f GB -> %.3f TB/s (copy rate of this part: %.1f-%.1f TB/s)" %
            (1e3 * km / steps, b / 1e9, b / (km * 1e-3) / 1e12, COPY[0] / 1e12, COPY[1] / 1e12),
            "    path_trace(-1) kernel %.3f ms = %.3f us per record (calls %s); whole call %.3f ms; bytes %.1f KB (16 B per record)" %
            (tm, 1e3 * tm / steps, " ".join("%.3f" % x for x in kt), statistics.median(wt), 16.0 * steps / 1e3), ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, nargs="*", default=[200, 2000])
    ap.add_argument("--particles", type=int, default=100000)
    a = ap.parse_args()
    c = course(os.path.join(ROOT, "data", "example_webmap.mat"), 100000)
    lines = ["path_probe: example_webmap (%d observation steps), FastSLAM 2, fast build, known association; 2 runs of warm-up, median of 7" % len(c["ctl"]), "",
             "(a) cost of recording: run_observe over 200 steps, wall time of the call + sync, per step"]
    for N in (a.particles, 1000):
        lines += recording_cost(c, N)
    lines += ["", "(b) walks over the records, %d particles" % a.particles]
    for steps in a.steps:
        lines += walks(c, a.particles, min(steps, len(c["ctl"])))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
