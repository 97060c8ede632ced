"""Cost of the pose posterior (slamgpu_pose_summary, slamgpu_pose_history_*), in one process, example_webmap, FastSLAM 2, fast build,
known association:

  (a) one slamgpu_pose_summary call at 10^5 particles after 200 steps of the course: the two kernels' time between event pairs
      (slamgpu_profile / slamgpu_kernel_time), the whole call between two events, the algorithmic bytes (40 B per particle: poseA, poseB,
      poseC) and that rate beside the copy rate this tree has measured on the part (profiles/copy_ceiling_r04.txt).
  (b) the per-step ring: slamgpu_run_observe over a window of observation steps (default 2 000) with the ring on against the same call
      with it off (fresh contexts of the same seed, the arms taken in turn), at 10^5 particles and at 1 000 -- where the persistent
      one-launch loop is what the ring gives up.  Wall time of the call + a synchronisation, per step; 2 runs of warm-up, median of 7.

A library without the entry points (the parent commit's, loaded through SLAMGPU_LIB for an A/B) runs the ring-off arm only: take the
two libraries in turn, process by process.

    python tools/pose_probe.py [--out profiles/pose_summary.txt] [--steps 2000] [--arms off on] [--label text]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import slam_amd  # noqa: E402
from particle_lists_probe import course  # noqa: E402

COPY = (4.9e12, 5.3e12)
KERNELS = ("pose_summary", "pose_finish")


def known(c, N):
    s = slam_amd.SlamGpu(N, c["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         math_mode=slam_amd.MATH_FAST)
    s.set_map(c["lm"])
    return s


def run(s, c, a, b):
    s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)


def one_call(c, N, reps=7, warm=2):
    s = known(c, N)
    run(s, c, 0, 200)
    s.history_fetch()
    s.profile(True)
    ks, ws = [], []
    for rep in range(warm + reps):
        a = sum(s.kernel_time(k)[0] for k in KERNELS)
        s.timer_start()
        o = s.pose_summary()
        w = s.timer_stop()
        k = sum(s.kernel_time(k)[0] for k in KERNELS) - a
        if rep >= warm:
            ks.append(k), ws.append(w)
    each = [s.kernel_time(k)[0] / (warm + reps) for k in KERNELS]
    s.profile(False)
    s.close()
    km, wm, b = statistics.median(ks), statistics.median(ws), 40.0 * N
    return ["  N = %d after 200 steps: effective sample size %.1f, resultant length of the headings %.6f" % (N, 1.0 / o[0], (o[4] ** 2 + o[5] ** 2) ** 0.5),
            "    kernels (pose_summary %.1f us + pose_finish %.1f us, event pairs)  %.1f us  (calls %s)" %
            (1e3 * each[0], 1e3 * each[1], 1e3 * km, " ".join("%.1f" % (1e3 * x) for x in ks)),
            "    whole call (two launches, the copy of 144 B, sync)  %.1f us  (calls %s)" % (1e3 * wm, " ".join("%.1f" % (1e3 * x) for x in ws)),
            "    algorithmic bytes %.2f MB -> %.3f TB/s of kernel time (copy rate of this part: %.1f-%.1f TB/s): launch latency, not bandwidth" %
            (b / 1e6, b / (km * 1e-3) / 1e12, COPY[0] / 1e12, COPY[1] / 1e12), ""]


def ring_cost(c, N, steps, arms, reps=7, warm=2):
    us = {a: [] for a in arms}
    launches = {a: 0 for a in arms}
    for rep in range(warm + reps):
        for arm in arms:
            s = known(c, N)
            run(s, c, 0, 8)  # (first launches, allocations)
            s.history_fetch()
            if arm == "on":
                s.pose_history_enable(steps)
            s.sync()
            t0 = time.perf_counter()
            run(s, c, 8, 8 + steps)
            s.sync()
            dt = time.perf_counter() - t0
            if rep >= warm:
                us[arm].append(1e6 * dt / steps)
            launches[arm] = s.persist_info()[0]
            s.close()
    out = []
    for arm in arms:
        out.append("  N = %d, ring %-3s  %.2f us per step (runs %s)  [persistent launches of the last run: %d]" %
                   (N, arm, statistics.median(us[arm]), " ".join("%.2f" % x for x in us[arm]), launches[arm]))
    if "on" in us and "off" in us:
        off, on_ = statistics.median(us["off"]), statistics.median(us["on"])
        out.append("  %s  -> +%.2f us per step, x %.2f" % (" " * len("N = %d," % N), on_ - off, on_ / off))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--arms", nargs="*", default=["off", "on"])
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    have = hasattr(slam_amd.load_library(), "slamgpu_pose_summary")
    arms = [x for x in a.arms if x == "off" or have]
    c = course(os.path.join(ROOT, "data", "example_webmap.mat"), 100000)
    steps = min(a.steps, len(c["ctl"]) - 8)
    lines = ["pose_probe%s: example_webmap, FastSLAM 2, fast build, known association; 2 runs of warm-up, median of 7; library %s" %
             (" [%s]" % a.label if a.label else "", slam_amd.lib_path()), ""]
    if have:
        lines += ["(a) one slamgpu_pose_summary call"] + one_call(c, a.particles)
    lines += ["(b) the per-step ring: run_observe over %d steps, wall time of the call + sync, per step" % steps]
    for N in (a.particles, 1000):
        lines += ring_cost(c, N, steps, arms)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
