"""Cost of the innovation posterior (slamgpu_innovation_summary, slamgpu_innovation_*), in one process, example_webmap, FastSLAM 2, fast
build, known association, host-made packets:

  (a) one slamgpu_innovation_summary call for a packet of 8 at 10^5 particles after 200 steps of the course, beside slamgpu_map_summary
      over the same 8 slots on the same context (the same records, plus 16 B of pose per particle): the kernels' time between event
      pairs (slamgpu_profile / slamgpu_kernel_time) and the whole call between two events; 2 calls of warm-up, median of 7.
  (b) the per-step loop: slamgpu_step over a window of observation steps (default 2 000) with the ring on against the same loop with it
      off (fresh contexts of the same seed, the arms taken in turn).  Wall time of the loop + a synchronisation, per step; 2 runs of
      warm-up, median of 7.

A library without the entry points (the parent commit's, loaded through SLAMGPU_LIB for an A/B) runs the ring-off arm only: take the
two libraries in turn, process by process.

    python tools/innovation_probe.py [--out profiles/innovation.txt] [--steps 2000] [--particles 100000] [--arms off on] [--label text]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slam_amd  # noqa: E402
from slam_amd import host  # noqa: E402

f32 = np.float32


def tape_of(N, steps):
    args = ["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", N, "-NEFFECTIVE", int(0.75 * N),
            "-SWITCH_SEED_RANDOM", 7]
    return host.make_tape(args, max_obs=steps)


def context(tape, N):
    return slam_amd.SlamGpu(N, tape["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, math_mode=slam_amd.MATH_FAST)


def calls(s, tape, a, b):
    """the steps' slamgpu_step calls, marshalled once (what a C++ host that holds plain arrays would pay nothing for)"""
    out = []
    for st in tape["steps"][a:b]:
        out.append(s.prepare_step(np.array(st["controls"], f32).reshape(-1, 3), tape["Q"], float(tape["dt"]), np.array(st["zf"], f32).reshape(-1, 2),
                                  np.array(st["idf"], np.int32), np.array(st["zn"], f32).reshape(-1, 2), tape["R"]))
    return out


def one_call(tape, N, reps=7, warm=2):
    s = context(tape, N)
    for f in calls(s, tape, 0, 200):
        f()
    s.history_fetch()
    nf = s.nf()
    first = max(0, nf - 8)
    idf = np.arange(first, first + 8, dtype=np.int32)
    zf = np.tile(np.array([[15.0, 0.1]], f32), (8, 1))
    s.profile(True)
    res = {}
    for what, kernels, call in (("innovation_summary", ("innovation_summary", "innovation_finish"), lambda: s.innovation_summary(zf, idf, tape["R"])),
                                ("map_summary", ("map_summary", "map_finish"), lambda: s.map_summary(first, 8))):
        ks, ws = [], []
        for rep in range(warm + reps):
            a = sum(s.kernel_time(k)[0] for k in kernels)
            s.timer_start()
            call()
            w = s.timer_stop()
            k = sum(s.kernel_time(k)[0] for k in kernels) - a
            if rep >= warm:
                ks.append(k), ws.append(w)
        res[what] = (statistics.median(ks), statistics.median(ws), ks, ws)
    s.profile(False)
    s.close()
    out = ["  N = %d after 200 steps, %d slots in the map, the packet names slots %d .. %d" % (N, nf, first, first + 7)]
    for what, (km, wm, ks, ws) in res.items():
        out.append("    %-18s kernels %.1f us (calls %s); whole call %.1f us (calls %s)" %
                   (what, 1e3 * km, " ".join("%.1f" % (1e3 * x) for x in ks), 1e3 * wm, " ".join("%.1f" % (1e3 * x) for x in ws)))
    out.append("    innovation / map: kernels x %.2f, whole call x %.2f" %
               (res["innovation_summary"][0] / res["map_summary"][0], res["innovation_summary"][1] / res["map_summary"][1]))
    return out + [""]


def ring_cost(tape, N, steps, arms, reps=7, warm=2):
    us = {a: [] for a in arms}
    entries = 0
    for rep in range(warm + reps):
        for arm in arms:
            s = context(tape, N)
            for f in calls(s, tape, 0, 8):  # (first launches, allocations)
                f()
            s.history_fetch()
            if arm == "on":
                s.innovation_history_enable(65536)
            todo = calls(s, tape, 8, 8 + steps)
            s.sync()
            t0 = time.perf_counter()
            for f in todo:
                f()
            s.sync()
            dt = time.perf_counter() - t0
            if rep >= warm:
                us[arm].append(1e6 * dt / steps)
            if arm == "on":
                entries = s.innovation_history_info()[1]
            s.close()
    out = []
    for arm in arms:
        out.append("  N = %d, ring %-3s  %.2f us per step (runs %s)" % (N, arm, statistics.median(us[arm]), " ".join("%.2f" % x for x in us[arm])))
    if "on" in us and "off" in us:
        off, on_ = statistics.median(us["off"]), statistics.median(us["on"])
        out.append("  -> +%.2f us per step, x %.2f (%d entries over %d steps)" % (on_ - off, on_ / off, entries, steps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--arms", nargs="*", default=["off", "on"])
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    have = hasattr(slam_amd.load_library(), "slamgpu_innovation_summary")
    arms = [x for x in a.arms if x == "off" or have]
    tape = tape_of(a.particles, a.steps + 8)
    steps = min(a.steps, len(tape["steps"]) - 8)
    lines = ["innovation_probe%s: example_webmap, FastSLAM 2, fast build, known association, host-made packets; 2 runs of warm-up, median of 7; "
             "library %s" % (" [%s]" % a.label if a.label else "", slam_amd.lib_path()), ""]
    if have:
        lines += ["(a) one slamgpu_innovation_summary call for a packet of 8, beside slamgpu_map_summary over the same 8 slots"] + one_call(tape, a.particles)
    lines += ["(b) the per-step loop: slamgpu_step over %d steps, wall time of the loop + sync, per step" % steps]
    lines += ring_cost(tape, a.particles, steps, arms)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
