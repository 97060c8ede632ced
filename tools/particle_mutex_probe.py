"""Mutual exclusion for contested landmarks (slamgpu_set_particle_mutex), in one process:

  * cost: run_particle(LISTS) at 10^5 particles on config 5 (MAX_RANGE 60) and on example_webmap, the first 60 steps: 10 of warm-up,
    5 windows of 10, two contexts alternating (mutual exclusion off / on), device events around each window; then, profiling on in a run
    of its own, the kernel's own time (slamgpu_kernel_time "particle_mutex") beside the iteration's, and the time the kernel's
    algorithmic bytes take at the rate this part copies at: per particle and observation the label read twice (8 B), the holder's word
    read, written and reset (6 B) -- 14 B; what a contest or a re-match reads on top of that is not in the yardstick;
  * effect: the whole config-5 tape, ONE run per arm, with the settings of DESIGN section 7b's spacing-rule run (10^5 particles,
    run_particle(LISTS), slot capacity 15 000, exclusion rule 2 m / 0.05 per m / ratio 2 with the spacing factor 0.5): mutual exclusion
    off; on; on with negative information (p_miss 0.5, margin 3).  Per arm the mean / final position error, the slots in use, the true
    landmarks seen during the run that the best particle covers within 1 m, its strays, the landmarks held in view and unmatched per
    particle and step (counted in every arm: p_miss = 1 where the factor is off) and the five counters.  One run per arm: a
    difference inside the run-to-run scatter section 7b reports is not an effect.

    python tools/particle_mutex_probe.py [--part cost|effect|both] [--steps 0] [--out profiles/particle_mutex.txt]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import slam_amd  # noqa: E402
from particle_excl_spacing_probe import nearest, seen_mask  # noqa: E402
from particle_lists_probe import EXCL_ON, OPT, config5_map, course, device_steps, window  # noqa: E402

K = 64                 # iterations per run_particle call
N = 100000
CAP5 = 15000
COPY_TBS = 5.0         # what this part copies at, TB/s (profiles/README.md: 4.9 - 5.3)
BYTES_PER_PAIR = 14    # per particle and observation: the label twice, the holder's word read / written / reset
COUNTERS = ("steps", "contested", "lost", "rematched", "overturned")


def context(c, cap, mutex, miss=None, spacing=0.0):
    s = slam_amd.SlamGpu(N, cap, method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         particle_maps=True, math_mode=slam_amd.MATH_FAST, log_weights=True)
    s.set_map(c["lm"])
    s.set_particle_excl_spacing(spacing)
    s.set_particle_mutex(mutex)
    if miss is not None:
        s.set_particle_miss(*miss)
    return s


def cost_of(c, cap, tag, lines, spacing=0.0, warm=10, width=10):
    opt = dict(OPT, excl=EXCL_ON, mode=slam_amd.capi.ASSOC_LISTS)
    ctxs = []
    for mutex in (0, 1):
        s = context(c, cap, mutex, spacing=spacing)
        device_steps(s, c, 0, warm, opt, width)
        s.history_fetch()
        s.particle_report_fetch()
        ctxs.append(s)
    times = [[], []]
    for w in range(5):
        lo, hi = warm + w * width, warm + (w + 1) * width
        for i in range(2):
            times[i].append(window(ctxs[i], device_steps, c, lo, hi, opt, width))
    for s in ctxs:
        s.close()
    med = [statistics.median(t) for t in times]
    # the kernel's own time: profiling on, in a run of its own
    s = context(c, cap, 1, spacing=spacing)
    s.profile(True)
    device_steps(s, c, 0, warm + 5 * width, opt, width)
    s.sync()
    kms, kn = s.kernel_time("particle_mutex")
    ams, an = s.kernel_time("associate")
    rms, rn = s.kernel_time("particle_resolve")
    st = s.particle_mutex_stats()
    nf = s.nf()
    s.close()
    out = ["  %s: run_particle(LISTS), 10^5 particles, steps %d .. %d: off %.4f ms per iteration (windows %s), on %.4f (windows %s), difference %.4f ms "
           "= %.1f %%" % (tag, warm, warm + 5 * width, med[0], " ".join("%.4f" % x for x in times[0]), med[1], " ".join("%.4f" % x for x in times[1]),
                          med[1] - med[0], 100.0 * (med[1] - med[0]) / med[0]),
           "  %s: particle_mutex %.4f ms per launch over %d launches (profiling on: event pairs around each launch); for scale associate %.4f ms, "
           "particle_resolve %.4f ms per launch; %d slots in use at the end; per particle and step: contested %.3f, lost %.3f, re-matched %.3f, "
           "overturned %.3f" % (tag, kms / max(kn, 1), kn, ams / max(an, 1), rms / max(rn, 1), nf,
                                st["contested"] / max(1, st["steps"]) / N, st["lost"] / max(1, st["steps"]) / N,
                                st["rematched"] / max(1, st["steps"]) / N, st["overturned"] / max(1, st["steps"]) / N)]
    return out, kms / max(kn, 1)


def observations_per_step(c, steps):
    lm = np.asarray(c["lm"], np.float32).reshape(2, -1)
    r = c["max_range"]
    n = []
    for k in range(steps):
        x, y, ph = (float(v) for v in c["xt"][k])
        dx, dy = lm[0] - np.float32(x), lm[1] - np.float32(y)
        n.append(int(np.sum((np.abs(dx) < r) & (np.abs(dy) < r) & (dx * np.cos(ph) + dy * np.sin(ph) > 0) & (dx.astype(float) ** 2 + dy.astype(float) ** 2 < r * r))))
    return float(np.mean(n))


def cost(lines):
    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("particle_mutex_probe cost: two contexts alternating window by window (mutual exclusion off / on), device events around each window "
        "ending in a synchronisation; exclusion rule on")
    from particle_device_probe import course as webmap_course
    with tempfile.TemporaryDirectory() as d:
        c5 = course(config5_map(d), 60)
    for c, cap, tag, spacing in ((c5, CAP5, "config 5 (MAX_RANGE %g)" % c5["max_range"], 0.5), (webmap_course(60), None, "example_webmap", 0.0)):
        out, per_launch = cost_of(c, cap or 4 * c["nlm"], tag, lines, spacing)
        nz = observations_per_step(c, 60)
        derived = nz * N * BYTES_PER_PAIR / (COPY_TBS * 1e12) * 1e3
        for ln in out:
            say(ln)
        say("  %s: %.1f observations per step x 10^5 particles x %d B at %.1f TB/s: %.4f ms -- measured / derived %.2f"
            % (tag, nz, BYTES_PER_PAIR, COPY_TBS, derived, per_launch / derived if derived > 0 else float("nan")))


def effect_arm(c, steps, name, mutex, p_miss, margin, seen):
    view = (c["max_range"] - margin, margin)
    s = context(c, CAP5, mutex, miss=(p_miss,) + view, spacing=0.5)
    opt = dict(OPT, excl=EXCL_ON, mode=slam_amd.capi.ASSOC_LISTS)
    est, reps = [], []
    t0 = time.perf_counter()
    for a in range(0, steps, K):
        device_steps(s, c, a, min(steps, a + K), opt, K)
        est.append(s.history_fetch()[0])
        reps.append(s.particle_report_fetch())
    wall = time.perf_counter() - t0
    est, rep = np.concatenate(est), np.concatenate(reps)
    xt = np.asarray(c["xt"][:steps], np.float64)
    err = np.hypot(est[:, 0] - xt[:, 0], est[:, 1] - xt[:, 1])
    best = int(np.argmax(s.download(landmarks=False)["w"]))
    d = s.download(first=best, count=1)
    ms, mx = s.particle_miss_stats(), s.particle_mutex_stats()
    s.close()
    xf = d["xf"][0][: d["nf"]]
    held = xf[~np.isnan(xf[:, 0])].astype(np.float64)
    true = np.asarray(c["lm"], np.float64).reshape(2, -1).T
    return ("  %-34s mean err %7.3f m  final %7.3f m  slots in use %5d  best particle's landmarks %5d  true seen covered within 1 m %5d of %d  stray %5d  "
            "missed per particle and step %.2f  mutual exclusion: %s  (wall %.1f s)"
            % (name, float(err.mean()), float(err[-1]), int(rep[-1][4]), len(held), int((nearest(true[seen], held) < 1.0).sum()), int(seen.sum()),
               int((nearest(held, true) >= 1.0).sum()), ms["missed"] / max(1, ms["steps"]) / N, " ".join("%s %d" % (k, mx[k]) for k in COUNTERS), wall))


def effect(a, lines):
    def say(text):
        print(text, flush=True)
        lines.append(text)
    with tempfile.TemporaryDirectory() as d:
        c = course(config5_map(d), a.steps if a.steps > 0 else None)
    steps = len(c["xt"])
    seen = seen_mask(c, steps)
    say("particle_mutex_probe effect: config 5, FastSLAM 2, %d particles, MAX_RANGE %g, %d observation steps (the tape's %s), run_particle(LISTS) K = %d, "
        "slot capacity %d, new_share 0.02, p_new 0.05, census every step, log-weights, fast build; rule: base 2 m, 0.05 per m, unique ratio 2, spacing "
        "factor 0.5; negative information counted in every arm (p_miss 1 unless stated), view %g m deep, %g m ahead.  ONE run per arm: differences "
        "inside the run-to-run scatter of DESIGN section 7b are not effects" % (N, c["max_range"], steps, "whole" if a.steps <= 0 else "first", K, CAP5,
                                                                                   c["max_range"] - a.margin, a.margin))
    for name, mutex, p in (("off", 0, 1.0), ("mutual exclusion", 1, 1.0), ("mutual exclusion, p_miss 0.5", 1, 0.5)):
        say(effect_arm(c, steps, name, mutex, p, a.margin, seen))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("cost", "effect", "both"))
    ap.add_argument("--steps", type=int, default=0, help="observation steps of the effect runs (0: the whole tape)")
    ap.add_argument("--margin", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    if a.part in ("cost", "both"):
        cost(lines)
    if a.part in ("effect", "both"):
        effect(a, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
