"""The exclusion rule's radius capped by the observation spacing (slamgpu_set_particle_excl_spacing) at config 5, in one process:

  * whole: the whole config-5 tape (FastSLAM 2, 10^5 particles, the synthetic 10^4-landmark map at MAX_RANGE 60, every observation step)
    through run_particle(LISTS), arm by arm: the known-association twin (run_observe), the gates alone, the fixed rule, the spacing rule
    at each --factors value.  Per arm: mean and final position error of the estimate, slots in use and observations dropped for want
    of a slot, the best (largest-weight) particle's landmarks, how many true landmarks seen during the run have one of those within
    1 m, how many of its landmarks have no true landmark within 1 m, ms per iteration (device events around each call);
  * cost: 60 steps of the same tape, run_particle(LISTS) with the rule off against the spacing rule (f = --cost-factor), the two
    alternating window by window (tools/particle_lists_probe.py's windows); the lists' entries per observation of each, and the radius
    kernel's own time (slamgpu_kernel_time, profiling on, in a run of its own).

    python tools/particle_excl_spacing_probe.py [--part whole|cost|both] [--factors 0.5,0.75] [--steps N] [--out FILE]"""
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
from particle_lists_probe import EXCL_OFF, EXCL_ON, OPT, config5_map, course, device_steps, window  # noqa: E402

N = 100000
CAP = 15000      # slots: room for the gates alone to open duplicates of the map's 10^4 landmarks
K = 64           # iterations per run_particle call


def context(c, known):
    s = slam_amd.SlamGpu(N, c["nlm"] if known else CAP, method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5,
                         device_observe=True, particle_maps=not known, math_mode=slam_amd.MATH_FAST, log_weights=True)
    s.set_map(c["lm"])
    return s


def seen_mask(c, steps):
    """true landmarks inside the sensor's range (observe_kernel's test) at some step"""
    lm = np.asarray(c["lm"], np.float32).reshape(2, -1)
    seen = np.zeros(lm.shape[1], bool)
    r = c["max_range"]
    for k in range(steps):
        x, y, ph = (float(v) for v in c["xt"][k])
        dx, dy = lm[0] - np.float32(x), lm[1] - np.float32(y)
        seen |= (np.abs(dx) < r) & (np.abs(dy) < r) & (dx * np.cos(ph) + dy * np.sin(ph) > 0) & (dx.astype(float) ** 2 + dy.astype(float) ** 2 < r * r)
    return seen


def nearest(a, b):
    """for each row of a [n,2], the distance to the nearest row of b [m,2]"""
    out = np.full(len(a), np.inf)
    for i in range(0, len(a), 256):
        d = np.hypot(a[i:i + 256, None, 0] - b[None, :, 0], a[i:i + 256, None, 1] - b[None, :, 1])
        out[i:i + 256] = d.min(1) if b.shape[0] else np.inf
    return out


def whole_arm(c, steps, name, opt, f, seen):
    known = opt is None
    s = context(c, known)
    if not known:
        s.set_particle_excl_spacing(f)
    est, reps, ms = [], [], 0.0
    t0 = time.perf_counter()
    for a in range(0, steps, K):
        b = min(steps, a + K)
        s.timer_start()
        if known:
            s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)
        else:
            s.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **opt)
        ms += s.timer_stop()
        est.append(s.history_fetch()[0])
        if not known:
            reps.append(s.particle_report_fetch())
    wall = time.perf_counter() - t0
    est = np.concatenate(est)
    xt = np.asarray(c["xt"][:steps], np.float64)
    err = np.hypot(est[:, 0] - xt[:, 0], est[:, 1] - xt[:, 1])
    w = s.download(landmarks=False)["w"]
    best = int(np.argmax(w))
    d = s.download(first=best, count=1)
    s.close()
    xf = d["xf"][0][: d["nf"]]
    held = xf[~np.isnan(xf[:, 0])].astype(np.float64)
    true = np.asarray(c["lm"], np.float64).reshape(2, -1).T
    covered = int((nearest(true[seen], held) < 1.0).sum())
    stray = int((nearest(held, true) >= 1.0).sum())
    line = ("  %-22s mean err %7.3f m  final %7.3f m  best particle's landmarks %5d  true seen covered within 1 m %5d of %d  stray %5d  "
            % (name, float(err.mean()), float(err[-1]), len(held), covered, int(seen.sum()), stray))
    if known:
        line += "slots %5d (known association)" % d["nf"]
    else:
        rep = np.concatenate(reps)
        line += "slots in use %5d  opened %6d  dropped %6d" % (int(rep[-1][4]), int(rep[:, 1].sum()), int(rep[:, 3].sum()))
    line += "  %.3f ms/iteration (device events; wall %.1f s)" % (ms / steps, wall)
    print(line, flush=True)
    return line


def cost(c, f, warm=10, width=10):
    lists = dict(OPT, mode=slam_amd.capi.ASSOC_LISTS)
    arms = (("rule off", dict(lists, excl=EXCL_OFF), 0.0), ("spacing rule f = %g" % f, dict(lists, excl=EXCL_ON), f))
    ctxs = []
    for _, opt, fa in arms:
        s = context(c, False)
        s.set_particle_excl_spacing(fa)
        device_steps(s, c, 0, warm, opt, width)
        s.history_fetch()
        s.particle_report_fetch()
        ctxs.append(s)
    times = [[], []]
    for w in range(5):
        lo, hi = warm + w * width, warm + (w + 1) * width
        for i, (_, opt, _) in enumerate(arms):
            times[i].append(window(ctxs[i], device_steps, c, lo, hi, opt, width))
    out = []
    for i, (name, _, _) in enumerate(arms):
        st = ctxs[i].particle_list_stats()
        out.append("  run_particle(LISTS), %-22s %.4f ms per iteration (windows %s); lists: %.1f entries per step, %d steps, overflowed %d"
                   % (name, statistics.median(times[i]), " ".join("%.4f" % x for x in times[i]), st["entries"] / max(st["steps"], 1), st["steps"],
                      st["overflowed"]))
        ctxs[i].close()
    out.append("  ratio spacing / off: %.3f" % (statistics.median(times[1]) / statistics.median(times[0])))
    # the radius kernel's own time: profiling on, in a run of its own
    s = context(c, False)
    s.set_particle_excl_spacing(f)
    s.profile(True)
    device_steps(s, c, 0, warm + 5 * width, dict(lists, excl=EXCL_ON), width)
    s.sync()
    kms, kn = s.kernel_time("excl_radii")
    ams, an = s.kernel_time("associate")
    bms, bn = s.kernel_time("assoc_lists")
    s.close()
    out.append("  radius kernel (excl_radii): %.4f ms per launch over %d launches; for scale the walk (associate) %.4f ms, the lists (assoc_lists) "
               "%.4f ms per launch (profiling on: event pairs around each launch)" % (kms / max(kn, 1), kn, ams / max(an, 1), bms / max(bn, 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("whole", "cost", "both"))
    ap.add_argument("--factors", default="0.5,0.75")
    ap.add_argument("--cost-factor", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=0, help="observation steps of the whole run (0: the whole tape)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        mp = config5_map(d)
        c = course(mp, a.steps if a.steps > 0 else None)
    steps = len(c["xt"])
    lines = []
    if a.part in ("whole", "both"):
        lines.append("particle_excl_spacing_probe whole: config 5, FastSLAM 2, %d particles, MAX_RANGE %g, %d observation steps (the tape's %s), "
                     "run_particle(LISTS) K = %d, slot capacity %d, new_share 0.02, p_new 0.05, census every step, log-weights, fast build; "
                     "rule: base 2 m, 0.05 per m, unique ratio 2" % (N, c["max_range"], steps, "whole" if a.steps <= 0 else "first", K, CAP))
        print(lines[-1], flush=True)
        seen = seen_mask(c, steps)
        lists = dict(OPT, mode=slam_amd.capi.ASSOC_LISTS)
        lines.append(whole_arm(c, steps, "known association", None, 0.0, seen))
        lines.append(whole_arm(c, steps, "gates alone", dict(lists, excl=EXCL_OFF), 0.0, seen))
        lines.append(whole_arm(c, steps, "fixed rule", dict(lists, excl=EXCL_ON), 0.0, seen))
        for f in (float(x) for x in a.factors.split(",")):
            lines.append(whole_arm(c, steps, "spacing rule f = %g" % f, dict(lists, excl=EXCL_ON), f, seen))
    if a.part in ("cost", "both"):
        cc = course_first(c, 60)
        lines.append("particle_excl_spacing_probe cost: config 5, %d particles, the first 60 steps: 10 of warm-up, 5 windows of 10, the two "
                     "contexts alternating, device events around each window ending in a synchronisation" % N)
        print(lines[-1], flush=True)
        for ln in cost(cc, a.cost_factor):
            print(ln, flush=True)
            lines.append(ln)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def course_first(c, n):
    return dict(c, ctl=c["ctl"][:n], xt=c["xt"][:n])


if __name__ == "__main__":
    main()
