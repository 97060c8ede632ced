"""Negative information for the per-particle steps (slamgpu_set_particle_miss), in one process:

  * whole: whole runs with the factor off / count only (p_miss = 1) / on, beside each other.  example_webmap, FastSLAM 2, fast build,
    run_particle with the exclusion rule on, --seeds x --particles contexts, the view MAX_RANGE - margin deep and margin ahead; per run
    the mean position error, the best (largest-weight) particle's landmarks, how many true landmarks seen during the run have one of
    them within 1 m, how many of them have no true landmark within 1 m (stray), and from slamgpu_map_summary the slots held by at least
    half of the weight / by less than half (minority) / by nobody (dead); --config5: one config-5 tape per arm as well
    (tools/particle_excl_spacing_probe.py's whole run, spacing rule f = 0.5);
  * cost: run_particle(LISTS) at 10^5 particles on example_webmap and on config 5 (MAX_RANGE 60), the first 60 steps: 10 of warm-up,
    5 windows of 10, two contexts alternating (factor off / count only), device events around each window; then, profiling on in a run
    of its own, the kernel's own time (slamgpu_kernel_time "particle_missed"), the records it looked at per particle and step, and the
    time those bytes take at the rate this part copies at.

    python tools/particle_miss_probe.py [--part whole|cost|both] [--seeds 7..16] [--particles 512,2048] [--p 1,0.5,0.1] [--margin 3]
                                        [--config5] [--out FILE]"""
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
COPY_TBS = 5.0         # what this part copies at, TB/s (profiles/README.md: 4.9 - 5.3)
BYTES_PER_VISIT = 26   # 20 B record + 4 B genealogy entry + 2 B claim: the issue's yardstick per (particle, slot) looked at


def context(c, N, cap, seed, miss):
    s = slam_amd.SlamGpu(N, cap, method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=seed, device_observe=True,
                         particle_maps=True, math_mode=slam_amd.MATH_FAST, log_weights=True)
    s.set_map(c["lm"])
    if miss is not None:
        s.set_particle_miss(*miss)
    return s


def whole_run(c, N, cap, seed, miss, opt, seen, spacing=0.0):
    steps = len(c["xt"])
    s = context(c, N, cap, seed, miss)
    s.set_particle_excl_spacing(spacing)
    est, reps = [], []
    for a in range(0, steps, K):
        device_steps(s, c, a, min(steps, a + K), opt, K)
        est.append(s.history_fetch()[0])
        reps.append(s.particle_report_fetch())
    est, rep = np.concatenate(est), np.concatenate(reps)
    xt = np.asarray(c["xt"][:steps], np.float64)
    err = np.hypot(est[:, 0] - xt[:, 0], est[:, 1] - xt[:, 1])
    best = int(np.argmax(s.download(landmarks=False)["w"]))
    d = s.download(first=best, count=1)
    share = np.concatenate([s.map_summary(a, min(4096, d["nf"] - a))["share"] for a in range(0, d["nf"], 4096)]) if d["nf"] else np.zeros(0)
    st = s.particle_miss_stats()
    s.close()
    xf = d["xf"][0][: d["nf"]]
    held = xf[~np.isnan(xf[:, 0])].astype(np.float64)
    true = np.asarray(c["lm"], np.float64).reshape(2, -1).T
    return dict(err=float(err.mean()), best=len(held), covered=int((nearest(true[seen], held) < 1.0).sum()), stray=int((nearest(held, true) >= 1.0).sum()),
                confident=int((share >= 0.5).sum()), minority=int(((share > 0) & (share < 0.5)).sum()), dead=int((share == 0).sum()),
                slots=int(rep[-1][4]), missed=st["missed"], steps=st["steps"])


def fmt(r):
    return "err %6.3f m  best %3d  covered %3d  stray %3d | posterior: half+ %3d  minority %3d  dead %3d | slots %4d  missed/particle/step %.3f" % (
        r["err"], r["best"], r["covered"], r["stray"], r["confident"], r["minority"], r["dead"], r["slots"], r["missed_rate"])


def whole(a, lines):
    def say(text):
        print(text, flush=True)
        lines.append(text)
    from particle_device_probe import course as webmap_course  # (example_webmap's whole tape)
    c = webmap_course(None)
    steps = len(c["xt"])
    seen = seen_mask(c, steps)
    view = (c["max_range"] - a.margin, a.margin)
    arms = [("off", None)] + [("count only" if p == 1.0 else "p_miss %g" % p, (p,) + view) for p in a.p]
    opt = dict(OPT, excl=EXCL_ON)
    say("particle_miss_probe whole: example_webmap, FastSLAM 2, fast build, log-weights, %d observation steps, run_particle K = %d, slot capacity %d, "
        "exclusion rule base 2 m / 0.05 per m / ratio 2, new_share 0.02, p_new 0.05, census every step; view: closer than %g m, more than %g m ahead; "
        "%d true landmarks seen during the run" % (steps, K, 4 * c["nlm"], view[0], view[1], int(seen.sum())))
    for N in a.particles:
        totals = {name: [] for name, _ in arms}
        for seed in a.seeds:
            for name, miss in arms:
                r = whole_run(c, N, 4 * c["nlm"], seed, miss, opt, seen)
                r["missed_rate"] = r["missed"] / max(1, r["steps"]) / N
                totals[name].append(r)
                say("  N %5d seed %2d %-11s %s" % (N, seed, name, fmt(r)))
        for name, _ in arms:
            t = totals[name]
            say("  N %5d all %d seeds %-11s mean err %6.3f m  mean best %5.1f  mean covered %5.1f  stray: total %3d, runs with any %2d  minority total %3d  "
                "dead total %3d" % (N, len(t), name, statistics.mean(r["err"] for r in t), statistics.mean(r["best"] for r in t),
                                    statistics.mean(r["covered"] for r in t), sum(r["stray"] for r in t), sum(1 for r in t if r["stray"]),
                                    sum(r["minority"] for r in t), sum(r["dead"] for r in t)))
    if a.config5:
        with tempfile.TemporaryDirectory() as d:
            c5 = course(config5_map(d), a.config5_steps if a.config5_steps > 0 else None)
        steps = len(c5["xt"])
        seen = seen_mask(c5, steps)
        view = (c5["max_range"] - a.margin, a.margin)
        say("particle_miss_probe whole: config 5 (10^4 landmarks, MAX_RANGE %g), 10^5 particles, %d observation steps, run_particle(LISTS), slot capacity "
            "15000, spacing rule f = 0.5; %d true landmarks seen" % (c5["max_range"], steps, int(seen.sum())))
        for name, miss in [("off", None)] + [("count only" if p == 1.0 else "p_miss %g" % p, (p,) + view) for p in a.p]:
            t0 = time.perf_counter()
            r = whole_run(c5, 100000, 15000, 5, miss, dict(OPT, excl=EXCL_ON, mode=slam_amd.capi.ASSOC_LISTS), seen, spacing=0.5)
            r["missed_rate"] = r["missed"] / max(1, r["steps"]) / 100000
            say("  config 5 %-11s %s  (wall %.1f s)" % (name, fmt(r), time.perf_counter() - t0))


def cost_of(c, cap, tag, margin, lines, warm=10, width=10):
    N = 100000
    opt = dict(OPT, excl=EXCL_ON, mode=slam_amd.capi.ASSOC_LISTS)
    view = (c["max_range"] - margin, margin)
    arms = (("factor off", None), ("count only", (1.0,) + view))
    ctxs = []
    for _, miss in arms:
        s = context(c, N, cap, 5, miss)
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
    s = context(c, N, cap, 5, arms[1][1])
    s.profile(True)
    device_steps(s, c, 0, warm + 5 * width, opt, width)
    s.sync()
    kms, kn = s.kernel_time("particle_missed")
    rms, rn = s.kernel_time("particle_resolve")
    st = s.particle_miss_stats()
    nf = s.nf()
    s.close()
    per = st["visited"] / max(1, st["steps"]) / N
    derived = per * N * BYTES_PER_VISIT / (COPY_TBS * 1e12) * 1e3
    out = ["  %s: run_particle(LISTS), 10^5 particles, steps %d .. %d: factor off %.4f ms per iteration (windows %s), count only %.4f (windows %s), "
           "difference %.4f ms = %.1f %%" % (tag, warm, warm + 5 * width, med[0], " ".join("%.4f" % x for x in times[0]), med[1],
                                             " ".join("%.4f" % x for x in times[1]), med[1] - med[0], 100.0 * (med[1] - med[0]) / med[0]),
           "  %s: particle_missed %.4f ms per launch over %d launches (profiling on: event pairs around each launch); %.1f records looked at per "
           "particle and step of %d slots in use at the end (missed per particle and step %.3f); %d B per record at %.1f TB/s: %.4f ms -- measured / "
           "derived %.2f; for scale particle_resolve %.4f ms per launch" % (tag, kms / max(kn, 1), kn, per, nf, st["missed"] / max(1, st["steps"]) / N,
                                                                              BYTES_PER_VISIT, COPY_TBS, derived,
                                                                              (kms / max(kn, 1)) / derived if derived > 0 else float("nan"), rms / max(rn, 1))]
    for ln in out:
        print(ln, flush=True)
        lines.append(ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("whole", "cost", "both"))
    ap.add_argument("--seeds", default="7..16")
    ap.add_argument("--particles", default="512,2048")
    ap.add_argument("--p", default="1,0.5,0.1")
    ap.add_argument("--margin", type=float, default=3.0)
    ap.add_argument("--config5", action="store_true")
    ap.add_argument("--config5-steps", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lo, hi = (int(v) for v in a.seeds.split(".."))
    a.seeds = list(range(lo, hi + 1))
    a.particles = [int(v) for v in a.particles.split(",")]
    a.p = [float(v) for v in a.p.split(",")]
    lines = []
    if a.part in ("cost", "both"):
        lines.append("particle_miss_probe cost: two contexts alternating window by window, device events around each window ending in a synchronisation")
        print(lines[-1], flush=True)
        from particle_device_probe import course as webmap_course
        cw = webmap_course(60)
        cost_of(cw, 4 * cw["nlm"], "example_webmap", a.margin, lines)
        with tempfile.TemporaryDirectory() as d:
            c5 = course(config5_map(d), 60)
        cost_of(c5, 15000, "config 5 (MAX_RANGE %g)" % c5["max_range"], a.margin, lines)
    if a.part in ("whole", "both"):
        whole(a, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
