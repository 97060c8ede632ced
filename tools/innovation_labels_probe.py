"""Cost of the innovation posterior with every particle's own match (slamgpu_innovation_summary_labels, and the ring entries
slamgpu_update_particle records by itself), in one process, example_webmap, FastSLAM 2, fast build, per-particle association with the
observation made on the device and the step driven by the host (tools/innovation_probe.py is the known-association twin of this file):

  (a) one slamgpu_innovation_summary_labels call for 8 observations at 10^5 particles after 60 steps of the course, beside
      slamgpu_innovation_summary over the same 8 slots on the same context: unanimous labels (the same records read), and labels drawn
      per particle over all slots (divergent gathers).  The kernels' time between event pairs (slamgpu_profile / slamgpu_kernel_time)
      and the whole call between two events (the new call's includes the labels' way down: N x 8 words through pinned memory);
      2 calls of warm-up, median of 7.
  (b) the per-step loop: predicts + slamgpu_observe + slamgpu_update_particle + slamgpu_estimate_async over a window of observation
      steps (default 150) with the ring on against the same loop with it off (fresh contexts of the same seed, the arms taken in turn).
      Wall time of the loop + a synchronisation, per step; 2 runs of warm-up, median of 7.

  (c) --whole-run N ...: the whole course with the ring on; mean mixture NIS, the share of entries under 5.9915, the mean share and the
      share-0 entries, as slam-backend's end-of-run line gives them for the other associations.

A library without the entry point (the parent commit's, loaded through SLAMGPU_LIB for an A/B) runs the ring-off arm only: take the two
libraries in turn, process by process.

    python tools/innovation_labels_probe.py [--out profiles/innovation.txt] [--steps 150] [--particles 100000] [--arms off on] [--label text]"""
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
OPT = dict(gate_reject=4.0, gate_augment=25.0, mode=0, new_share=0.02, p_new=0.05, census_every=1, excl=(2.0, 0.05, 2.0))


def course_of(steps):
    args = ["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75, "-SWITCH_SEED_RANDOM", 7]
    tape = host.make_tape(args, max_obs=steps)
    sim = host.HostSim(args)
    lm, _ = sim.map()
    max_range = float(sim.conf.MAX_RANGE)
    sim.close()
    return dict(ctl=[np.array(st["controls"], f32).reshape(-1, 3) for st in tape["steps"]], xt=[np.asarray(st["true"], f32) for st in tape["steps"]], lm=lm,
                max_range=max_range, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]), nlm=tape["nlm"])


def context(c, N):
    s = slam_amd.SlamGpu(N, c["nlm"] * 4, method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, math_mode=slam_amd.MATH_FAST,
                         device_observe=True, particle_maps=True)
    s.set_map(c["lm"])
    return s


def step(s, c, k):
    for V, G, phi in c["ctl"][k]:
        s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
    o = s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)
    if len(o["z"]):
        s.update_particle(o["z"], c["R"], **OPT)
    s.estimate_async()
    return len(o["z"])


def one_call(c, N, reps=7, warm=2):
    s = context(c, N)
    for k in range(60):
        step(s, c, k)
    s.history_fetch()
    nf = s.nf()
    first = max(0, nf - 8)
    idf = np.arange(first, first + 8, dtype=np.int32)
    z = np.tile(np.array([[15.0, 0.1]], f32), (8, 1))
    same = np.ascontiguousarray(np.tile(idf, (N, 1)))
    mixed = np.random.default_rng(1).integers(-2, nf, (N, 8)).astype(np.int32)
    s.profile(True)
    res = {}
    for what, kernels, call in (("labels, unanimous", ("innovation_summary_labels", "innovation_finish"), lambda: s.innovation_summary_labels(z, same, c["R"])),
                                ("labels, per particle", ("innovation_summary_labels", "innovation_finish"), lambda: s.innovation_summary_labels(z, mixed, c["R"])),
                                ("known association", ("innovation_summary", "innovation_finish"), lambda: s.innovation_summary(z, idf, c["R"]))):
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
    out = ["  N = %d after 60 per-particle steps, %d slots in use, the observations name slots %d .. %d (per particle: any of -2 .. %d)" % (N, nf, first, first + 7, nf - 1)]
    for what, (km, wm, ks, ws) in res.items():
        out.append("    %-22s kernels %.1f us (calls %s); whole call %.1f us (calls %s)" %
                   (what, 1e3 * km, " ".join("%.1f" % (1e3 * x) for x in ks), 1e3 * wm, " ".join("%.1f" % (1e3 * x) for x in ws)))
    kn = res["known association"]
    for what in ("labels, unanimous", "labels, per particle"):
        out.append("    %s / known association: kernels x %.2f, whole call x %.2f" % (what, res[what][0] / kn[0], res[what][1] / kn[1]))
    return out + [""]


def ring_cost(c, N, steps, arms, reps=7, warm=2):
    us = {a: [] for a in arms}
    entries = 0
    for rep in range(warm + reps):
        for arm in arms:
            s = context(c, N)
            for k in range(8):  # (first launches, allocations)
                step(s, c, k)
            s.history_fetch()
            if arm == "on":
                s.innovation_history_enable(65536)
            s.sync()
            t0 = time.perf_counter()
            for k in range(8, 8 + steps):
                step(s, c, k)
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
        out.append("  -> +%.2f us per step, x %.3f (%d entries over %d steps)" % (on_ - off, on_ / off, entries, steps))
    return out


def whole_run(c, N):
    """every observation step of the course with the ring on: the figures slam-backend's end-of-run line gives for the other associations"""
    steps = len(c["ctl"])
    s = context(c, N)
    s.innovation_history_enable(65536)
    for k in range(steps):
        step(s, c, k)
        if k % 512 == 511:
            s.history_fetch()
    first, nxt, cap, recs = s.innovation_history_info()
    ent, rec, slot = s.innovation_history_fetch()
    nis, bad = host.innovation_nis(ent)
    ok = ~np.isnan(nis)
    line = ("  N = %d, %d observation steps, %d records: %d entries summarised, %d retained; mean mixture NIS %.4f, NIS <= 5.9915 in %.4f of the "
            "entries; mean per-particle NIS %.4f; mean share %.4f; %d share-0 entries; %d bad entries; %d slots in use at the end" %
            (N, steps, recs, nxt, nxt - first, nis[ok].mean(), (nis[ok] <= 5.9915).mean(), np.nanmean(ent[:, 9]), np.nanmean(ent[:, 0]),
             int((ent[:, 0] == 0).sum()), bad, s.nf()))
    s.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--arms", nargs="*", default=["off", "on"])
    ap.add_argument("--label", default="")
    ap.add_argument("--whole-run", type=int, nargs="*", default=[], metavar="N", help="(c) the whole course with the ring on at these particle counts")
    a = ap.parse_args()
    have = hasattr(slam_amd.load_library(), "slamgpu_innovation_summary_labels")
    arms = [x for x in a.arms if x == "off" or have]
    c = course_of(10 ** 6 if a.whole_run else max(a.steps + 8, 60))
    steps = min(a.steps, len(c["ctl"]) - 8)
    lines = ["innovation_labels_probe%s: example_webmap, FastSLAM 2, fast build, per-particle association (host-driven steps, device-made "
             "observations); 2 runs of warm-up, median of 7; library %s" % (" [%s]" % a.label if a.label else "", slam_amd.lib_path()), ""]
    if have and "on" in arms:
        lines += ["(a) one slamgpu_innovation_summary_labels call for 8 observations, beside slamgpu_innovation_summary over the same 8 slots"] + one_call(c, a.particles)
    lines += ["(b) the per-step loop: predicts + observe + slamgpu_update_particle + estimate over %d steps, wall time of the loop + sync, per step" % steps]
    lines += ring_cost(c, a.particles, steps, arms)
    if have and a.whole_run:
        lines += ["", "(c) whole run, seed 7, rule on, new_share 0.02, gates 4 / 25: the ring's entries through slamhost_innovation_nis"]
        lines += [whole_run(c, N) for N in a.whole_run]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
