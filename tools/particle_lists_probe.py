"""Per-particle association through the device-built candidate lists (SLAMGPU_ASSOC_LISTS), in one process:

  * config 5 (FastSLAM 2, 10^5 particles, the synthetic 10^4-landmark map at its MAX_RANGE 60, exclusion rule off): the host-driven
    slamgpu_update_particle through the grid (today's path on that map) against slamgpu_run_particle through the lists;
  * example_webmap at 10^5 particles (exclusion rule on): slamgpu_run_particle, lists against the exhaustive scan.

Windows as in tools/particle_device_probe.py: device events on the context's stream around a window of observation steps, ending in a
synchronisation; after a warm-up the two paths alternate window by window; the median of five windows per path, in ms per step.

    python tools/particle_lists_probe.py [--out profiles/particle_lists_r08.txt] [--trace]

--trace: only run_particle through the lists on config 5, 30 iterations after the warm-up, for rocprofv3 --kernel-trace --stats;
--summarize KERNEL_TRACE_CSV: launches and copy / fill kernels per iteration of those iterations (particle_device_probe's summary)."""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import slam_amd  # noqa: E402
from slam_amd import host  # noqa: E402
from particle_device_probe import summarize  # noqa: E402

f32 = np.float32
WINDOWS = 5
OPT = dict(gate_reject=4.0, gate_augment=25.0, new_share=0.02, p_new=0.05, census_every=1)
EXCL_OFF, EXCL_ON = (0.0, 0.0, 2.0), (2.0, 0.05, 2.0)


def config5_map(d):
    """the 10 000-landmark map of BASELINE config 5 (tests/test_gpu_config5.py's recipe)"""
    lm = host.synthetic_landmarks(12345, 10000, -130, 100, -100, 90)
    h = host.HostSim(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75,
                      "-SWITCH_SEED_RANDOM", 7])
    _, wp = h.map()
    h.close()
    mp = os.path.join(d, "synthetic10k.mat")
    host.write_map(mp, lm, wp)
    open(os.path.join(d, "synthetic10k.ini"), "w").write(open(os.path.join(ROOT, "data", "example_webmap.ini")).read())
    return mp


def course(mp, steps):
    args = ["-m", mp, "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75, "-SWITCH_SEED_RANDOM", 7]
    tape = host.make_tape(args, max_obs=steps)
    sim = host.HostSim(args)
    lm, _ = sim.map()
    max_range = float(sim.conf.MAX_RANGE)
    sim.close()
    return dict(ctl=[np.array(st["controls"], f32).reshape(-1, 3) for st in tape["steps"]], xt=[np.asarray(st["true"], f32) for st in tape["steps"]],
                lm=lm, max_range=max_range, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]), nlm=tape["nlm"])


def context(c, N, cap):
    s = slam_amd.SlamGpu(N, cap, method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         particle_maps=True, math_mode=slam_amd.MATH_FAST, log_weights=True)
    s.set_map(c["lm"])
    return s


def host_steps(s, c, lo, hi, opt, K):
    for k in range(lo, hi):
        for V, G, phi in c["ctl"][k]:
            s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
        o = s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)
        if len(o["z"]):
            s.update_particle(o["z"], c["R"], **opt)
        s.estimate_async()


def device_steps(s, c, lo, hi, opt, K):
    for a in range(lo, hi, K):
        b = min(hi, a + K)
        s.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **opt)


def window(s, fn, c, lo, hi, opt, K):
    s.timer_start()
    fn(s, c, lo, hi, opt, K)
    ms = s.timer_stop()
    s.history_fetch()  # (outside the window)
    if fn is device_steps:
        s.particle_report_fetch()
    return ms / (hi - lo)


def compare(c, N, cap, a, b, warm, width, K):
    """(name, fn, opt) a against b: medians and windows"""
    sa, sb = context(c, N, cap), context(c, N, cap)
    for s, (_, fn, opt) in ((sa, a), (sb, b)):
        fn(s, c, 0, warm, opt, K)
        s.history_fetch()
        if fn is device_steps:
            s.particle_report_fetch()
    ta, tb = [], []
    for w in range(WINDOWS):
        lo, hi = warm + w * width, warm + (w + 1) * width
        ta.append(window(sa, a[1], c, lo, hi, a[2], K))
        tb.append(window(sb, b[1], c, lo, hi, b[2], K))
    stats = sb.particle_list_stats()
    sa.close()
    sb.close()
    out = []
    for (name, _, _), t in ((a, ta), (b, tb)):
        out.append("  %-34s %.4f ms per step  (windows %s)" % (name, statistics.median(t), " ".join("%.4f" % x for x in t)))
    out.append("  %-34s %.2fx; lists counters of the second: %s" % ("ratio first / second", statistics.median(ta) / statistics.median(tb), stats))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        text = summarize(a.summarize, 30)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return
    with tempfile.TemporaryDirectory() as d:
        c5 = course(config5_map(d), 60)
    lists_off = dict(OPT, mode=slam_amd.capi.ASSOC_LISTS, excl=EXCL_OFF)
    if a.trace:
        s = context(c5, 100000, 10000)
        device_steps(s, c5, 0, 10, lists_off, 10)
        s.history_fetch()
        s.particle_report_fetch()
        s.sync()
        device_steps(s, c5, 10, 40, lists_off, 30)
        s.history_fetch()
        s.close()
        print("trace run: config 5, 10^5 particles, 30 iterations through the lists after 10 of warm-up")
        return
    lines = ["particle_lists_probe: FastSLAM 2, new_share 0.02, census every step, log-weights, fast build; median of %d windows, the two paths "
             "alternating, device events around each window ending in a synchronisation" % WINDOWS, ""]
    lines.append("config 5: 10^5 particles, synthetic 10^4-landmark map, MAX_RANGE %g, slot capacity 10^4, exclusion rule off; 10 steps of "
                 "warm-up, windows of 10 steps, run_particle K = 10" % c5["max_range"])
    lines += compare(c5, 100000, 10000, ("host-driven update_particle(GRID)", host_steps, dict(OPT, mode=slam_amd.capi.ASSOC_GRID, excl=EXCL_OFF)),
                     ("run_particle(LISTS)", device_steps, lists_off), 10, 10, 10)
    web = course(os.path.join(ROOT, "data", "example_webmap.mat"), 540)
    lines.append("")
    lines.append("example_webmap: 10^5 particles, slot capacity 4 x 35, exclusion rule on; 40 steps of warm-up, windows of 100 steps, K = 20")
    lines += compare(web, 100000, 4 * web["nlm"], ("run_particle(EXHAUSTIVE)", device_steps, dict(OPT, mode=slam_amd.capi.ASSOC_EXHAUSTIVE, excl=EXCL_ON)),
                     ("run_particle(LISTS)", device_steps, dict(OPT, mode=slam_amd.capi.ASSOC_LISTS, excl=EXCL_ON)), 40, 100, 20)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
