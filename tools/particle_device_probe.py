"""Per-particle association, host-driven against device-driven (slamgpu_run_particle), on example_webmap at 512 and 10^5 particles,
in one process.

Both paths walk the same course: the host-driven twin (slamgpu_predict + slamgpu_observe + slamgpu_update_particle +
slamgpu_estimate_async per observation step) and slamgpu_run_particle with K = 20 iterations per call.  A window is 100
observation steps, bracketed by device events on the context's stream (slamgpu_timer_start / _stop: the second event is recorded
behind the window's last launch and waited for, so the window ends in a synchronisation).  After a warm-up of 40 steps on each
path the two paths alternate window by window; the median of five windows per path is reported, in ms per observation step.

    python tools/particle_device_probe.py [--out profiles/particle_device_r07.txt] [--trace]

--trace: only the device-driven path at 512 particles, 200 iterations after the warm-up (for rocprofv3 --kernel-trace
--memory-copy-trace --stats: the launches and copies of an iteration).  --summarize KERNEL_TRACE_CSV: launches and copy kernels per
iteration between the first and the last bookkeeping launch of those 200 iterations."""
import csv
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slam_amd  # noqa: E402
from slam_amd import host  # noqa: E402

f32 = np.float32
K, WINDOW, WARM, WINDOWS = 20, 100, 40, 5
OPT = dict(gate_reject=4.0, gate_augment=25.0, mode=0, new_share=0.02, p_new=0.05,
           census_every=1, excl=(2.0, 0.05, 2.0))


def course(steps):
    args = ["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75,
            "-SWITCH_SEED_RANDOM", 7]
    tape = host.make_tape(args, max_obs=steps)
    sim = host.HostSim(args)
    lm, _ = sim.map()
    max_range = float(sim.conf.MAX_RANGE)
    sim.close()
    return dict(ctl=[np.array(st["controls"], f32).reshape(-1, 3) for st in tape["steps"]], xt=[np.asarray(st["true"], f32) for st in tape["steps"]],
                lm=lm, max_range=max_range, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]), nlm=tape["nlm"])


def context(c, N):
    s = slam_amd.SlamGpu(N, 4 * c["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         particle_maps=True, math_mode=slam_amd.MATH_FAST)
    s.set_map(c["lm"])
    return s


def host_steps(s, c, lo, hi):
    for k in range(lo, hi):
        for V, G, phi in c["ctl"][k]:
            s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
        o = s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)
        if len(o["z"]):
            s.update_particle(o["z"], c["R"], **OPT)
        s.estimate_async()


def device_steps(s, c, lo, hi):
    for a in range(lo, hi, K):
        b = min(hi, a + K)
        s.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **OPT)


def window(s, fn, c, lo, hi):
    s.timer_start()
    fn(s, c, lo, hi)
    ms = s.timer_stop()
    s.history_fetch()  # (keeps the history and the report ring from filling; outside the window)
    if fn is device_steps:
        s.particle_report_fetch()
    return ms / (hi - lo)


def summarize(path, iters=200):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].split("(")[0].replace("void ", "") for r in rows]
    book = [i for i, n in enumerate(names) if n.endswith("pp_book_kernel")]
    win = names[book[-iters] + 1:book[-1] + 1]  # (bookkeeping launch to bookkeeping launch: iters - 1 whole iterations)
    n = iters - 1
    kinds = {}
    for k in win:
        kinds[k] = kinds.get(k, 0) + 1
    out = ["steady window: %d iterations (bookkeeping launch to bookkeeping launch) of the --trace run" % n,
           "kernel launches: %d = %.2f per iteration; copy / fill kernels (hipMemcpy*, hipMemset*): %d"
           % (len(win), len(win) / n, sum("copyBuffer" in k or "fillBuffer" in k for k in win))]
    out += ["  %-56s %5d  (%.2f per iteration)" % (k, v, v / n) for k, v in sorted(kinds.items(), key=lambda x: (-x[1], x[0]))]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        text = summarize(a.summarize)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return
    if a.trace:
        c = course(WARM + 200)
        s = context(c, 512)
        device_steps(s, c, 0, WARM)
        s.history_fetch()
        s.particle_report_fetch()
        s.sync()
        device_steps(s, c, WARM, WARM + 200)
        s.history_fetch()
        s.close()
        print("trace run: 512 particles, %d device-driven iterations after %d of warm-up" % (200, WARM))
        return
    c = course(WARM + WINDOWS * WINDOW)
    lines = ["particle_device_probe: example_webmap, FastSLAM 2, exclusion rule on, new_share 0.02, census every step, fast build",
             "window = %d observation steps, device events around it ending in a synchronisation; %d steps of warm-up; median of %d windows, "
             "the two paths alternating; slamgpu_run_particle with K = %d per call" % (WINDOW, WARM, WINDOWS, K), ""]
    for N, target in ((512, 0.10), (100000, 0.15)):
        sh, sd = context(c, N), context(c, N)
        host_steps(sh, c, 0, WARM)
        device_steps(sd, c, 0, WARM)
        for s in (sh, sd):
            s.history_fetch()
        sd.particle_report_fetch()
        th, td = [], []
        for w in range(WINDOWS):
            lo, hi = WARM + w * WINDOW, WARM + (w + 1) * WINDOW
            th.append(window(sh, host_steps, c, lo, hi))
            td.append(window(sd, device_steps, c, lo, hi))
        sh.close()
        sd.close()
        mh, md = statistics.median(th), statistics.median(td)
        lines.append("N = %6d  host-driven   %.4f ms per step  (windows %s)" % (N, mh, " ".join("%.4f" % x for x in th)))
        lines.append("N = %6d  device-driven %.4f ms per step  (windows %s)  target <= %.2f: %s; %.2fx the host-driven step"
                     % (N, md, " ".join("%.4f" % x for x in td), target, "met" if md <= target else "MISSED", mh / md))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
