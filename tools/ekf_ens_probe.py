"""The numbers of DESIGN.md section 7i (not a test): the device EKF ensemble (slamgpu_ens_*) on the bundled maps, beside B host
filters and beside the single device filter, taken in the same visit.  Appends to profiles/ekf_ensemble.txt (or --out).

    python tools/ekf_ens_probe.py [--out profiles/ekf_ensemble.txt] [--members 1,64,256,1024,4096] [--nees-members 1024]

Per map the simulator runs once without its own control and sensor noise and the tape (true controls, true heading, noise-free
observations, visible ids, true pose) is replayed through slamgpu_ens_sim_noise for every B, twice on fresh handles: once
pipelined (the whole run enqueued, one synchronisation at the end: the time per control step and the filter-steps per second) and
once with a synchronisation after every step (the time of a control step and of an observation step apart).  The first 200 steps of
a third handle run untimed before either.  The baselines: slamhost_ekf_step on one core (per control step, times B), and
slamgpu_ekf_sim fed the host run's tape.

    python tools/ekf_ens_probe.py --batch 1,16,64,256,1024 [--out profiles/ekf_ensemble_run.txt] [--members 1,64,256,1024,4096]

The batch table of slamgpu_ens_run_noise instead: us per control step of the whole ensemble with the run enqueued in batches of K steps
and one synchronisation at the end, the median of five runs after a warm-up run, smallest and largest beside it.  K = 1 is the loop of
slamgpu_ens_sim_noise calls, the comparison, taken in the same session; a library without slamgpu_ens_run_noise (an older build
selected with SLAMGPU_LIB) gives that column alone.

    python tools/ekf_ens_probe.py --moments [--out profiles/ens_moments.txt] [--members 256,1024,4096] [--maps example_webmap,example_loop1] [--calls 20]

slamgpu_ens_moments at the end of each map's run with the known association (D = the whole state): the whole call (a host clock around
it; the call ends in a synchronisation), with and without Pbar and C, the median of --calls calls after three; beside it what the same
answer costs without it, one slamgpu_ens_state per member and numpy (this needs nothing of the new entry point, so it is the parent's
cost too), and how far the two answers are apart.  At B = --nees-members the findings: moments_summary against the true pose and map,
with the known association and, for the pose alone (D = 3), with the gates.

    rocprofv3 --kernel-trace -d DIR -- python tools/ekf_ens_probe.py --moments --members 4096 --maps example_webmap --calls 20 --out /dev/null
    python tools/ekf_ens_probe.py --moments-kernels DIR --calls 20 [--out profiles/ens_moments.txt]

The kernels of those calls, from the trace of a run of its own: per ekf_ens_mom_* kernel the launches and the mean time per CALL (the
warm-up calls and the findings' calls counted in: DIR's total over all of them), and the mean-of-P pass's bytes over its time.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32
MAPS = (("example_webmap", 7), ("example_loop1", 3))
HEADROOM = 8  # landmarks more than the map has, as slam-backend -runs allocates: what the gates open besides must not cost a step's update


def cfg_of(c):
    return dict(use_heading=c.SWITCH_HEADING_KNOWN == 1, batch_update=c.SWITCH_BATCH_UPDATE == 1, association_known=c.SWITCH_ASSOCIATION_KNOWN != 0,
                wheel_base=c.WHEELBASE, sigma_phi=c.sigmaT, gate_reject=c.GATE_REJECT, gate_augment=c.GATE_AUGMENT)


def record(host, name, seed, extra=()):
    """the noise-free tape of a run, and what its settings say about the noise"""
    m = os.path.join(ROOT, "data", name + ".mat")
    user = host.HostSim(["-m", m, "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed, *extra])
    flags = (1 if user.conf.SWITCH_CONTROL_NOISE else 0) | 2 | (4 if user.conf.SWITCH_SENSOR_NOISE else 0)
    user.close()
    sim = host.HostSim(["-m", m, "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed, "-SWITCH_CONTROL_NOISE", 0, "-SWITCH_SENSOR_NOISE", 0, *extra])
    tape = []
    while True:
        r, _, _, phi = sim.control()
        if r < 0:
            break
        V, G = sim.true_controls()
        z, vis = (None, None)
        if r == 1:
            sim.observe(0)
            z, vis = sim.last_z()
        tape.append((r, V, G, phi, z, vis, sim.true_pose()))
    out = dict(tape=tape, conf=sim.conf, nlm=sim.nlm, noise=sim.sim_noise(), flags=flags, lm=sim.map()[0].astype(np.float64))
    sim.close()
    return out


def replay(ens, rec, steps=None, sync_each=False):
    nz, t_ctl, t_obs = rec["noise"], 0.0, 0.0
    t0 = time.perf_counter()
    for k, (r, V, G, phi, z, vis, xt) in enumerate(rec["tape"][:steps]):
        t1 = time.perf_counter()
        ens.sim_noise(V, G, phi, nz["Q"], nz["dt"], k, z, vis, nz["Re"], nz["R"], r, truth=xt, Qe=nz["Qe"], noise=rec["flags"])
        if sync_each:
            ens.sync()
            if r:
                t_obs += time.perf_counter() - t1
            else:
                t_ctl += time.perf_counter() - t1
    ens.sync()
    return time.perf_counter() - t0, t_ctl, t_obs


def packed(slam_amd, rec, K):
    """the tape in batches of K steps, as run_noise takes them (made once, outside the timed region)"""
    nz, out = rec["noise"], []
    dicts = [dict(V=V, G=G, phi_true=phi, dt=nz["dt"], step=k, truth=xt, observe=int(r), z_true=z, ids=vis)
             for k, (r, V, G, phi, z, vis, xt) in enumerate(rec["tape"])]
    for at in range(0, len(dicts), K):
        out.append(slam_amd.pack_tape(dicts[at:at + K]))
    return out


def replay_batches(ens, rec, batches):
    nz = rec["noise"]
    t0 = time.perf_counter()
    for steps, z_true, ids in batches:
        ens.run_noise(steps, z_true, ids, nz["Q"], nz["Re"], nz["R"], Qe=nz["Qe"], noise=rec["flags"])
    ens.sync()
    return time.perf_counter() - t0


def batch_table(slam_amd, host, a, say):
    has_run = hasattr(slam_amd.load_library(), "slamgpu_ens_run_noise")
    Ks = [int(k) for k in a.batch.split(",") if int(k) == 1 or has_run]
    say("# tools/ekf_ens_probe.py --batch %s --members %s   library %s%s" % (a.batch, a.members, "SLAMGPU_LIB" if os.environ.get("SLAMGPU_LIB") else os.path.relpath(slam_amd.lib_path(), ROOT),
                                                                          "" if has_run else " (no slamgpu_ens_run_noise: K = 1 only)"))
    say("# us per control step of the whole ensemble, pipelined, one synchronisation at the end: median of 5 runs after a warm-up run [smallest .. largest]")
    for name, seed in MAPS:
        rec = record(host, name, seed)
        n = len(rec["tape"])
        say("%s seed %d: %d control steps, %d with an observation, noise flags %d" % (name, seed, n, sum(1 for t in rec["tape"] if t[0]), rec["flags"]))
        say("    %6s " % "B" + " ".join("%28s" % ("K = %d" % K) for K in Ks))
        tapes = {K: packed(slam_amd, rec, K) for K in Ks if K > 1}
        for B in (int(b) for b in a.members.split(",")):
            cells = []
            for K in Ks:
                times = []
                for rep in range(6):
                    e = slam_amd.EkfEnsemble(B, rec["nlm"] + HEADROOM, **cfg_of(rec["conf"]), seed=seed)
                    t = replay(e, rec)[0] if K == 1 else replay_batches(e, rec, tapes[K])
                    e.close()
                    if rep:
                        times.append(1e6 * t / n)
                cells.append("%9.2f [%7.2f .. %7.2f]" % (float(np.median(times)), min(times), max(times)))
            say("    %6d " % B + " ".join("%28s" % c for c in cells))


def pbar_bytes(n, D):
    """what the mean-of-P pass reads: per member and row r the 16-byte loads that reach into the lower triangle, r // 4 + 1 of them"""
    return n * 16 * sum(r // 4 + 1 for r in range(D))


def moments_table(slam_amd, host, a, say):
    calls = a.calls

    def timed(call):
        for _ in range(3):
            call()
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            ts.append(1e6 * (time.perf_counter() - t0))
        return float(np.median(ts)), min(ts), max(ts)

    say("# tools/ekf_ens_probe.py --moments --members %s --maps %s --calls %d" % (a.members, a.maps, calls))
    say("# slamgpu_ens_moments at the end of the run, known association, D = the whole state; us per call, host clock, median of %d after 3 [smallest .. largest]" % calls)
    for name, seed in MAPS:
        if name not in a.maps.split(","):
            continue
        rec = record(host, name, seed, ("-SWITCH_ASSOCIATION_KNOWN", 1))
        order = []
        for t in rec["tape"]:
            if t[0]:
                order += [int(i) for i in t[5] if int(i) not in order]
        xt = rec["tape"][-1][6]
        say("%s seed %d: %d control steps, %d landmarks, sigmaT %.6g" % (name, seed, len(rec["tape"]), rec["nlm"], rec["conf"].sigmaT))
        for B in (int(b) for b in a.members.split(",")):
            e = slam_amd.EkfEnsemble(B, rec["nlm"], **cfg_of(rec["conf"]), seed=seed)
            replay(e, rec)
            dims = e.dims()
            D = int(dims.min())
            full, noP, noC, mean_only = (timed(lambda kw=kw: e.moments(D, **kw)) for kw in
                                         ({}, dict(want_Pbar=False), dict(want_C=False), dict(want_C=False, want_Pbar=False)))
            m = e.moments(D)
            t0 = time.perf_counter()
            xs, Ps = zip(*(e.state(b) for b in range(B)))
            t1 = time.perf_counter()
            xs, Ps = np.stack([x[:D] for x in xs]).astype(np.float64), np.stack([P[:D, :D] for P in Ps]).astype(np.float64)
            v = xs - xs[0]
            v[:, 2] = np.remainder(v[:, 2] + np.pi, 2 * np.pi) - np.pi
            Cn, Pn = np.cov(v.T, bias=True), Ps.mean(0)
            t2 = time.perf_counter()
            say("    B %5d D %3d (dims %d .. %d, status bits in %d members): whole call %8.1f [%7.1f .. %7.1f]   without Pbar %8.1f   without C %8.1f   mean alone %8.1f" %
                (B, D, dims.min(), dims.max(), int((e.status() != 0).sum()), *full, noP[0], noC[0], mean_only[0]))
            say("          the same from B slamgpu_ens_state calls + numpy: %10.1f us of copies + %9.1f us of numpy = x %.0f the whole call; "
                "largest |C - numpy| / max |C| %.2e, |Pbar - numpy| / max |Pbar| %.2e; counted %d, the mean-of-P pass reads %.2f MB (the slabs' [0, D) x ld: %.2f MB)" %
                (1e6 * (t1 - t0), 1e6 * (t2 - t1), 1e6 * (t2 - t0) / full[0], np.abs(m["C"] - Cn).max() / np.abs(Cn).max(),
                 np.abs(m["Pbar"] - Pn).max() / np.abs(Pn).max(), m["counted"], pbar_bytes(m["counted"], D) / 1e6, m["counted"] * D * e.ld * 4 / 1e6))
            if B == a.nees_members:
                s = slam_amd.moments_summary(m["mean"], m["C"], m["Pbar"], truth_pose=xt, truth_landmarks=rec["lm"][:, order[:(D - 3) // 2]].T)
                say("    findings, known association, B = %d, D = %d: %s" % (B, D, ", ".join("%s %.6g" % kv for kv in s.items())))
                say("          mean heading error %.6g rad against sigmaT / 2 = %.6g; sqrt(Pbar_22) %.6g, sqrt(C_22) %.6g; position: sqrt(tr Pbar) %.6g m, sqrt(tr C) %.6g m" %
                    (s["bias_heading"], rec["conf"].sigmaT / 2, np.sqrt(m["Pbar"][2, 2]), np.sqrt(m["C"][2, 2]), np.sqrt(np.trace(m["Pbar"][:2, :2])),
                     np.sqrt(np.trace(m["C"][:2, :2]))))
            e.close()
        if a.nees_members <= 0:  # (a traced run: the timed calls alone)
            continue
        # the pose alone under the gates (the setting of section 7i's NEES figures: 8 landmarks of headroom)
        rec = record(host, name, seed)
        B = a.nees_members
        e = slam_amd.EkfEnsemble(B, rec["nlm"] + HEADROOM, **cfg_of(rec["conf"]), seed=seed)
        replay(e, rec)
        m = e.moments(3)
        s = slam_amd.moments_summary(m["mean"], m["C"], m["Pbar"], truth_pose=rec["tape"][-1][6])
        acc = e.consistency()
        say("    findings, the gates, B = %d, D = 3 (counted %d): %s; Monte Carlo NEES of the run %.4f" %
            (B, m["counted"], ", ".join("%s %.6g" % kv for kv in s.items() if not kv[0].startswith("feature")), acc[:, 2].sum() / acc[:, 0].sum()))
        e.close()


def moments_kernels(a, say):
    """the ekf_ens_mom_* kernels of a rocprofv3 --kernel-trace run of --moments with ONE map and ONE B: per call of the 3 + calls of each of
    the four variants and the 1 of the agreement check (4 (3 + calls) + 1 calls in all; Pbar is asked for in 2 (3 + calls) + 1 of them)"""
    import csv
    import glob
    import re
    files = glob.glob(os.path.join(a.moments_kernels, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % a.moments_kernels)
    tot, cnt = {}, {}
    for f in files:
        for row in csv.DictReader(open(f)):
            k = row["Kernel_Name"]
            k = re.search(r"ekf_ens_mom_[a-z_]+?_kernel", k)
            if k:
                k = k.group(0)
                tot[k] = tot.get(k, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                cnt[k] = cnt.get(k, 0) + 1
    all_calls, pbar_calls = 4 * (3 + a.calls) + 1, 2 * (3 + a.calls) + 1
    say("# tools/ekf_ens_probe.py --moments-kernels: %d calls traced, Pbar asked for in %d of them" % (all_calls, pbar_calls))
    for k in sorted(tot):
        say("    %-34s %6d launches, %9.2f us per launch, %10.1f us in all" % (k, cnt[k], tot[k] / cnt[k], tot[k]))


def baselines(slam_amd, host, name, seed, say):
    sim = host.HostSim(["-m", os.path.join(ROOT, "data", name + ".mat"), "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed])
    ekf = host.HostEkf(sim)
    nz = sim.sim_noise()
    steps, t_host = [], 0.0
    while True:
        t0 = time.perf_counter()
        r = ekf.step()
        t_host += time.perf_counter() - t0
        if r < 0:
            break
        V, G, phi, ob = ekf.last_inputs()
        z, vis = sim.last_z() if ob else (np.zeros((0, 2), f32), np.zeros(0, np.int32))
        steps.append((V, G, phi, ob, z, vis))
    dev = slam_amd.EkfGpu(sim.nlm, **cfg_of(sim.conf))
    t0 = time.perf_counter()
    for (V, G, phi, ob, z, vis) in steps:
        dev.sim(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], ob)
    dev.sync()
    t_dev = time.perf_counter() - t0
    say("    host filter (slamhost_ekf_step, one core)   %8.2f us per control step; single device handle (slamgpu_ekf_sim) %8.2f us per control step; final dim %d" %
        (1e6 * t_host / len(steps), 1e6 * t_dev / len(steps), dev.dim))
    dev.close()
    ekf.close()
    sim.close()
    return t_host / len(steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/ekf_ensemble.txt, or profiles/ens_moments.txt for the moments modes")
    ap.add_argument("--members", default="1,64,256,1024,4096")
    ap.add_argument("--nees-members", type=int, default=1024)
    ap.add_argument("--batch", default=None, help="K,K,...: the batch table of slamgpu_ens_run_noise instead")
    ap.add_argument("--moments", action="store_true", help="slamgpu_ens_moments instead: the call's time, the cost without it, the findings")
    ap.add_argument("--moments-kernels", default=None, help="DIR: the ekf_ens_mom_* kernels of a rocprofv3 --kernel-trace of --moments")
    ap.add_argument("--maps", default="example_webmap,example_loop1")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "ens_moments.txt" if a.moments or a.moments_kernels else "ekf_ensemble.txt")
    if a.moments_kernels:
        out = open(a.out, "a")

        def say_k(line):
            print(line, flush=True)
            out.write(line + "\n")
        moments_kernels(a, say_k)
        return
    import slam_amd
    from slam_amd import host
    if slam_amd.device_count() < 1:
        raise SystemExit("ekf_ens_probe needs a GPU: the ensemble has no CPU fallback")
    slam_amd.EkfEnsemble(1, 1).close()  # (the HIP runtime re-seeds libc rand() when it comes up: before any simulator is seeded)
    out = open(a.out, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if a.batch:
        batch_table(slam_amd, host, a, say)
        return
    if a.moments:
        moments_table(slam_amd, host, a, say)
        return
    say("# tools/ekf_ens_probe.py --members %s --nees-members %d" % (a.members, a.nees_members))
    for name, seed in MAPS:
        rec = record(host, name, seed)
        n = len(rec["tape"])
        nobs = sum(1 for t in rec["tape"] if t[0])
        say("%s seed %d: %d control steps, %d with an observation, %d landmarks, noise flags %d" % (name, seed, n, nobs, rec["nlm"], rec["flags"]))
        t_host = baselines(slam_amd, host, name, seed, say)
        say("    %6s %14s %14s %14s %16s %18s" % ("B", "us/step (pipe)", "us/ctl (sync)", "us/obs (sync)", "filter-steps/s", "B host filters us"))
        for B in (int(b) for b in a.members.split(",")):
            def fresh():
                return slam_amd.EkfEnsemble(B, rec["nlm"] + HEADROOM, **cfg_of(rec["conf"]), seed=seed)
            e = fresh()
            replay(e, rec, steps=200)
            e.close()
            e = fresh()
            t_all, _, _ = replay(e, rec)
            acc, dims, st = e.consistency(), e.dims(), e.status()
            e.close()
            e = fresh()
            _, t_ctl, t_obs = replay(e, rec, sync_each=True)
            e.close()
            say("    %6d %14.2f %14.2f %14.2f %16.4g %18.2f" % (B, 1e6 * t_all / n, 1e6 * t_ctl / max(n - nobs, 1), 1e6 * t_obs / max(nobs, 1), B * n / t_all,
                                                            1e6 * t_host * B))
            if B == a.nees_members:
                cnt = acc[:, 0].sum()
                per = acc[:, 2] / np.maximum(acc[:, 0], 1)
                say("    Monte Carlo NEES, B = %d: mean %.4f over %.0f member-steps, %.2f %% inside the 95 %% bound, %.0f not counted; per-member mean %.3f .. %.3f; "
                    "landmarks %d / %.2f / %d (min / mean / max); status bits set in %d members" %
                    (B, acc[:, 2].sum() / cnt, cnt, 100 * acc[:, 3].sum() / cnt, acc[:, 1].sum(), per.min(), per.max(), (dims.min() - 3) // 2,
                     ((dims - 3) // 2).mean(), (dims.max() - 3) // 2, int((st != 0).sum())))


if __name__ == "__main__":
    main()
