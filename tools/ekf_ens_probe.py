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


def record(host, name, seed):
    """the noise-free tape of a run, and what its settings say about the noise"""
    m = os.path.join(ROOT, "data", name + ".mat")
    user = host.HostSim(["-m", m, "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed])
    flags = (1 if user.conf.SWITCH_CONTROL_NOISE else 0) | 2 | (4 if user.conf.SWITCH_SENSOR_NOISE else 0)
    user.close()
    sim = host.HostSim(["-m", m, "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed, "-SWITCH_CONTROL_NOISE", 0, "-SWITCH_SENSOR_NOISE", 0])
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
    out = dict(tape=tape, conf=sim.conf, nlm=sim.nlm, noise=sim.sim_noise(), flags=flags)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ekf_ensemble.txt"))
    ap.add_argument("--members", default="1,64,256,1024,4096")
    ap.add_argument("--nees-members", type=int, default=1024)
    ap.add_argument("--batch", default=None, help="K,K,...: the batch table of slamgpu_ens_run_noise instead")
    a = ap.parse_args()
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
