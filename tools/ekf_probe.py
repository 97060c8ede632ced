"""The numbers of DESIGN.md section 7h (not a test): the device EKF (slamgpu_ekf_*) beside the host filter, and at the size of
BASELINE config 5.  Appends to profiles/ekf.txt (or --out).

    python tools/ekf_probe.py [--out profiles/ekf.txt] [--no-small] [--no-large] [--no-kernels] [--max-range 20] [--obs-steps 200]
    python tools/ekf_probe.py --local 20 [--local-new 64] [--max-range 20] [--obs-steps 2172] [--out profiles/ekf_local.txt]
    python tools/ekf_probe.py --remove [--max-range 20] [--obs-steps 200] [--out profiles/ekf_remove.txt]

--remove: slamgpu_ekf_remove on the synthetic D = 20 003 state of large(), hipEvent times on the handle's stream (the median of five, the
state uploaded again before each), four removal sets, bytes and rate beside the device-to-device copy rate of profiles/copy_ceiling_r04.txt;
the host route (state, numpy gather, upload) once at D = 4 003; then the config-5-size course with the GATES (association unknown) with and
without the pruning rule of slam-backend -EKF_PRUNE_AGE 10 -EKF_PRUNE_HITS 3; nothing else runs.

--local margin: the config-5-size course once through the full filter and once in local periods (slamgpu_ekf_local_*) under the policy
of slam-backend -EKF_LOCAL margin, the two printed side by side; nothing else runs.

Times are wall-clock around a region that ends in slamgpu_ekf_sync, after one untimed pass over the same calls; a kernel's own
time is that of a region holding nothing else (the update chunk: four kernels, so its rate is a LOWER bound on ekf_syrk_kernel's).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32


def dev_for(slam_amd, c, nlm, **over):
    kw = dict(use_heading=c.SWITCH_HEADING_KNOWN == 1, batch_update=c.SWITCH_BATCH_UPDATE == 1, association_known=c.SWITCH_ASSOCIATION_KNOWN != 0,
              wheel_base=c.WHEELBASE, sigma_phi=c.sigmaT, gate_reject=c.GATE_REJECT, gate_augment=c.GATE_AUGMENT)
    kw.update(over)
    return slam_amd.EkfGpu(nlm, **kw)


def small_map(slam_amd, host, name, seed, max_controls, say):
    sim = host.HostSim(["-m", os.path.join(ROOT, "data", name + ".mat"), "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed])
    ekf = host.HostEkf(sim)
    nz = sim.sim_noise()
    steps, t_host = [], 0.0
    while len(steps) < max_controls:
        t0 = time.perf_counter()
        r = ekf.step()
        t_host += time.perf_counter() - t0
        if r < 0:
            break
        V, G, phi, ob = ekf.last_inputs()
        z, vis = sim.last_z() if ob else (np.zeros((0, 2), f32), np.zeros(0, np.int32))
        steps.append((V, G, phi, ob, z, vis))
    dim_host = ekf.state(cap=512, want_P=False)[0].shape[0]
    dev = dev_for(slam_amd, sim.conf, sim.nlm)
    t_ctl = t_obs = 0.0
    for (V, G, phi, ob, z, vis) in steps:
        t0 = time.perf_counter()
        dev.sim(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], ob)
        if ob:
            dev.sync()
            t_obs += time.perf_counter() - t0
        else:
            t_ctl += time.perf_counter() - t0
    dev.sync()
    nobs = sum(s[3] for s in steps)
    say("%s seed %d, %d control steps (%d with an observation), final dim host %d device %d, status %d" % (name, seed, len(steps), nobs, dim_host, dev.dim, dev.status()))
    say("    host filter      %9.1f us per control step (all steps)" % (1e6 * t_host / len(steps)))
    say("    device filter    %9.1f us per control step without an observation (enqueue only), %9.1f us per observation step (synchronised)" %
        (1e6 * t_ctl / max(len(steps) - nobs, 1), 1e6 * t_obs / max(nobs, 1)))
    dev.close()
    ekf.close()
    sim.close()


def timed(dev, fn, reps=5):
    fn()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / reps


def large(slam_amd, host, max_range, obs_steps, kernels, say):
    nlm = 10000
    lm = host.synthetic_landmarks(12345, nlm, -130, 100, -100, 90)
    s0 = host.HostSim(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "EKF1"])
    _, wp = s0.map()
    s0.close()
    with tempfile.TemporaryDirectory() as wd:
        mp = os.path.join(wd, "synthetic10k.mat")
        host.write_map(mp, lm, wp)
        open(os.path.join(wd, "synthetic10k.ini"), "w").write(open(os.path.join(ROOT, "data", "example_webmap.ini")).read())
        sim = host.HostSim(["-m", mp, "-method", "EKF1", "-SWITCH_SEED_RANDOM", 7, "-MAX_RANGE", max_range, "-SWITCH_ASSOCIATION_KNOWN", 1])
        nz = sim.sim_noise()
        try:
            dev = dev_for(slam_amd, sim.conf, nlm)
        except slam_amd.SlamGpuError as e:
            say("config-5 size: the filter does not fit: %s" % e)
            return
        table, nobs, t_obs, m_sum, t0_all = {}, 0, 0.0, 0, time.perf_counter()
        while nobs < obs_steps:
            r, V, G, phi = sim.control()
            if r < 0:
                break
            z, vis = (np.zeros((0, 2), f32), np.zeros(0, np.int32))
            if r == 1:
                sim.observe(0)
                z, vis = sim.last_z()
            t0 = time.perf_counter()
            dev.sim(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], r)
            if r == 1:
                dev.sync()
                t_obs += time.perf_counter() - t0
                m_sum += sum(1 for i in vis if int(i) in table)
                for i in vis:
                    table.setdefault(int(i), len(table))
                nobs += 1
        x, _ = dev.state(want_P=False)
        nf = (x.shape[0] - 3) // 2
        ids = np.array(sorted(table, key=table.get))
        err = np.hypot(x[3::2] - lm[0, ids], x[4::2] - lm[1, ids])
        diag = dev.block(np.arange(0, x.shape[0], max(1, x.shape[0] // 4096), dtype=np.int32)).diagonal()
        say("config-5-size run: 10 000-landmark synthetic map, MAX_RANGE %g, known association, %d observation steps (%.1f s wall in all)" %
            (max_range, nobs, time.perf_counter() - t0_all))
        say("    %d landmarks mapped (dim %d of 20 003), mean re-observed per step %.1f, %.2f ms per observation step (synchronised)" %
            (nf, x.shape[0], m_sum / max(nobs, 1), 1e3 * t_obs / max(nobs, 1)))
        say("    mean landmark error %.3f m (max %.3f), pose error %.3f m, status %d, smallest sampled diagonal entry of P %.3e" %
            (err.mean(), err.max(), float(np.hypot(*(x[:2] - sim.true_pose()[:2]))), dev.status(), diag.min()))
        dev.close()
        if not kernels:
            sim.close()
            return
        # the kernels at FULL size: a synthetic symmetric positive definite P of dimension 20 003 (diagonal plus rank one)
        D = 3 + 2 * nlm
        dev = dev_for(slam_amd, sim.conf, nlm, use_heading=True, sigma_phi=0.0175)
        rng = np.random.default_rng(1)
        u = rng.normal(0, 0.1, D).astype(f32)
        P = np.outer(u, u)
        P[np.diag_indices(D)] += f32(0.5)
        xs = np.zeros(D, f32)
        xs[3::2], xs[4::2] = lm[0], lm[1]
        dev.upload(xs, P)
        del P
        idf = np.arange(64, dtype=np.int32) * 100
        dx, dy = xs[3 + 2 * idf], xs[4 + 2 * idf]
        zf = np.stack([np.hypot(dx, dy), np.arctan2(dy, dx)], axis=1).astype(f32)
        bytes_P = 4.0 * D * D
        t = timed(dev, lambda: dev.predict(3.0, 0.01, nz["Qe"], nz["dt"]))
        say("full size, D = 20 003 (P = %.2f GB):" % (bytes_P / 1e9))
        say("    ekf_predict_kernel          %8.3f ms (touches 6 D floats of P, strided mirror writes)" % (1e3 * t))
        t = timed(dev, lambda: dev.observe_heading(0.001))
        say("    heading update (two kernels) %8.3f ms = %.2f TB/s over P read once and written once (%.2f GB)" % (1e3 * t, 2 * bytes_P / t / 1e12, 2 * bytes_P / 1e9))
        t = timed(dev, lambda: dev.update(zf, idf, nz["R"]))
        fl = 2.0 * 128 * (D * (D + 128.0) / 2)  # the tiles on or below the diagonal
        say("    update chunk, 64 observations (innov + chol + gain + syrk) %8.3f ms: ekf_syrk_kernel's %.1f GFLOP at >= %.1f TFLOP/s (155 measured "
            "FP32-MFMA peak), P read once and written once at >= %.2f TB/s" % (1e3 * t, fl / 1e9, fl / t / 1e12, 2 * bytes_P / t / 1e12))
        x, _ = dev.state(want_P=False)
        say("    after these calls: status %d, x finite %s" % (dev.status(), bool(np.isfinite(x).all())))
        dev.close()
        sim.close()


class LocalPolicy:
    """slam-backend -EKF_LOCAL margin, in Python: the region is the features within MAX_RANGE + margin of the estimate at begin; the period
    ends when the estimate is more than margin / 2 from there, when an observed id is on a passive feature, or when it is full"""

    def __init__(self, dev, host, max_range, margin, max_new):
        self.dev, self.host, self.radius, self.margin, self.max_new = dev, host, max_range + margin, margin, max_new
        self.open, self.sizes, self.t_commit = False, [], 0.0

    def begin(self, room):
        x, _ = self.dev.state(want_P=False)
        feats = self.host.ekf_local_region(x, self.radius)
        self.nf0, self.centre = (x.shape[0] - 3) // 2, x[:2].astype(np.float64)
        self.active = np.zeros(max(self.nf0, 1), bool)
        self.active[feats] = True
        self.dev.local_begin(feats, max(room, self.max_new))
        self.sizes.append(3 + 2 * feats.shape[0])
        self.open = True

    def end(self):
        if not self.open:
            return
        self.dev.sync()
        t0 = time.perf_counter()
        self.dev.local_end()
        self.dev.sync()
        self.t_commit += time.perf_counter() - t0
        self.open = False

    def sim(self, slam_amd, *args):
        vis, ob = args[6], args[9]
        nz = len(vis) if ob else 0
        if self.open and nz:
            f = self.dev.lookup(vis)
            f = f[(f >= 0) & (f < self.nf0)]
            if not self.active[f].all():
                self.end()
        if not self.open:
            self.begin(nz)
        try:
            self.dev.sim(*args)
        except slam_amd.SlamGpuError as e:
            if e.code != -3:
                raise
            self.end()  # the period is full, nothing was applied: the next one has room
            self.begin(nz)
            self.dev.sim(*args)
        if ob:
            xyt, _ = self.dev.pose()
            if np.hypot(*(xyt[:2] - self.centre)) > 0.5 * self.margin:
                self.end()


def local_course(slam_amd, host, max_range, obs_steps, margin, max_new, say):
    """the config-5-size course, recorded once, through the full filter and through local periods"""
    nlm = 10000
    lm = host.synthetic_landmarks(12345, nlm, -130, 100, -100, 90)
    s0 = host.HostSim(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "EKF1"])
    _, wp = s0.map()
    s0.close()
    with tempfile.TemporaryDirectory() as wd:
        mp = os.path.join(wd, "synthetic10k.mat")
        host.write_map(mp, lm, wp)
        open(os.path.join(wd, "synthetic10k.ini"), "w").write(open(os.path.join(ROOT, "data", "example_webmap.ini")).read())
        sim = host.HostSim(["-m", mp, "-method", "EKF1", "-SWITCH_SEED_RANDOM", 7, "-MAX_RANGE", max_range, "-SWITCH_ASSOCIATION_KNOWN", 1])
        nz = sim.sim_noise()
        course, nobs = [], 0
        while nobs < obs_steps:
            r, V, G, phi = sim.control()
            if r < 0:
                break
            z, vis = (np.zeros((0, 2), f32), np.zeros(0, np.int32))
            if r == 1:
                sim.observe(0)
                z, vis = sim.last_z()
                nobs += 1
            course.append((V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], r))
        truth = sim.true_pose()
        conf = sim.conf
        sim.close()
    say("config-5-size course: 10 000-landmark synthetic map, MAX_RANGE %g, known association, %d control steps, %d observation steps" %
        (max_range, len(course), nobs))
    finals = []
    for mode in ("full filter", "local periods, margin %g m, max_new %d" % (margin, max_new)):
        dev = dev_for(slam_amd, conf, nlm)
        pol = LocalPolicy(dev, host, max_range, margin, max_new) if mode != "full filter" else None
        table, t_obs, t0_all = {}, 0.0, time.perf_counter()
        for args in course:
            t0 = time.perf_counter()
            if pol:
                pol.sim(slam_amd, *args)
            else:
                dev.sim(*args)
            if args[9]:
                dev.sync()
                t_obs += time.perf_counter() - t0
                for i in args[6]:
                    table.setdefault(int(i), len(table))
        if pol:
            pol.end()
        dev.sync()
        wall = time.perf_counter() - t0_all
        x, _ = dev.state(want_P=False)
        ids = np.array(sorted(table, key=table.get))
        err = np.hypot(x[3::2] - lm[0, ids], x[4::2] - lm[1, ids])
        say("  %s:" % mode)
        say("    %.2f ms per observation step (synchronised%s), %.1f s wall in all" % (1e3 * t_obs / max(nobs, 1), ", commits included" if pol else "", wall))
        if pol:
            n = dev.local_info()["commits"]
            say("    %d commits, %.2f ms per commit (synchronised); active state |A| at begin: mean %.0f, largest %d of dim %d" %
                (n, 1e3 * pol.t_commit / max(n, 1), np.mean(pol.sizes), max(pol.sizes), x.shape[0]))
        say("    %d landmarks mapped (dim %d), mean landmark error %.3f m (max %.3f), pose error %.3f m, status %d" %
            ((x.shape[0] - 3) // 2, x.shape[0], err.mean(), err.max(), float(np.hypot(*(x[:2] - truth[:2]))), dev.status()))
        finals.append(x)
        dev.close()
    say("  largest |x_local - x_full| at the end: %.3e (pose %.3e)" % (np.abs(finals[1] - finals[0]).max(), np.abs(finals[1][:3] - finals[0][:3]).max()))


COPY_CEILING = 4.90e12  # hipMemcpyDtoD, bytes read + written per second (profiles/copy_ceiling_r04.txt)


class HipEvents:
    """a stream of the caller's and two events on it, through the HIP runtime libslamgpu.so runs on"""

    def __init__(self):
        import ctypes as C
        self.C = C
        self.hip = hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        vp = C.c_void_p
        hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
        hip.hipEventCreate.argtypes = [C.POINTER(vp)]
        hip.hipEventRecord.argtypes = [vp, vp]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        for fn in (hip.hipEventSynchronize, hip.hipEventDestroy, hip.hipStreamDestroy):
            fn.argtypes = [vp]
        self.stream, self.a, self.b = vp(), vp(), vp()
        assert hip.hipStreamCreate(C.byref(self.stream)) == 0 and hip.hipEventCreate(C.byref(self.a)) == 0 and hip.hipEventCreate(C.byref(self.b)) == 0

    def seconds(self, fn):
        ms = self.C.c_float()
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        assert self.hip.hipEventElapsedTime(self.C.byref(ms), self.a, self.b) == 0
        return 1e-3 * ms.value

    def close(self):
        self.hip.hipEventDestroy(self.a)
        self.hip.hipEventDestroy(self.b)
        self.hip.hipStreamDestroy(self.stream)


def remove_traffic(dim, feats):
    """bytes slamgpu_ekf_remove reads and writes: each triangle of the moved region once each way, the diagonal and x, the zeroed strip"""
    n, s0 = dim - 2 * len(feats), 3 + 2 * int(feats[0])
    tri = (n * (n - 1) - s0 * (s0 - 1)) // 2 if s0 < n else 0
    moved = 4 * (2 * tri + 4 * max(n - s0, 0))
    return moved + 4 * n * (s0 < n), moved + 4 * ((dim - n) * (dim + n) + dim - n)


def gather_host(x, P, feats):
    nf = (x.shape[0] - 3) // 2
    keep = np.setdiff1d(np.arange(nf), feats)
    src = np.concatenate([np.arange(3), np.stack([3 + 2 * keep, 4 + 2 * keep], axis=1).reshape(-1)])
    return x[src], P[np.ix_(src, src)]


def synthetic_P(D, lm):
    rng = np.random.default_rng(1)
    u = rng.normal(0, 0.1, D).astype(f32)
    P = np.outer(u, u)
    P[np.diag_indices(D)] += f32(0.5)
    xs = np.zeros(D, f32)
    xs[3::2], xs[4::2] = lm[0, :(D - 3) // 2], lm[1, :(D - 3) // 2]
    return xs, P


def remove_kernels(slam_amd, host, say):
    nlm = 10000
    lm = host.synthetic_landmarks(12345, nlm, -130, 100, -100, 90)
    D = 3 + 2 * nlm
    ev = HipEvents()
    dev = slam_amd.EkfGpu(nlm, external_stream=ev.stream.value)
    xs, P = synthetic_P(D, lm)
    sets = (("feature 0", np.array([0])), ("the middle feature", np.array([nlm // 2])), ("the last 64 features", np.arange(nlm - 64, nlm)),
            ("64 features spread evenly", np.arange(64) * (nlm // 64)))
    say("slamgpu_ekf_remove at D = 20 003 (P = %.2f GB), hipEvent time on the handle's stream, median of 5, the state uploaded again before each;" % (4.0 * D * D / 1e9))
    say("the copy rate to compare with: %.2f TB/s read + written (hipMemcpyDtoD, profiles/copy_ceiling_r04.txt)" % (COPY_CEILING / 1e12))
    for name, feats in sets:
        ts = []
        for rep in range(6):  # (the first: untimed, it makes the staging buffers)
            dev.upload(xs, P)
            t = ev.seconds(lambda: dev.remove(feats))
            if rep:
                ts.append(t)
        rd, wr = remove_traffic(D, feats)
        t = float(np.median(ts))
        say("    %-28s %8.3f ms (min %.3f, max %.3f)  read %.3f GB, written %.3f GB, %.2f TB/s = %.0f %% of the copy rate" %
            (name, 1e3 * t, 1e3 * min(ts), 1e3 * max(ts), rd / 1e9, wr / 1e9, (rd + wr) / t / 1e12, 100.0 * (rd + wr) / t / COPY_CEILING))
    x, _ = dev.state(want_P=False)
    gone = np.stack([3 + 2 * sets[-1][1], 4 + 2 * sets[-1][1]]).reshape(-1)
    xm = xs[np.setdiff1d(np.arange(D), gone)]
    say("    after the last one: dim %d, x is the gather %s, status %d" % (dev.dim, bool(np.array_equal(x, xm)), dev.status()))
    dev.close()
    del P
    # the route the library offered before: state -> numpy gather -> upload, at a size whose P the host handles comfortably
    nf = 2000
    D = 3 + 2 * nf
    xs, P = synthetic_P(D, lm)
    dev = slam_amd.EkfGpu(nf, external_stream=ev.stream.value)
    dev.upload(xs, P)
    feats = np.arange(64) * (nf // 64)
    dev.sync()
    t0 = time.perf_counter()
    x1, P1 = dev.state()
    t1 = time.perf_counter()
    x2, P2 = gather_host(x1, P1, feats)
    t2 = time.perf_counter()
    dev.upload(x2, P2)
    dev.sync()
    t3 = time.perf_counter()
    dev.upload(xs, P)
    dev.remove(feats)  # (untimed: the staging buffers)
    dev.upload(xs, P)
    t = ev.seconds(lambda: dev.remove(feats))
    x3, P3 = dev.state()
    say("D = 4 003 (P = %.0f MB), 64 features spread evenly, once:" % (4.0 * D * D / 1e6))
    say("    host route  %8.3f ms wall (state %.3f, numpy gather %.3f, upload %.3f); it synchronises and resets the id table" %
        (1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
    say("    slamgpu_ekf_remove %8.3f ms (hipEvent), the same bits: %s" % (1e3 * t, bool(np.array_equal(x3, x2) and np.array_equal(P3, P2))))
    dev.close()
    ev.close()


def gated_course(slam_amd, host, max_range, obs_steps, age, hits, say):
    """the config-5-size course with the gates, without and with the pruning rule of slam-backend -EKF_PRUNE_AGE age -EKF_PRUNE_HITS hits"""
    nlm = 10000
    lm = host.synthetic_landmarks(12345, nlm, -130, 100, -100, 90)
    s0 = host.HostSim(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "EKF1"])
    _, wp = s0.map()
    s0.close()
    with tempfile.TemporaryDirectory() as wd:
        mp = os.path.join(wd, "synthetic10k.mat")
        host.write_map(mp, lm, wp)
        open(os.path.join(wd, "synthetic10k.ini"), "w").write(open(os.path.join(ROOT, "data", "example_webmap.ini")).read())
        sim = host.HostSim(["-m", mp, "-method", "EKF1", "-SWITCH_SEED_RANDOM", 7, "-MAX_RANGE", max_range, "-SWITCH_ASSOCIATION_KNOWN", 0])
        nz = sim.sim_noise()
        course, nobs, seen = [], 0, set()
        while nobs < obs_steps:
            r, V, G, phi = sim.control()
            if r < 0:
                break
            z = np.zeros((0, 2), f32)
            if r == 1:
                sim.observe(0)
                z, vis = sim.last_z()
                seen.update(int(i) for i in vis)
                nobs += 1
            course.append((V, G, nz["Qe"], nz["dt"], phi, z, None, nz["Re"], nz["R"], r))
        truth, conf = sim.true_pose(), sim.conf
        sim.close()
    say("config-5-size course with the GATES: 10 000-landmark synthetic map, MAX_RANGE %g, association unknown, %d control steps, %d observation "
        "steps, %d distinct landmarks seen" % (max_range, len(course), nobs, len(seen)))
    for prune in (False, True):
        dev = dev_for(slam_amd, conf, nlm)
        t_obs, removed, t0_all = 0.0, 0, time.perf_counter()
        for args in course:
            t0 = time.perf_counter()
            dev.sim(*args)
            if args[9]:
                if prune:
                    st = dev.feature_stats()
                    due = np.nonzero((st["epoch"] - st["born"] == age) & (st["hits"] < hits))[0]
                    if due.shape[0]:
                        dev.remove(due)
                        removed += due.shape[0]
                dev.sync()
                t_obs += time.perf_counter() - t0
        x, _ = dev.state(want_P=False)
        nf = (x.shape[0] - 3) // 2
        near = np.array([np.hypot(lm[0] - x[3 + 2 * f], lm[1] - x[4 + 2 * f]).min() for f in range(nf)]) if nf else np.zeros(1)
        say("  %s:" % ("pruned, age %d, fewer than %d hits" % (age, hits) if prune else "every feature kept"))
        say("    %d features in the map (%d removed) for %d landmarks seen, mean distance to the nearest true landmark %.3f m (max %.3f), "
            "pose error %.3f m, status %d" % (nf, removed, len(seen), near.mean(), near.max(), float(np.hypot(*(x[:2] - truth[:2]))), dev.status()))
        say("    %.2f ms per observation step (synchronised, the rule and its removals included), %.1f s wall in all" %
            (1e3 * t_obs / max(nobs, 1), time.perf_counter() - t0_all))
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ekf.txt"))
    ap.add_argument("--no-small", action="store_true", help="skip the bundled maps")
    ap.add_argument("--no-large", action="store_true", help="skip the config-5-size run and the full-size kernels")
    ap.add_argument("--no-kernels", action="store_true", help="skip the full-size kernels (D = 20 003)")
    ap.add_argument("--max-range", type=float, default=20.0)
    ap.add_argument("--obs-steps", type=int, default=200)
    ap.add_argument("--local", type=float, default=0.0, metavar="MARGIN", help="the config-5-size course through local periods beside the full filter")
    ap.add_argument("--local-new", type=int, default=64, help="with --local: the features a period may create")
    ap.add_argument("--remove", action="store_true", help="slamgpu_ekf_remove at full size, the host route, the gated course with and without pruning")
    a = ap.parse_args()
    import slam_amd
    from slam_amd import host
    if slam_amd.device_count() < 1:
        raise SystemExit("ekf_probe needs a GPU: the device EKF has no CPU fallback")
    slam_amd.EkfGpu(1).close()  # (the HIP runtime re-seeds libc rand() when it comes up: before any simulator is seeded)
    out = open(a.out, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    say("# tools/ekf_probe.py")
    if a.remove:
        remove_kernels(slam_amd, host, say)
        gated_course(slam_amd, host, a.max_range, a.obs_steps, 10, 3, say)
        return
    if a.local > 0.0:
        local_course(slam_amd, host, a.max_range, a.obs_steps, a.local, a.local_new, say)
        return
    if not a.no_small:
        small_map(slam_amd, host, "example_webmap", 7, 10 ** 9, say)
        small_map(slam_amd, host, "example_loop902", 3, 2000, say)
    if not a.no_large:
        large(slam_amd, host, a.max_range, a.obs_steps, not a.no_kernels, say)


if __name__ == "__main__":
    main()
