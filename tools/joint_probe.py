"""Cost of the joint posterior (slamgpu_joint_summary), in one process, FastSLAM 2, fast build, known association:

  (a) example_webmap, 10^5 particles after 100 steps of the course: one call over ALL slots in use -- the five kernels' time between
      event pairs (slamgpu_profile / slamgpu_kernel_time) and the whole call between two events -- beside slamgpu_map_summary over
      the same slots plus slamgpu_pose_summary, which together read the same bytes.
  (b) the same on a 126-slot subset of a synthetic 1 000-landmark map (log-weights) after 40 steps: D = 255, the widest list.
  (c) a finding, not a cost: example_webmap, seed 7, at the end of the run, the FastSLAM 2 joint P (512 and 10^5 particles,
      slamhost_joint_dense) beside the EKF's P on the same course (slamhost_ekf_state; the same map, waypoints and simulator seed: the
      FastSLAM arm's observations are made on the device with its own noise stream, the EKF's by the host's: not the same realisation): traces of the pose and landmark blocks and the
      largest cross-correlations.

2 calls of warm-up, median of 7.

    python tools/joint_probe.py [--out profiles/joint.txt] [--particles 100000] [--skip-ekf]"""
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
from particle_lists_probe import course  # noqa: E402

JOINT = ("joint_hold", "joint_pivot", "joint_gram", "joint_reduce", "joint_finish")
MARG = ("map_summary", "map_finish", "pose_summary", "pose_finish")


def known(c, N, logw=False):
    s = slam_amd.SlamGpu(N, c["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=slam_amd.RNG_PHILOX, seed=5, device_observe=True,
                         math_mode=slam_amd.MATH_FAST, log_weights=logw)
    s.set_map(c["lm"])
    return s


def run(s, c, a, b):
    s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)


def timed(s, names, call, reps=7, warm=2):
    """(median kernel ms, median whole-call ms, per-kernel mean ms, the calls' whole times)"""
    ks, ws = [], []
    base = {k: s.kernel_time(k)[0] for k in names}
    for rep in range(warm + reps):
        a = sum(s.kernel_time(k)[0] for k in names)
        s.timer_start()
        call()
        w = s.timer_stop()
        k = sum(s.kernel_time(k)[0] for k in names) - a
        if rep >= warm:
            ks.append(k), ws.append(w)
    each = {k: (s.kernel_time(k)[0] - base[k]) / (warm + reps) for k in names}
    return statistics.median(ks), statistics.median(ws), each, ws


def one_state(tag, c, N, steps, logw, slots_of):
    s = known(c, N, logw)
    run(s, c, 0, steps)
    s.history_fetch()
    slots = slots_of(s)
    k, D = len(slots), 3 + 2 * len(slots)
    s.profile(True)
    jk, jw, je, jws = timed(s, JOINT, lambda: s.joint_summary(slots))
    os.environ["SLAMGPU_JOINT_PLAIN_FMA"] = "1"   # the Gram pass by plain double FMAs from the same LDS tile
    fk, fw, fe, fws = timed(s, JOINT, lambda: s.joint_summary(slots))
    del os.environ["SLAMGPU_JOINT_PLAIN_FMA"]
    lo, n = int(min(slots)), int(max(slots)) - int(min(slots)) + 1

    def marginals():
        s.map_summary(lo, n)
        s.pose_summary()
    mk, mw, me, mws = timed(s, MARG, marginals)
    o = s.joint_summary(slots)
    s.profile(False)
    s.close()
    rec = N * (20.0 * k + 40.0)   # 16 + 4 B per record, 40 B per pose
    fma = N * D * D / 2.0
    return ["%s: N = %d after %d steps, k = %d slots listed (D = %d), joint share %.6f, %d particles hold them all" % (tag, N, steps, k, D, o["share"], o["both"]),
            "    joint_summary kernels %.1f us (%s)" % (1e3 * jk, ", ".join("%s %.1f" % (q, 1e3 * je[q]) for q in JOINT)),
            "    joint_summary whole call %.1f us  (calls %s)" % (1e3 * jw, " ".join("%.1f" % (1e3 * x) for x in jws)),
            "    the same with the Gram pass by plain double FMAs (SLAMGPU_JOINT_PLAIN_FMA=1): kernels %.1f us (joint_gram %.1f), whole call %.1f us: "
            "MFMA / plain x %.2f in joint_gram" % (1e3 * fk, 1e3 * fe["joint_gram"], 1e3 * fw, je["joint_gram"] / fe["joint_gram"]),
            "    map_summary over slots [%d, %d) + pose_summary: kernels %.1f us (%s), whole calls %.1f us  (calls %s)" %
            (lo, lo + n, 1e3 * mk, ", ".join("%s %.1f" % (q, 1e3 * me[q]) for q in MARG), 1e3 * mw, " ".join("%.1f" % (1e3 * x) for x in mws)),
            "    joint / marginals: kernels x %.2f, whole call x %.2f" % (jk / mk, jw / mw),
            "    per call: %.3g double FMAs in the Gram pass (%.2f TFLOP/s of joint_gram's time), records + poses %.1f MB (read by joint_hold in part "
            "and by joint_gram once per group of 16 block pairs)" % (fma, 2.0 * fma / (je["joint_gram"] * 1e-3) / 1e12, rec / 1e6), ""]


def blocks(x, P):
    D = len(x)
    k = (D - 3) // 2
    sd = np.sqrt(np.clip(np.diag(P), 0, None))
    with np.errstate(all="ignore"):
        R = np.abs(P / np.outer(sd, sd))
    R = np.nan_to_num(R)
    lm = (np.arange(3, D) - 3) // 2
    other = lm[:, None] != lm[None, :]
    return dict(k=k, pose=float(np.trace(P[:2, :2])), heading=float(P[2, 2]), lm=float(np.trace(P[3:, 3:])) / max(k, 1),
                cpl=float(R[3:, :3].max()) if k else 0.0, cll=float((R[3:, 3:] * other).max()) if k > 1 else 0.0)


def ekf_compare():
    args = ["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "EKF1", "-SWITCH_SEED_RANDOM", 7]
    sim = host.HostSim(args)
    e = host.HostEkf(sim)
    while e.step() >= 0:
        pass
    xe, Pe = e.state(cap=128)
    e.close()
    sim.close()
    be = blocks(xe.astype(np.float64), Pe.astype(np.float64))
    lines = ["(c) example_webmap, seed 7, at the end of the course: the joint P of FastSLAM 2 (known association) beside the EKF's (same course, not the same noise)",
             "    %-28s %3s  %12s %12s %14s %10s %10s" % ("filter", "k", "tr P_xy m^2", "P_theta", "tr P_lm / k", "max |r| pl", "max |r| ll"),
             "    %-28s %3d  %12.5g %12.5g %14.5g %10.4f %10.4f" % ("EKF-SLAM", be["k"], be["pose"], be["heading"], be["lm"], be["cpl"], be["cll"])]
    c = course(os.path.join(ROOT, "data", "example_webmap.mat"), 100000)
    for N in (512, 100000):
        s = known(c, N)
        for a in range(0, len(c["ctl"]), 1000):
            run(s, c, a, min(a + 1000, len(c["ctl"])))
            s.history_fetch()
        o = s.joint_summary(np.arange(s.nf()))
        x, P, status = host.joint_dense(o)
        s.close()
        b = blocks(x, P)
        lines.append("    %-28s %3d  %12.5g %12.5g %14.5g %10.4f %10.4f   (P %s)" %
                     ("FastSLAM 2, N = %d" % N, b["k"], b["pose"], b["heading"], b["lm"], b["cpl"], b["cll"],
                      {0: "positive definite", 1: "NOT positive definite", -1: "holds NaN"}[status]))
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--skip-ekf", action="store_true")
    a = ap.parse_args()
    lines = ["joint_probe: FastSLAM 2, fast build, known association; 2 calls of warm-up, median of 7; library %s" % os.path.basename(slam_amd.lib_path()), ""]
    c = course(os.path.join(ROOT, "data", "example_webmap.mat"), 100)
    lines += one_state("(a) example_webmap", c, a.particles, 100, False, lambda s: np.arange(s.nf()))
    with tempfile.TemporaryDirectory() as d:
        lm = host.synthetic_landmarks(12345 + 1000, 1000, -130, 100, -100, 90)
        h = host.HostSim(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75,
                          "-SWITCH_SEED_RANDOM", 7])
        _, wp = h.map()
        h.close()
        mp = os.path.join(d, "synthetic1000.mat")
        host.write_map(mp, lm, wp)
        open(os.path.join(d, "synthetic1000.ini"), "w").write(open(os.path.join(ROOT, "data", "example_webmap.ini")).read())
        c2 = course(mp, 40)
        lines += one_state("(b) synthetic 1 000-landmark map, log-weights", c2, a.particles, 40, True, lambda s: np.arange(min(s.nf(), slam_amd.capi.JOINT_MAX_SLOTS)))
    if not a.skip_ekf:
        lines += ekf_compare()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
