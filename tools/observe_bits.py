#!/usr/bin/env python3
"""GPU box diagnostic: one SHA-256 per output array of the observation layer's entry points (slamgpu_set_map, slamgpu_observe,
slamgpu_step_observe, slamgpu_observe_fetch, slamgpu_run_observe, slamgpu_persist_info) and of the calls that hand the genealogy book
between device and host (slamgpu_num_landmarks, slamgpu_step, slamgpu_download, slamgpu_peek, slamgpu_genealogy_rows), to compare two
builds of libslamgpu.so bit for bit: run it once per library (SLAMGPU_LIB selects one) and diff the listings.  A line whose name ends
in "~" would mark a quantity that is not reproducible from run to run of ONE library (grep -v " ~ "); nothing here is: every line compares.

The states: example_webmap as a compact context, example_webmap with plain rows (SLAMGPU_NO_COMPACT=1) and the synthetic map of
tests/test_gpu_observe.py (1 000 landmarks, MAX_RANGE 20), both with SLAMGPU_FLAG_DEVICE_OBSERVE; both kernel builds, FastSLAM 1 and
2, 256 particles (the smallest block) and 1 024.  Per state:
  - slamgpu_observe along the true path with noise 0, 1 (a tape) and 2 (Philox), a fresh association table each;
  - slamgpu_step_observe, slamgpu_observe_fetch every 5th step, slamgpu_peek against slamgpu_download_range of the same particles,
    the history taken in two parts;
  - slamgpu_run_observe with K = 2, then K = 300 (the queue grows past its first 256 entries), as the persistent loop where the
    context qualifies and with SLAMGPU_NO_PERSIST=1; the slamgpu_persist_info counts;
  - a hand-over in the middle of a run: device steps, slamgpu_num_landmarks (pull), a host-made slamgpu_step that re-observes what the
    last device step saw (no new landmark: a compact context allows that one too), device steps again (push), slamgpu_download;
  - slamgpu_genealogy_rows after each.

usage: python tools/observe_bits.py [steps]"""
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import slam_amd as sg  # noqa: E402
from slam_amd import host  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
K1, K2 = 2, 300
FIRST = 7  # history entries the first of the two fetches takes
f32 = np.float32
DATA = os.path.join(ROOT, "data")
n_digests = 0


def digest(tag, name, a):
    global n_digests
    a = np.ascontiguousarray(a)
    n_digests += 1
    print("%-36s %-34s %-12s %s" % (tag, name, "x".join(map(str, a.shape)) or "1", hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def load(args):
    tape = host.make_tape(args, max_obs=K1 + K2)
    sim = host.HostSim(args)
    lm, _ = sim.map()
    mr = float(sim.conf.MAX_RANGE)
    sim.close()
    steps = tape["steps"]
    assert len(steps) == K1 + K2, len(steps)
    return dict(nlm=tape["nlm"], lm=lm, mr=mr, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]),
                ctl=[np.array(st["controls"], f32).reshape(-1, 3) for st in steps], xt=[np.asarray(st["true"], f32) for st in steps])


def synthetic(tmp):
    lmk = host.synthetic_landmarks(4321, 1000, -130, 100, -100, 90)
    h0 = host.HostSim(["-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-SWITCH_SEED_RANDOM", 7])
    _, wp = h0.map()
    h0.close()
    mp = os.path.join(tmp, "syn1000.mat")
    host.write_map(mp, lmk, wp)
    ini = open(os.path.join(DATA, "example_webmap.ini")).read().replace("MAX_RANGE           = 60.0", "MAX_RANGE           = 20.0")
    open(os.path.join(tmp, "syn1000.ini"), "w").write(ini)
    return load(["-m", mp, "-method", "FASTSLAM2", "-SWITCH_SEED_RANDOM", 3])


def state(tag, name, s):
    rows = s.genealogy_rows()  # (before the download, which flattens the records into one row)
    digest(tag, "%s genealogy_rows = %d of %d" % ((name,) + rows), np.array(rows, np.int32))
    d = s.download()
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        digest(tag, "%s download.%s" % (name, k), d[k])
    digest(tag, "%s persist_info = %d, %d" % ((name,) + s.persist_info()), np.array(s.persist_info(), np.int64))


def history(tag, name, s):
    for part, count in (("first", FIRST), ("rest", 4096)):
        for key, v in zip(("xyt", "neff", "resampled"), s.history_fetch(count)):
            digest(tag, "%s history %s.%s" % (name, part, key), v)
        digest(tag, "%s history %s.status" % (name, part), s.last_history_status)


def packets(ps):
    out = {k: np.concatenate([p[k].ravel() for p in ps]) for k in ("z", "vis", "zf", "idf", "zn")}
    out["counts"] = np.array([[len(p[k]) for k in ("z", "zf", "zn")] for p in ps], np.int32)
    return out


def observe_run(M, make, tag):
    s = make()
    rng = np.random.default_rng(11)
    for noise in (0, 1, 2):
        s.set_map(M["lm"])  # (a fresh association table)
        ps = []
        for x in M["xt"][:STEPS:3]:
            r1, r2 = (rng.normal(size=M["nlm"]).astype(f32) for _ in range(2))
            ps.append(s.observe(x, M["mr"], M["R"], noise=noise, r1=r1 if noise == 1 else None, r2=r2 if noise == 1 else None))
        for k, v in packets(ps).items():
            digest(tag, "observe noise %d.%s" % (noise, k), v)
    s.close()


def step_run(M, make, tag):
    s = make()
    s.set_map(M["lm"])
    ps = []
    for k in range(STEPS):
        s.step_observe(M["ctl"][k], M["Q"], M["dt"], M["xt"][k], M["mr"], M["R"], noise=2)
        if k % 5 == 4:
            ps.append(s.observe_fetch())
    for k, v in packets(ps).items():
        digest(tag, "step_observe fetch.%s" % k, v)
    pk, dl = s.peek(first=3, stride=1, count=40), s.download(first=3, count=40)
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        digest(tag, "step_observe peek.%s" % k, pk[k])
        digest(tag, "step_observe download_range.%s" % k, dl[k])
        digest(tag, "step_observe peek == range.%s" % k, np.int32(pk[k].tobytes() == dl[k].tobytes()))
    for k, v in s.peek(first=1, stride=37).items():
        digest(tag, "step_observe peek stride 37.%s" % k, np.asarray(v))
    history(tag, "step_observe", s)
    state(tag, "step_observe", s)
    s.close()


def loop_run(M, make, tag, persist):
    if not persist:
        os.environ["SLAMGPU_NO_PERSIST"] = "1"
    s = make()
    os.environ.pop("SLAMGPU_NO_PERSIST", None)
    s.set_map(M["lm"])
    name = "run_observe" if persist else "run_observe per step"
    for a, b in ((0, K1), (K1, K1 + K2)):
        s.run_observe(M["ctl"][a:b], M["Q"], M["dt"], M["xt"][a:b], M["mr"], M["R"], noise=2)
    digest(tag, "%s observe_fetch.z" % name, s.observe_fetch()["z"])
    history(tag, name, s)
    state(tag, name, s)
    s.close()


def handover_run(M, make, tag):
    s = make()
    s.set_map(M["lm"])
    T = min(STEPS, 24) // 2
    for k in range(T):
        s.step_observe(M["ctl"][k], M["Q"], M["dt"], M["xt"][k], M["mr"], M["R"], noise=2)
    p = s.observe_fetch()
    digest(tag, "hand-over nf = %d" % s.nf(), np.int32(s.nf()))  # (pull)
    s.step(M["ctl"][T], M["Q"], M["dt"], p["zf"], p["idf"], np.zeros((0, 2), f32), M["R"])  # host-made, nothing new
    for k in range(T + 1, 2 * T):  # (push)
        s.step_observe(M["ctl"][k], M["Q"], M["dt"], M["xt"][k], M["mr"], M["R"], noise=2)
    history(tag, "hand-over", s)
    state(tag, "hand-over", s)
    s.close()


with tempfile.TemporaryDirectory() as tmp:
    web = load(["-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-SWITCH_SEED_RANDOM", 7])
    maps = (("webmap compact", web, False), ("webmap plain", web, True), ("synthetic plain", synthetic(tmp), True))
    for math_mode in (sg.MATH_STRICT, sg.MATH_FAST):
        for method in (sg.FASTSLAM1, sg.FASTSLAM2):
            for N in (256, 1024):
                for mname, M, plain in maps:
                    tag = "%s fs%d %d %s" % ("strict" if math_mode == sg.MATH_STRICT else "fast", method, N, mname)

                    def make():
                        if plain:
                            os.environ["SLAMGPU_NO_COMPACT"] = "1"
                        s = sg.SlamGpu(N, M["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7, math_mode=math_mode,
                                       device_observe=True)
                        os.environ.pop("SLAMGPU_NO_COMPACT", None)
                        return s

                    observe_run(M, make, tag)
                    step_run(M, make, tag)
                    if not plain:
                        loop_run(M, make, tag, True)
                    loop_run(M, make, tag, False)
                    handover_run(M, make, tag)
print("observe_bits: %d digests" % n_digests)
