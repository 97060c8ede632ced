#!/usr/bin/env python3
"""GPU box diagnostic: one SHA-256 per output array of the multi-GPU layer's entry points (slamgpu_shard_*, slamgpu_dist_*,
slamgpu_dist_group_*) and of the single-context estimate / history calls that share helpers with them, to compare two builds of
libslamgpu.so bit for bit: run it once per library (SLAMGPU_LIB selects one) and diff the listings.  A line whose name ends in "~"
would mark a quantity that is not reproducible from run to run of ONE library (grep -v " ~ "); nothing here is: every line compares.

The states: example_webmap, 512 particles as 2 logical shards of 256 and 1 024 as 4 (256: the smallest shard; 4: peers that are not
neighbours), all on one device, both kernel builds, FastSLAM 1 and 2.  Per state:
  - distributed steps (DistFilter.local) under the gather collective, and with 2 shards under push and fold (one process drives at
    most two logical shards of one device through the flag barrier: tests/test_gpu_dist.py), a download in the middle of the run
    (a settle launch), the history of every shard taken in two parts (max_count below the recorded count), the remote reads;
  - the group API (slamgpu_dist_group_*) the same way;
  - sharded plan / pack / unpack / finish steps (ShardedFilter) with the default arrival pool and with SLAMGPU_POOL_CAP=1 (every step
    with arrivals settles): the plans, slamgpu_shard_estimate at some steps, slamgpu_shard_estimate_async and its fetch in two parts,
    the caller's totals buffer (slamgpu_shard_set_totals_buffer) for the first half of the run and the context's own after it;
  - a single context on the same tape: slamgpu_estimate at some steps, slamgpu_estimate_async, slamgpu_history_fetch in two parts.

usage: python tools/multigpu_bits.py [steps]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import slam_amd as sg  # noqa: E402
from slam_amd import host  # noqa: E402
from slam_amd.dist import DistFilter  # noqa: E402
from slam_amd.sharded import GpuEngine, LocalComm, ShardedFilter  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
SHARD = 256
FIRST = 7  # history entries the first of the two fetches takes
f32 = np.float32
ARGS = ["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75,
        "-SWITCH_SEED_RANDOM", 7]
tape = host.make_tape(ARGS, max_obs=STEPS)
Q, R, dt = tape["Q"], tape["R"], float(tape["dt"])
STEP_ARGS = [(np.array(st["controls"], f32).reshape(-1, 3), np.array(st["zf"], f32).reshape(-1, 2), np.array(st["idf"], np.int32),
              np.array(st["zn"], f32).reshape(-1, 2)) for st in tape["steps"][:STEPS]]
MID = len(STEP_ARGS) // 2
n_digests = 0


def digest(tag, name, a):
    global n_digests
    a = np.ascontiguousarray(a)
    n_digests += 1
    print("%-40s %-30s %-12s %s" % (tag, name, "x".join(map(str, a.shape)) or "1", hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def state(tag, name, d):
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        digest(tag, "%s.%s" % (name, k), d[k])


def cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in ("xv", "Pv", "w", "xf", "Pf")}


def dist_run(kw, tag, G, collective):
    t = "%s dist x%d %s" % (tag, G, collective)
    f = DistFilter.local(G, SHARD, tape["nlm"], **kw)
    if collective != "gather" and not f.use_push(fold=(collective == "fold")):
        print("%-40s the flag barrier did not complete on this stack: left out" % t, flush=True)
        f.close()
        return
    for c in f.ctx:
        c.dist_remote_reads()  # (the counter is kept from the first time it is asked for)
    for k, (ctl, zf, idf, zn) in enumerate(STEP_ARGS):
        f.step(ctl, Q, dt, zf, idf, zn, R)
        if k == MID:
            state(t, "download at %d" % k, cat(f.download()))
    f.settle()
    for part, count in (("first", FIRST), ("rest", 4096)):
        for g, c in enumerate(f.ctx):
            for name, v in zip(("raw4", "neff", "resampled", "status"), c.shard_estimate_fetch_full(count)):
                digest(t, "history %s, shard %d.%s" % (part, g, name), v)
    state(t, "download", cat(f.download()))
    remote = [c.dist_remote_reads() for c in f.ctx]
    digest(t, "remote_reads = %d" % sum(remote), np.array(remote, np.uint64))
    if collective != "gather":
        digest(t, "collective_ok", np.int32(f.collective_ok()))
    f.close()


def group_run(kw, tag, G):
    t = "%s group x%d" % (tag, G)
    g = sg.DistGroup(G, SHARD, tape["nlm"], **kw)
    for k, (ctl, zf, idf, zn) in enumerate(STEP_ARGS):
        g.step(ctl, Q, dt, zf, idf, zn, R)
        if k == MID:
            state(t, "download at %d" % k, g.download())
    for part, count in (("first", FIRST), ("rest", 4096)):
        for name, v in zip(("xyt", "neff", "resampled"), g.history_fetch(count)):
            digest(t, "history %s.%s" % (part, name), v)
        digest(t, "history %s.status" % part, g.last_history_status)
    state(t, "download", g.download())
    g.close()


def sharded_run(kw, tag, G, pool_cap):
    t = "%s sharded x%d pool %s" % (tag, G, pool_cap or "default")
    if pool_cap:
        os.environ["SLAMGPU_POOL_CAP"] = pool_cap
    eng = [GpuEngine(g, G, SHARD, tape["nlm"], rng_mode=sg.RNG_PHILOX, **kw) for g in range(G)]
    flt = ShardedFilter(eng, LocalComm(eng), G)  # (the engines write their totals into the filter's buffers: a caller's)
    plans, now = [], []
    for k, (ctl, zf, idf, zn) in enumerate(STEP_ARGS):
        p = flt.step(ctl, Q, dt, zf, idf, zn, R)
        plans.append([p.wsum, p.wsq, p.neff, float(p.resampled)] + [float(x) for x in p.K[:G + 1]])
        if k % 5 == 2:
            now.append(np.concatenate([e.estimate_local() for e in eng]))
        if k == MID:  # ... and back to the contexts' own
            for e in eng:
                e.ctx.shard_set_totals_buffer(None)
                e._totals_direct = False
    digest(t, "plans, %d resampled" % sum(int(p[3]) for p in plans), np.array(plans, np.float64))
    digest(t, "shard_estimate", np.array(now, np.float64))
    digest(t, "exchanged_records = %d" % flt.exchanged_records, np.int64(flt.exchanged_records))
    for part, count in (("first", FIRST), ("rest", 4096)):
        for g, e in enumerate(eng):
            digest(t, "estimate_fetch %s, shard %d" % (part, g), e.ctx.shard_estimate_fetch(count))
    state(t, "download", cat([e.ctx.download() for e in eng]))
    digest(t, "ancestors", np.concatenate([e.ctx.ancestors() for e in eng]))
    flt.close()
    os.environ.pop("SLAMGPU_POOL_CAP", None)


def single_run(kw, tag, N):
    t = "%s single %d" % (tag, N)
    s = sg.SlamGpu(N, tape["nlm"], rng_mode=sg.RNG_PHILOX, **kw)
    now = []
    for k, (ctl, zf, idf, zn) in enumerate(STEP_ARGS):
        s.step(ctl, Q, dt, zf, idf, zn, R)  # (records: slamgpu_estimate_async)
        if k % 5 == 2:
            now.append(s.estimate())
        if k % 5 == 3:  # an estimate of a set that has moved since its update
            s.predict(1.0, 0.01, Q, dt)
            now.append(s.estimate())
            s.estimate_async()
    digest(t, "estimate", np.array(now, np.float64))
    for part, count in (("first", FIRST), ("rest", 4096)):
        for name, v in zip(("xyt", "neff", "resampled"), s.history_fetch(count)):
            digest(t, "history %s.%s" % (part, name), v)
        digest(t, "history %s.status" % part, s.last_history_status)
    state(t, "download", s.download())
    s.close()


for math_mode in (sg.MATH_STRICT, sg.MATH_FAST):
    for method in (sg.FASTSLAM1, sg.FASTSLAM2):
        for G in (2, 4):
            N = G * SHARD
            tag = "%s fs%d" % ("strict" if math_mode == sg.MATH_STRICT else "fast", method)
            kw = dict(method=method, n_effective=int(0.75 * N), seed=7, math_mode=math_mode)
            for collective in ("gather", "push", "fold") if G == 2 else ("gather",):
                dist_run(kw, tag, G, collective)
            group_run(kw, tag, G)
            sharded_run(kw, tag, G, None)
            sharded_run(kw, tag, G, "1")
            single_run(kw, tag, N)
print("multigpu_bits: %d digests" % n_digests)
