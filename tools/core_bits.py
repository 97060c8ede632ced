#!/usr/bin/env python3
"""GPU box diagnostic: one SHA-256 per output array of the core's entry points that tools/posterior_bits.py, observe_bits.py,
association_bits.py and multigpu_bits.py do not reach, to compare two builds of libslamgpu.so bit for bit: run it once per library
(SLAMGPU_LIB selects one) and diff the listings.  A line whose name ends in "~" would mark a quantity that is not reproducible from run
to run of ONE library (grep -v " ~ "); nothing here is: every line compares.

example_webmap, 256 particles (one block) and 1 024.  The states:
  - the caller's draws (SLAMGPU_RNG_TAPE: normals and strata through the pinned tape staging, FastSLAM 1's predict noise too), strict
    build, FastSLAM 1 and 2: slamgpu_predict + slamgpu_update per step, slamgpu_stats, slamgpu_ancestors and slamgpu_step_status after
    each, slamgpu_estimate, slamgpu_download;
  - a plain-row context (SLAMGPU_NO_COMPACT=1) stepped with host-made packets for 70 observation steps (more than the 64 slots of the
    big-packet ring: every slot is reused and waited for), both kernel builds, FastSLAM 1 and 2, with slamgpu_profile off and on:
    stats / ancestors / status every 10th step, slamgpu_download and slamgpu_upload of it after step 35 and the steps that follow,
    slamgpu_estimate, slamgpu_estimate_async and slamgpu_estimate_fetch taken in two parts, slamgpu_peek with and without landmarks,
    of a range and with a stride, slamgpu_download;
  - the row policy of host-made packets (do_update), FastSLAM 2, fast build, slamgpu_genealogy_rows after every step, history and download:
    the default compact context for the same 70 steps (its row consolidation is live); the plain-row context with
    SLAMGPU_PLAIN_ROWS_TARGET=6 (plain consolidation on a 35-landmark map); example_loop902 (117 landmarks: a compact context of a
    mid-size map), 256 particles, with its consolidation and -- SLAMGPU_NO_CONSOLIDATE=1, so that the 40 rows run out -- until 30 steps
    past its demotion to plain rows (the capacity is checked to cross 40).

usage: python tools/core_bits.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import slam_amd as sg  # noqa: E402
from slam_amd import host  # noqa: E402

STEPS, TAPE_STEPS, FIRST, LOOP_STEPS = 70, 20, 7, 2000
f32 = np.float32
KEYS = ("xv", "Pv", "w", "xf", "Pf")
n_digests = 0


def digest(tag, name, a):
    global n_digests
    a = np.ascontiguousarray(a)
    n_digests += 1
    print("%-24s %-34s %-12s %s" % (tag, name, "x".join(map(str, a.shape)) or "1", hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def load(N):
    tape = host.make_tape(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", N, "-SWITCH_SEED_RANDOM", 7],
                          max_obs=STEPS)
    assert len(tape["steps"]) == STEPS
    return tape


def after_update(s):
    ne, did, ws = s.stats()
    return np.array([ne, did, ws, s.status()], np.float64), s.ancestors()


def tape_run(T, N, method, tag):
    s = sg.SlamGpu(N, T["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_TAPE, math_mode=sg.MATH_STRICT)
    rng = np.random.default_rng(5)
    st, anc = [], []
    for step in T["steps"][:TAPE_STEPS]:
        for V, G, phi in step["controls"]:
            s.predict(V, G, T["Q"], float(T["dt"]), phi, rng.normal(size=(N, 2)).astype(f32) if s.cfg.add_predict_noise else None)
        normals = rng.normal(size=(N, 3)).astype(f32)
        strata = ((np.arange(N) + rng.uniform(size=N)) / N).astype(f32)
        s.update(step["zf"], step["idf"], step["zn"], T["R"], normals, strata)
        a, b = after_update(s)
        st.append(a)
        anc.append(b)
    digest(tag, "stats | status", np.stack(st))
    digest(tag, "ancestors", np.stack(anc))
    digest(tag, "estimate", s.estimate())
    for k, v in s.download().items():
        digest(tag, "download.%s" % k, np.asarray(v))
    s.close()


def plain_run(T, N, method, math_mode, profile, tag):
    os.environ["SLAMGPU_NO_COMPACT"] = "1"
    s = sg.SlamGpu(N, T["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7, math_mode=math_mode)
    os.environ.pop("SLAMGPU_NO_COMPACT", None)
    if profile:
        s.profile(True)
    st, anc = [], []
    for k, step in enumerate(T["steps"]):
        s.step([c for c in step["controls"]], T["Q"], float(T["dt"]), step["zf"], step["idf"], step["zn"], T["R"])
        if k % 10 == 9:
            a, b = after_update(s)
            st.append(a)
            anc.append(b)
        if k == 35:
            d = s.download()
            for key in KEYS:
                digest(tag, "download at 35.%s" % key, d[key])
            s.upload(d)
    digest(tag, "stats | status", np.stack(st))
    digest(tag, "ancestors", np.stack(anc))
    digest(tag, "genealogy_rows", np.array(s.genealogy_rows(), np.int32))
    digest(tag, "estimate", s.estimate())
    s.estimate_async()
    digest(tag, "estimate_fetch first", s.estimate_fetch(FIRST))
    digest(tag, "estimate_fetch rest", s.estimate_fetch())
    for name, kw in (("peek", {}), ("peek poses", dict(landmarks=False)), ("peek range", dict(first=3, count=40)), ("peek stride 37", dict(first=1, stride=37))):
        for key, v in s.peek(**kw).items():
            if v is not None:
                digest(tag, "%s.%s" % (name, key), np.asarray(v))
    for key, v in s.download().items():
        digest(tag, "download.%s" % key, np.asarray(v))
    s.close()


def rows_run(T, N, cap, env, steps, tag, demotes=False):
    """host-made packets only; stops `30 steps past the demotion` where one is expected"""
    for k, v in env.items():
        os.environ[k] = v
    s = sg.SlamGpu(N, cap, method=sg.FASTSLAM2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7, math_mode=sg.MATH_FAST)
    for k in env:
        os.environ.pop(k, None)
    rows, left = [], -1
    for step in T["steps"][:steps]:
        s.step([c for c in step["controls"]], T["Q"], float(T["dt"]), step["zf"], step["idf"], step["zn"], T["R"])
        rows.append(s.genealogy_rows())
        if demotes and left < 0 and rows[-1][1] > 40:
            left = 30
        if left == 0:
            break
        left -= left > 0
    rows = np.array(rows, np.int32)
    if demotes:
        assert rows[0, 1] == 40 and rows[-1, 1] > 40 and left == 0, "no demotion to plain rows 30 steps before the end of the tape (capacity %d)" % rows[-1, 1]
        first = int(np.argmax(rows[:, 1] > 40))
        digest(tag, "genealogy_rows before", rows[first - 1])
        digest(tag, "genealogy_rows after", rows[first])
    digest(tag, "genealogy_rows", rows[9::10])
    digest(tag, "genealogy_rows every step", rows)
    for q, v in zip(("xyt", "neff", "resampled"), s.history_fetch()):
        digest(tag, "history_fetch." + q, v)
    for key, v in s.download().items():
        digest(tag, "download.%s" % key, np.asarray(v))
    s.close()


for N in (256, 1024):
    T = load(N)
    if N == 256:
        rows_run(T, N, T["nlm"], {}, STEPS, "rows compact %d" % N)
        rows_run(T, N, T["nlm"], {"SLAMGPU_NO_COMPACT": "1", "SLAMGPU_PLAIN_ROWS_TARGET": "6"}, STEPS, "rows plain target 6 %d" % N)
        L = host.make_tape(["-m", os.path.join(ROOT, "data", "example_loop902.mat"), "-method", "FASTSLAM2", "-NPARTICLES", N, "-SWITCH_SEED_RANDOM", 7],
                           max_obs=LOOP_STEPS)
        rows_run(L, N, L["nlm"], {}, 400, "rows loop902 %d" % N)
        rows_run(L, N, L["nlm"], {"SLAMGPU_NO_CONSOLIDATE": "1"}, LOOP_STEPS, "rows loop902 demoted %d" % N, demotes=True)
    for method in (sg.FASTSLAM1, sg.FASTSLAM2):
        tape_run(T, N, method, "tape strict fs%d %d" % (method, N))
        for math_mode in (sg.MATH_STRICT, sg.MATH_FAST):
            for profile in (False, True):
                plain_run(T, N, method, math_mode, profile,
                          "%s fs%d %d%s" % ("strict" if math_mode == sg.MATH_STRICT else "fast", method, N, " profile" if profile else ""))
print("core_bits: %d digests" % n_digests)
