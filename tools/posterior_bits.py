#!/usr/bin/env python3
"""GPU box diagnostic: one SHA-256 per output array of every posterior entry point (slamgpu_map_summary, _map_pairs, _joint_summary,
_pose_*, _innovation_*, _path_*, ring fetches included) on a few seeded states, to compare two builds of libslamgpu.so bit for bit:
run it once per library (SLAMGPU_LIB selects one) and diff the listings.

The states: example_webmap driven by slamgpu_step with host-made packets and all three rings on, N = 9 222 particles (ten tiles of
1 024 with six in the last), compact genealogy rows and plain ones, linear and log weights, both kernel builds; the calls are made
straight after an update that resampled (its gather pending), with counts of 11 cut into chunks by the diagnostic overrides, and once
more after download() has settled the state.

usage: python tools/posterior_bits.py [N] [steps]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import slam_amd as sg  # noqa: E402
from slam_amd import host  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 9222
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 70
f32 = np.float32
CHUNKS = {"SLAMGPU_MAP_CHUNK": "8", "SLAMGPU_INNOV_CHUNK": "8", "SLAMGPU_JOINT_CHUNK": "2", "SLAMGPU_PATH_CHUNK": "5"}
tape = host.make_tape(["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100,
                       "-NEFFECTIVE", 75, "-SWITCH_SEED_RANDOM", 7], max_obs=STEPS)
Q, R, dt = tape["Q"], tape["R"], float(tape["dt"])


def digest(tag, name, a):
    a = np.ascontiguousarray(a)
    print("%-34s %-22s %-10s %s" % (tag, name, "x".join(map(str, a.shape)) or "1", hashlib.sha256(a.tobytes()).hexdigest()))


def summaries(s, tag, zf, idf):
    nf = s.nf()
    count = min(11, nf)
    pairs = np.array([(a, b) for a in range(nf) for b in range(a, nf)], np.int32)[:11]
    zf11, idf11 = np.resize(zf, (11, 2)), np.resize(idf, 11)
    for chunked in (False, True):
        for k, v in CHUNKS.items():
            if chunked:
                os.environ[k] = v
            else:
                os.environ.pop(k, None)
        t = tag + (" chunked" if chunked else "")
        for q, v in s.map_summary(0, count).items():
            digest(t, "map_summary." + q, v)
        for q, v in s.map_pairs(pairs).items():
            digest(t, "map_pairs." + q, v)
        j = s.joint_summary(np.arange(count))
        digest(t, "joint_summary.raw", j["raw"])
        digest(t, "joint_summary.both", np.int32(j["both"]))
        digest(t, "pose_summary", s.pose_summary())
        out, holders = s.innovation_summary(zf11, idf11, R)
        digest(t, "innovation_summary.out", out)
        digest(t, "innovation_summary.holders", holders)
        for q, v in s.path_summary().items():
            digest(t, "path_summary." + q, v)
    for k in CHUNKS:
        os.environ.pop(k, None)
    xyt, index = s.path_trace()
    digest(tag, "path_trace.xyt", xyt)
    digest(tag, "path_trace.index", index)


for math_mode in (sg.MATH_STRICT, sg.MATH_FAST):
    for layout in ("compact", "plain"):
        for logw in (False, True):
            tag = "%s %s %s" % ("strict" if math_mode == sg.MATH_STRICT else "fast", layout, "log" if logw else "linear")
            s = sg.SlamGpu(N, tape["nlm"] if layout == "compact" else 300, method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7,
                           math_mode=math_mode, log_weights=logw)
            assert (s.genealogy_rows()[1] <= 40) == (layout == "compact"), "not the %s layout" % layout
            # rings that wrap: fewer slots than the run records
            s.path_enable(24)
            s.pose_history_enable(17)
            s.innovation_history_enable(50)
            done = False
            for k, st in enumerate(tape["steps"]):
                zf, idf, zn = np.array(st["zf"], f32).reshape(-1, 2), np.array(st["idf"], np.int32), np.array(st["zn"], f32).reshape(-1, 2)
                s.step(np.array(st["controls"], f32).reshape(-1, 3), Q, dt, zf, idf, zn, R)
                if not done and k >= 40 and len(idf) and s.stats()[1]:  # the update resampled: its gather is pending
                    summaries(s, tag + " pending", zf, idf)
                    s.download()
                    summaries(s, tag + " settled", zf, idf)
                    done = True
            assert done, "no update from step 40 on resampled"
            digest(tag, "pose_history_info", np.array(s.pose_history_info(), np.int64))
            digest(tag, "pose_history_fetch", s.pose_history_fetch())
            a, b, cap, rec = s.innovation_history_info()
            digest(tag, "innovation_history_info", np.array([a, b, cap, rec], np.int64))
            for name, v in zip(("out", "record", "slot"), s.innovation_history_fetch()):
                digest(tag, "innovation_history_fetch." + name, v)
            for name, v in zip(("out", "record", "slot"), s.innovation_history_fetch(b - 7, 7)):  # a window that ends at next
                digest(tag, "innovation_history_fetch[-7:]." + name, v)
            a, b, cap = s.path_info()
            digest(tag, "path_info", np.array([a, b, cap], np.int64))
            for r in (a, b - 1):
                xyt, parent = s.path_fetch(r)
                digest(tag, "path_fetch[%d].xyt" % (r - a), xyt)
                digest(tag, "path_fetch[%d].parent" % (r - a), parent)
            for q, v in s.path_summary(a + 3, 11).items():
                digest(tag, "path_summary[3:14]." + q, v)
            s.close()
print("posterior_bits: done")
