#!/usr/bin/env python3
"""GPU box diagnostic: one SHA-256 per output array of the association layer's entry points (slamgpu_associate_ex,
slamgpu_update_particle / _labels, slamgpu_run_particle, slamgpu_retire_landmarks, the settings and statistics calls), to compare two
builds of libslamgpu.so bit for bit: run it once per library (SLAMGPU_LIB selects one) and diff the listings.  Lines whose name ends in "~" are not reproducible from run
to run of ONE library (sums taken by atomics in arrival order): leave them out of the comparison (grep -v " ~ ").

The states: example_webmap, N = 300 particles (not a multiple of 256: the padding up to ncap is live), both kernel builds, linear and
log weights, FastSLAM 1 and 2.  Per state:
  - the gated association in every mode on a set the known association has driven, labels, consensus, support and stats[0], [1], [3]
    ([2] is a time); again with SLAMGPU_NO_ASSOC_LISTS=1 and with SLAMGPU_ASSOC_LCAP=1 (lists too short: the retry through the grid);
  - slamgpu_update_particle in _AUTO, _EXHAUSTIVE, _GRID and _LISTS, each plain, with the exclusion rule and the spacing factor, with
    sampling, with negative information and with mutual exclusion (a refused combination is listed with its error code), a landmark
    retired half way: the reports, the labels, the radii, the missed counts, the four statistics calls, download() and the history;
  - slamgpu_update_labels with the known association's labels;
  - slamgpu_run_particle with K = 8, exhaustive and through the lists, a host-driven step after it, K = 4 again.

usage: python tools/association_bits.py [N] [steps]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import slam_amd as sg  # noqa: E402
from slam_amd import capi, host  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
f32 = np.float32
ARGS = ["-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75,
        "-SWITCH_SEED_RANDOM", 7]
tape = host.make_tape(ARGS, max_obs=STEPS + 12)
sim = host.HostSim(ARGS)
LM, _ = sim.map()
MAX_RANGE = float(sim.conf.MAX_RANGE)
sim.close()
Q, R, dt = tape["Q"], tape["R"], float(tape["dt"])
MODES = (("auto", capi.ASSOC_AUTO), ("exhaustive", capi.ASSOC_EXHAUSTIVE), ("grid", capi.ASSOC_GRID), ("lists", capi.ASSOC_LISTS))
VARIANTS = ("plain", "excl+spacing", "sampling", "miss", "mutex")
n_digests = 0


def digest(tag, name, a):
    global n_digests
    a = np.ascontiguousarray(a)
    n_digests += 1
    print("%-44s %-22s %-10s %s" % (tag, name, "x".join(map(str, a.shape)) or "1", hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def arrays(st):
    return (np.array(st["controls"], f32).reshape(-1, 3), np.array(st["zf"], f32).reshape(-1, 2), np.array(st["idf"], np.int32),
            np.array(st["zn"], f32).reshape(-1, 2))


def predicts(s, ctl):
    for V, G, phi in ctl:
        s.predict(float(V), float(G), Q, dt, float(phi))


def state(s, tag):
    d = s.download()
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        digest(tag, "download." + k, d[k])
    digest(tag, "download.nf", np.int32(d["nf"]))
    for name, v in zip(("est", "nf", "resampled"), s.history_fetch()):
        digest(tag, "history." + name, v)


def settings(s, tag):
    digest(tag, "particle_labels", s.particle_labels())
    digest(tag, "particle_excl_radii", s.particle_excl_radii())
    digest(tag, "particle_missed", s.particle_missed())
    for name, d in (("list", s.particle_list_stats()), ("mutex", s.particle_mutex_stats()), ("sample", s.particle_sample_stats()),
                    ("miss", s.particle_miss_stats())):
        v = np.array(list(d.values()), np.int64)
        # (sample_stats: a library whose counters' zeroing is not ordered before the first launch loses that step's counts now and then)
        digest(tag, name + ("_stats ~" if name == "sample" else "_stats"), v)


def gated(kw, tag):
    s = sg.SlamGpu(N, tape["nlm"], **kw)
    for k, st in enumerate(tape["steps"][:STEPS]):
        ctl, zf, idf, zn = arrays(st)
        s.step(ctl, Q, dt, zf, idf, zn, R)
        if k not in (STEPS // 2, STEPS - 1) or len(zf) + len(zn) == 0:
            continue
        z = np.concatenate([zf, zn])
        for env in ({}, {"SLAMGPU_NO_ASSOC_LISTS": "1"}, {"SLAMGPU_ASSOC_LCAP": "1"}):
            os.environ.update(env)
            for mname, mode in MODES[:3]:
                t = "%s gated step %d %s%s" % (tag, k, mname, "".join(" %s=%s" % kv for kv in env.items()))
                lab, cons, sup, stt = s.associate(z, R, mode=mode, want_stats=True)
                digest(t, "labels", lab)
                digest(t, "consensus", cons)
                digest(t, "support ~", sup)  # (the device's vote adds the weights in arrival order)
                digest(t, "stats[0,1,3]", np.array([stt["triples"], stt["grid_entries"], float(stt["grid"])]))
                cons2 = s.associate(z, R, mode=mode, want_labels=False)[1]  # (the vote alone: no label array on the device)
                digest(t, "consensus, no labels", cons2)
            for k2 in env:
                os.environ.pop(k2)
        if k == STEPS // 2 and s.nf() > 2:
            s.retire_landmarks([1])
    state(s, tag + " gated")
    s.close()


def particle(kw, tag, mname, mode, variant):
    t = "%s particle %s %s" % (tag, mname, variant)
    s = sg.SlamGpu(N, 4 * tape["nlm"], particle_maps=True, **kw)
    opt = dict(gate_reject=4.0, gate_augment=25.0, mode=mode, new_share=0.02, p_new=0.05, census_every=1)
    if variant == "excl+spacing":
        opt["excl"] = (2.0, 0.05, 2.0)
        s.set_particle_excl_spacing(0.5)
    if variant == "sampling":
        s.set_particle_assoc_sampling(True)
    if variant == "miss":
        s.set_particle_miss(0.7, 20.0, 1.0)
    if variant == "mutex":
        s.set_particle_mutex(True)
    reports, labels = [], []
    try:
        for k, st in enumerate(tape["steps"][:STEPS]):
            ctl, zf, idf, zn = arrays(st)
            predicts(s, ctl)
            z = np.concatenate([zf, zn])
            if len(z):
                rep = s.update_particle(z, R, **opt)
                reports.append(list(rep.values()))
                labels.append(hashlib.sha256(s.particle_labels().tobytes()).digest())
            s.estimate_async()
            if k == STEPS // 2 and s.nf() > 2:
                s.retire_landmarks([1])
    except capi.SlamGpuError as e:  # (a combination the library refuses: the grid with the exclusion rule or with sampling)
        digest(t, "refused", np.int32(e.code))
        s.close()
        return
    digest(t, "reports", np.array(reports, np.int32))
    digest(t, "labels of every step", np.frombuffer(b"".join(labels), np.uint8))
    settings(s, t)
    state(s, t)
    s.close()


def labels_run(kw, tag):
    t = tag + " update_labels"
    s = sg.SlamGpu(N, 4 * tape["nlm"], particle_maps=True, **kw)
    reports = []
    for st in tape["steps"][:STEPS]:
        ctl, zf, idf, zn = arrays(st)
        predicts(s, ctl)
        if len(zf) + len(zn):
            lab = np.tile(np.concatenate([idf, np.full(len(zn), capi.ASSOC_NEW, np.int32)]), (N, 1))
            lab[N // 3::7, -1] = capi.ASSOC_DISCARD  # (some particles drop the step's last observation: slots not everybody holds)
            reports.append(list(s.update_labels(np.concatenate([zf, zn]), R, lab, p_new=0.05, census_every=2).values()))
        s.estimate_async()
    digest(t, "reports", np.array(reports, np.int32))
    settings(s, t)
    state(s, t)
    s.close()


def device_run(kw, tag, mname, mode):
    t = "%s run_particle %s" % (tag, mname)
    s = sg.SlamGpu(N, 4 * tape["nlm"], particle_maps=True, device_observe=True, **kw)
    s.set_map(LM)
    opt = dict(gate_reject=4.0, gate_augment=25.0, mode=mode, new_share=0.02, p_new=0.05, census_every=1, excl=(2.0, 0.05, 2.0))
    ctl = [arrays(st)[0] for st in tape["steps"]]
    xt = [np.asarray(st["true"], f32) for st in tape["steps"]]
    s.run_particle(ctl[0:8], Q, dt, xt[0:8], MAX_RANGE, R, noise=2, **opt)
    digest(t, "labels after K = 8", s.particle_labels())
    predicts(s, ctl[8])  # (a host-driven step: the per-particle state comes back from the device)
    o = s.observe(xt[8], MAX_RANGE, R, noise=2)
    if len(o["z"]):
        digest(t, "host step report", np.array(list(s.update_particle(o["z"], R, **opt).values()), np.int32))
    s.estimate_async()
    if s.nf() > 2:
        s.retire_landmarks([1])
    s.run_particle(ctl[9:13], Q, dt, xt[9:13], MAX_RANGE, R, noise=2, **opt)
    digest(t, "reports", s.particle_report_fetch())
    settings(s, t)
    state(s, t)
    s.close()


for math_mode in (sg.MATH_STRICT, sg.MATH_FAST):
    for method in (sg.FASTSLAM1, sg.FASTSLAM2):
        for logw in (False, True):
            tag = "%s fs%d %s" % ("strict" if math_mode == sg.MATH_STRICT else "fast", method, "log" if logw else "linear")
            kw = dict(method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7, math_mode=math_mode, log_weights=logw)
            gated(kw, tag)
            for mname, mode in MODES:
                for variant in VARIANTS:
                    particle(kw, tag, mname, mode, variant)
            labels_run(kw, tag)
            device_run(kw, tag, "exhaustive", capi.ASSOC_EXHAUSTIVE)
            device_run(kw, tag, "lists", capi.ASSOC_LISTS)
print("association_bits: %d digests" % n_digests)
