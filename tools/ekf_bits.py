#!/usr/bin/env python3
"""GPU box diagnostic: one SHA-256 per output array of the device EKF (slamgpu_ekf_*) and the EKF ensemble (slamgpu_ens_*), to compare
two builds of libslamgpu.so bit for bit: run it once per library (SLAMGPU_LIB selects one) and diff the listings.  A line whose name
ends in "~" would mark a quantity that is not reproducible from run to run of ONE library (grep -v " ~ "); nothing here is: every
line compares.  The inputs are those of tests/test_gpu_ekf.py and tests/test_gpu_ekf_ens.py (their generators are imported).

Single handle:
  - slamgpu_ekf_sim over the first 400 control steps of example_loop1 (seed 3) and example_webmap (seed 7), fed the host run's tape,
    with the gates and with the known association: the dimensions, x and P every 100 steps, pose, block, status;
  - predict / observe_heading / associate / update / augment one by one on the synthetic states of SHAPES (nf in {1, 62, 63, 64,
    128}, m up to 100), the state after each, the whole capacity through slamgpu_ekf_block (the sentinel padding included);
  - a chunk that is not positive definite: the status bit and the unchanged state.
Ensemble:
  - EDGE_CASES, sentinel-filled slabs: every member's slab, padding included;
  - the gates on tests/golden/kat_assoc.npz, batch_update off and on;
  - sim_noise with each of the eight noise-flag sets: last_inputs and the slabs;
  - the consistency accumulators and poses of a 40-step run;
  - a capacity refusal (the shared table full);
  - nz = 3, 70, 3: the buffers grow and the slot ring is reset;
  - (libraries that have slamgpu_ens_run_noise) a 24-step tape in one call and in calls of 1 + 7 + 16: the slabs, last_inputs, the
    accumulators and the trace's records and tags.
Both side by side: a B = 1 ensemble and the single handle fed the same 400 steps of example_loop1, their digests on adjacent lines
(whether they coincide is a finding, not a requirement: the rank update and the gain differ in form).

usage: python tools/ekf_bits.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import slam_amd as sg  # noqa: E402
from slam_amd import host  # noqa: E402
import test_gpu_ekf as T1  # noqa: E402
import test_gpu_ekf_ens as T2  # noqa: E402

f32 = np.float32
STEPS = 400
SENTINEL = T1.SENTINEL
n_digests = 0


def digest(tag, name, a):
    global n_digests
    a = np.ascontiguousarray(a)
    n_digests += 1
    print("%-30s %-28s %-12s %s" % (tag, name, "x".join(map(str, a.shape)) or "1", hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def state(tag, name, dev):
    x, P = dev.state()
    digest(tag, name + " x", x)
    digest(tag, name + " P", P)


def slabs(tag, name, ens):
    xs, Ps = zip(*(ens.slab(b) for b in range(ens.members)))
    digest(tag, name + " slab x", np.stack(xs))
    digest(tag, name + " slab P", np.stack(Ps))
    digest(tag, name + " dims | status", np.stack([ens.dims(), ens.status()]))


def tape(mapname, seed):
    """the host run's inputs of the first STEPS control steps"""
    sim = host.HostSim(["-m", os.path.join(ROOT, "data", mapname + ".mat"), "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed])
    ekf = host.HostEkf(sim)
    out = dict(conf=sim.conf, nlm=sim.nlm, noise=sim.sim_noise(), steps=[])
    for _ in range(STEPS):
        assert ekf.step() >= 0
        V, G, phi, ob = ekf.last_inputs()
        z, vis = sim.last_z() if ob else (np.zeros((0, 2), f32), np.zeros(0, np.int32))
        out["steps"].append((V, G, phi, ob, z, vis))
    ekf.close()
    sim.close()
    return out


# ---- single handle ----------------------------------------------------------------------------------------------------------------------
def single_run(tp, tag, known):
    nz = tp["noise"]
    dev = T1.make_dev(tp["conf"], tp["nlm"], association_known=known)
    dims = []
    for k, (V, G, phi, ob, z, vis) in enumerate(tp["steps"]):
        dev.sim(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], ob)
        dims.append(dev.dim)
        if k % 100 == 99:
            state(tag, "step %d" % k, dev)
    digest(tag, "dims", np.array(dims, np.int32))
    xyt, Pvv = dev.pose()
    digest(tag, "pose", np.concatenate([xyt, Pvv.reshape(-1)]))
    digest(tag, "block", dev.block(np.arange(0, dev.dim, 2, dtype=np.int32)))
    digest(tag, "status", np.array([dev.status()], np.int32))
    dev.close()


def staged(nf, m):
    sim, _, nz = T1.known_host()
    tag = "stages nf %d m %d" % (nf, m)
    rng = np.random.default_rng(1000 * nf + m)
    x0, P0 = T1.synthetic_state(nf, 7 * nf + m)
    cap = 3 + 2 * (nf + 2)
    idf = rng.permutation(nf)[:m].astype(np.int32)
    z = np.concatenate([T1.observations(x0, idf, rng), np.array([[17.0, 0.4]], f32)])
    dev = T1.make_dev(sim.conf, nf + 2, association_known=False)
    dev.upload(np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))
    dev.upload(x0, P0)
    dev.predict(3.0, 0.05, nz["Qe"], nz["dt"])
    state(tag, "predict", dev)
    dev.observe_heading(float(x0[2]) + 0.004)
    state(tag, "heading", dev)
    digest(tag, "associate", dev.associate(z, nz["Re"]))
    dev.update(z[:m], idf, nz["R"])
    state(tag, "update", dev)
    dev.augment(z[m:], nz["Re"])
    state(tag, "augment", dev)
    digest(tag, "block all", dev.block(np.arange(cap, dtype=np.int32)))
    xyt, Pvv = dev.pose()
    digest(tag, "pose | status", np.concatenate([xyt, Pvv.reshape(-1), [dev.status()]]))
    dev.close()


def not_positive_definite():
    sim, _, nz = T1.known_host()
    tag = "not positive definite"
    x0, P0 = T1.synthetic_state(6, 3)
    z = T1.observations(x0, np.arange(6), np.random.default_rng(11))
    Pbad = P0.copy()
    Pbad[3:, 3:] = -4.0 * np.eye(12, dtype=f32)
    dev = T1.make_dev(sim.conf, 6)
    dev.upload(x0, Pbad)
    dev.update(z[:3], [0, 1, 2], nz["R"])
    state(tag, "skipped chunk", dev)
    digest(tag, "status | unchanged", np.array([dev.status(), T1.bits_equal(dev.state()[1], Pbad)], np.int32))
    dev.upload(x0, P0)
    dev.update(z[:3], [0, 1, 2], nz["R"])
    state(tag, "good chunk after", dev)
    digest(tag, "status after", np.array([dev.status()], np.int32))
    dev.close()


# ---- ensemble ---------------------------------------------------------------------------------------------------------------------------
def ens_edge(nfs, m, nnew):
    """the launch of tests/test_gpu_ekf_ens.py::test_tiles_and_chunks"""
    sim, _, nz = T2.known_host()
    tag = "ens nf %s m %d new %d" % ("/".join(map(str, nfs)), m, nnew)
    rng = np.random.default_rng(1000 * nfs[2] + m)
    nmax = max(nfs)
    big_x, _ = T2.synthetic_state(nmax, 7 * nmax + m)
    ids_f = np.concatenate([rng.permutation(nmax) for _ in range(m // max(nmax, 1) + 1)])[:m].astype(np.int32) if nmax else np.zeros(0, np.int32)
    ids = np.concatenate([ids_f, nmax + np.arange(nnew)]).astype(np.int32)
    znew = np.stack([17.0 + np.arange(nnew), 0.4 - 0.3 * np.arange(nnew)], axis=1).astype(f32).reshape(-1, 2)
    ens = sg.EkfEnsemble(3, nmax + 5, **T2.cfg_of(sim.conf))
    cap = ens.cap_dim
    states, zs = [], []
    for nf in nfs:
        x0, P0 = T2.synthetic_state(nf, 7 * nf + m)
        states.append((x0, P0))
        zb = T2.observations(big_x, ids_f, rng) if m else np.zeros((0, 2), f32)
        own = ids_f < nf
        if own.any():
            zb[own] = T2.observations(x0, ids_f[own], rng)
        zs.append(np.concatenate([zb, znew]))
    for b in np.argsort(nfs):
        ens.upload(b, np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))
        ens.upload(b, *states[b])
    ens.sim(T2.tile([3.0, 0.05], 3), np.full(3, 0.104, f32), nz["Qe"], nz["dt"], np.stack(zs), ids, nz["Re"], nz["R"], 1)
    slabs(tag, "step", ens)
    for b in range(3):
        x, P = ens.state(b)
        digest(tag, "state %d x | P" % b, np.concatenate([x, P.reshape(-1)]))
    VG, phi, z = ens.last_inputs()
    digest(tag, "last_inputs", np.concatenate([VG.reshape(-1), phi, z.reshape(-1)]))
    ens.close()


def ens_gates():
    kat = np.load(os.path.join(ROOT, "tests", "golden", "kat_assoc.npz"))
    g1, g2 = (float(x) for x in kat["gates"])
    R = np.array([[0.1 ** 2, 0], [0, 0.017453292519943 ** 2]], f32)
    for g in range(int(kat["n_groups"])):
        xv, xf, Pf, z = (kat["g%d_%s" % (g, k)] for k in ("xv", "xf", "Pf", "z"))
        N, nf, nzg = xv.shape[0], xf.shape[1], z.shape[0]
        D = 3 + 2 * nf
        for batch in (0, 1):
            ens = sg.EkfEnsemble(N, nf + nzg, batch_update=bool(batch), gate_reject=g1, gate_augment=g2)
            for i in range(N):
                P = np.zeros((D, D), f32)
                for j in range(nf):
                    P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] = Pf[i][j]
                ens.upload(i, np.concatenate([xv[i], xf[i].reshape(-1)]).astype(f32), T2.mirrored(P))
            ens.sim(np.zeros((N, 2), f32), np.zeros(N, f32), T2.Q0, 0.025, T2.tile(z, N), None, R, R, 1)
            slabs("ens gates group %d batch %d" % (g, batch), "step", ens)
            ens.close()


def ens_noise():
    sim, _, nz = T2.known_host()
    x0, P0 = T2.synthetic_state(5, 9)
    zt = T2.observations(x0, np.arange(5), np.random.default_rng(1))
    Qc = np.array([[0.09, 0.004], [0.004, 0.0027]], f32)
    for flags in range(8):
        tag = "ens sim_noise flags %d" % flags
        ens = sg.EkfEnsemble(8, 6, **T2.cfg_of(sim.conf), seed=0xC0FFEE1234567)
        for b in range(8):
            ens.upload(b, x0, P0)
        ens.sim_noise(3.0, 0.1, 0.104, Qc, nz["dt"], 3, zt, np.arange(5, dtype=np.int32), nz["Re"], nz["R"], 1, Qe=nz["Qe"], noise=flags)
        for name, a in zip(("VG", "phi", "z"), ens.last_inputs()):
            digest(tag, "last_inputs " + name, a)
        slabs(tag, "step", ens)
        ens.close()


def ens_consistency():
    """the run of tests/test_gpu_ekf_ens.py::test_consistency_accumulators"""
    sim, _, nz = T2.known_host()
    tag = "ens consistency"
    ens = sg.EkfEnsemble(8, 4, **T2.cfg_of(sim.conf, use_heading=False), seed=77)
    lm = np.array([[15.0, 5.0], [10.0, -12.0], [-8.0, 14.0], [25.0, 20.0]])
    t, dt, poses = np.zeros(3, f32), nz["dt"], []
    for k in range(40):
        V, G = (0.0, 0.0) if k < 3 else (3.0, 0.04)
        t = np.array([t[0] + V * dt * np.cos(G + t[2]), t[1] + V * dt * np.sin(G + t[2]), t[2] + V * dt * np.sin(G) / sim.conf.WHEELBASE], f32)
        d = lm - t[:2].astype(np.float64)
        zt = np.stack([np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0]) - t[2]], axis=1).astype(f32)
        ens.sim_noise(V, G, float(t[2]), nz["Q"], dt, k, zt, np.arange(4), nz["Re"], nz["R"], k % 8 == 7, truth=t, Qe=nz["Qe"], noise=6 if k < 3 else 7)
        xyt, Pvv = ens.poses()
        poses.append(np.concatenate([xyt, Pvv.reshape(8, 9)], axis=1))
    digest(tag, "poses", np.stack(poses))
    digest(tag, "consistency", ens.consistency())
    slabs(tag, "end", ens)
    ens.consistency_reset()
    digest(tag, "after reset", ens.consistency())
    ens.close()


def ens_refusal():
    """known association, the shared table full: a new id is refused for every member (tests/test_gpu_ekf_ens.py::test_edges)"""
    sim, _, nz = T2.known_host()
    tag = "ens capacity refusal"
    x0, P0 = T2.synthetic_state(6, 3)
    x4, P4 = T2.synthetic_state(4, 3)
    z6 = T2.observations(x0, np.arange(6), np.random.default_rng(11))
    ens = sg.EkfEnsemble(3, 6, **T2.cfg_of(sim.conf, use_heading=False))
    for b, (x, P) in enumerate(((x4, P4), (x0, P0), (x0, P0))):
        ens.upload(b, x, P)
    zero = (np.zeros((3, 2), f32), np.zeros(3, f32), T2.Q0, nz["dt"])
    ens.sim(*zero, T2.tile(z6[:1], 3), [9], nz["Re"], nz["R"], 1)
    slabs(tag, "refused", ens)
    ens.sim(*zero, T2.tile(z6[:1], 3), [0], nz["Re"], nz["R"], 1)
    slabs(tag, "a known id after", ens)
    ens.close()


def ens_grow():
    """the gates, nz = 3, then 70 (the label and input buffers and the pinned slots grow, the slot ring is reset), then 3"""
    sim, _, nz = T2.known_host()
    tag = "ens nz 3 70 3"
    x0, P0 = T2.synthetic_state(10, 21)
    rng = np.random.default_rng(6)
    ens = sg.EkfEnsemble(3, 100, **T2.cfg_of(sim.conf, association_known=False))
    for b in range(3):
        ens.upload(b, x0, P0)
    for k, n in enumerate((3, 70, 3)):
        z = np.stack([T2.observations(x0, rng.integers(0, 10, n), rng) for _ in range(3)])
        ens.sim(T2.tile([3.0, 0.02], 3), np.full(3, 0.1, f32), nz["Qe"], nz["dt"], z, None, nz["Re"], nz["R"], 1)
        slabs(tag, "step %d nz %d" % (k, n), ens)
    ens.close()


def ens_run():
    """the tape of tests/test_gpu_ekf_ens_run.py::test_routes_agree_with_the_gates through slamgpu_ens_run_noise, the trace on"""
    import ekf_ens_run_model as M
    import test_gpu_ekf_ens_run as T3
    sim, _, nz = T2.known_host()
    ob = {3: [], 5: [0, 1, 2, 3], 6: [0, 1, 2, 3, 4, 5], 10: [1, 4], 15: [0, 2, 5, 6], 16: [3, 6, 7], 22: [0, 1, 2, 3, 4, 5, 6, 7]}
    tp = M.world_tape(24, ob, nz["dt"], sim.conf.WHEELBASE, T3.LM, seed=1)
    for name, cuts in (("one call", None), ("1 + 7 + 16", [1, 7, 16])):
        tag = "ens run " + name
        ens = sg.EkfEnsemble(3, 12, **T2.cfg_of(sim.conf, association_known=False), seed=1234)
        ens.trace_enable(32)
        M.drive_run(ens, tp, nz, cuts=cuts)
        slabs(tag, "end", ens)
        for what, a in zip(("VG", "phi", "z"), ens.last_inputs()):
            digest(tag, "last_inputs " + what, a)
        digest(tag, "consistency", ens.consistency())
        rec, tags = ens.trace_fetch(0, 24)
        digest(tag, "trace records", rec)
        digest(tag, "trace tags", tags)
        ens.close()


# ---- both, side by side -------------------------------------------------------------------------------------------------------------------
def side_by_side(tp):
    nz, c = tp["noise"], tp["conf"]
    dev = T1.make_dev(c, tp["nlm"])
    ens = sg.EkfEnsemble(1, tp["nlm"], **T2.cfg_of(c))
    equal = []
    for k, (V, G, phi, ob, z, vis) in enumerate(tp["steps"]):
        dev.sim(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], ob)
        ens.sim([[V, G]], [phi], nz["Qe"], nz["dt"], z[None] if len(z) else None, vis if len(z) else None, nz["Re"], nz["R"], ob)
        if k % 100 == 99:
            (xa, Pa), (xb, Pb) = dev.state(), ens.state(0)
            for name, a, b in (("x", xa, xb), ("P", Pa, Pb)):
                digest("side by side step %d" % k, "single   " + name, a)
                digest("side by side step %d" % k, "ensemble " + name, b)
            equal.append(int(T1.bits_equal(xa, xb) and T1.bits_equal(Pa, Pb)))
    digest("side by side", "equal at 99 199 299 399", np.array(equal, np.int32))
    print("# B = 1 ensemble against the single handle, example_loop1, x and P bit-identical after 100 / 200 / 300 / 400 steps: %s" % equal)
    dev.close()
    ens.close()


sg.EkfGpu(1).close()  # (the HIP runtime re-seeds libc rand() when it comes up: before any simulator is seeded)
tapes = {name: tape(name, seed) for name, seed in (("example_loop1", 3), ("example_webmap", 7))}
for name, tp in tapes.items():
    for known in (False, True):
        single_run(tp, "%s %s" % (name[8:], "known" if known else "gates"), known)
for nf, m in T1.SHAPES:
    staged(nf, m)
not_positive_definite()
for case in T2.EDGE_CASES:
    ens_edge(*case)
ens_gates()
ens_noise()
ens_consistency()
ens_refusal()
ens_grow()
side_by_side(tapes["example_loop1"])
if hasattr(sg.load_library(), "slamgpu_ens_run_noise"):  # new output, behind every line an older library prints
    ens_run()
print("ekf_bits: %d digests" % n_digests)
