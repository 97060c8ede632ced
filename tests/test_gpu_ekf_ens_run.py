"""The ensemble's K-step run and trace (include/slamgpu.h: slamgpu_ens_run_noise, slamgpu_ens_trace_*) on the GPU.  "Twin": a second
handle with the same config and seed, driven by one sim_noise per step.  "Identical": bit for bit on every member's slab(), dims(),
status(), consistency(), last_inputs(), and the trace where it is on (tests/ekf_ens_run_model.py: snapshot, identical).
  1. route equivalence with the gates;  2. with the known association, a step that does not fit included;  3. chunk and LDS edges inside
  one tape;  4. a skipped chunk mid-tape;  5. invariance;  6. steps without a truth;  7. the trace against its model;  8. the ring's
  rules;  9. refusals;  10. buffers that grow;  11. a whole run against the reference's numbers;  12. slam-backend."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT, bits_equal

import ekf_ens_run_model as M
from test_gpu_ekf_ens import cfg_of, errors, known_host, observations, symmetric, synthetic_state, within

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
LM = np.array([[15.0, 5.0], [10.0, -12.0], [-8.0, 14.0], [25.0, 20.0], [30.0, -6.0], [18.0, 16.0], [5.0, 22.0], [40.0, 4.0]])
INVALID, CAPACITY = -1, -3


def make(members, max_landmarks, seed=1234, **over):
    import slam_amd
    sim, _, nz = known_host()
    return slam_amd.EkfEnsemble(members, max_landmarks, **cfg_of(sim.conf, **over), seed=seed), nz, sim.conf


def close(*handles):
    for h in handles:
        h.close()


# ---- 1. route equivalence, gates ----------------------------------------------------------------------------------------------------
def test_routes_agree_with_the_gates():
    """3 members, 12 landmarks of room, heading observed, every noise drawn, 24 steps from a fresh filter: control-only steps, an
    observation step with nz = 0 (step 3), the first observation (step 5: dim 3 -> 3 + 2 n), steps that match and add at once (6, 15),
    two observation steps back to back (5 | 6, 15 | 16).  One call of 24, calls of 1 + 7 + 16 and the twin leave the same bits"""
    one, nz, c = make(3, 12, association_known=False)
    cut, _, _ = make(3, 12, association_known=False)
    twin, _, _ = make(3, 12, association_known=False)
    ob = {3: [], 5: [0, 1, 2, 3], 6: [0, 1, 2, 3, 4, 5], 10: [1, 4], 15: [0, 2, 5, 6], 16: [3, 6, 7], 22: [0, 1, 2, 3, 4, 5, 6, 7]}
    tape = M.world_tape(24, ob, nz["dt"], c.WHEELBASE, LM, seed=1)
    for e in (one, cut, twin):
        e.trace_enable(32)
    M.drive_run(one, tape, nz)
    M.drive_run(cut, tape, nz, cuts=[1, 7, 16])
    M.drive_single(twin, tape, nz)
    a, b, t = M.snapshot(one), M.snapshot(cut), M.snapshot(twin)
    assert not M.identical(a, t) and not M.identical(b, t), (M.identical(a, t), M.identical(b, t))
    assert (t["dims"] > 3 + 2 * 3).all() and t["trace_info"][1] == 24 and (t["acc"][:, 0] + t["acc"][:, 1] == 24).all()
    assert not bits_equal(t["x0"], t["x1"])  # every member its own noise
    close(one, cut, twin)


# ---- 2. route equivalence, known association ----------------------------------------------------------------------------------------
def test_routes_agree_with_the_known_association_and_a_step_that_does_not_fit():
    """max_landmarks 4; ids revisited; the fifth id arrives in step 9 and again in step 12: both steps are refused for every member
    (SLAMGPU_EKF_STATUS_CAPACITY), as in the twin; afterwards an id seen before the run finds its feature on both handles"""
    import slam_amd
    one, nz, c = make(3, 4)
    cut, _, _ = make(3, 4)
    twin, _, _ = make(3, 4)
    ob = {2: [0, 1], 4: [1, 2], 5: [0, 2, 3], 9: [0, 4, 1], 11: [3, 2], 12: [4], 14: [0, 1, 2, 3], 20: [3, 0]}
    tape = M.world_tape(24, ob, nz["dt"], c.WHEELBASE, LM, seed=2)
    pre = M.world_tape(2, {1: [2]}, nz["dt"], c.WHEELBASE, LM, seed=3)  # id 2 is seen before the run (feature 0)
    for e in (one, cut, twin):
        M.drive_single(e, pre, nz)
    M.drive_run(one, tape[:8], nz)
    assert not one.status().any()
    M.drive_run(one, tape[8:], nz)
    M.drive_run(cut, tape, nz, cuts=[1, 7, 16])
    M.drive_single(twin, tape[:9], nz)
    assert not twin.status().any()
    M.drive_single(twin, tape[9:10], nz)
    assert (twin.status() == slam_amd.EKF_STATUS_CAPACITY).all()
    M.drive_single(twin, tape[10:], nz)
    a, b, t = M.snapshot(one), M.snapshot(cut), M.snapshot(twin)
    assert not M.identical(a, t) and not M.identical(b, t), (M.identical(a, t), M.identical(b, t))
    assert (t["status"] == slam_amd.EKF_STATUS_CAPACITY).all() and (t["dims"] == 11).all()
    after = M.world_tape(1, {0: [2, 3]}, nz["dt"], c.WHEELBASE, LM, seed=4)  # the table was committed: ids 2 and 3 find their features
    for e in (one, cut, twin):
        M.drive_single(e, after, nz)
    a, b, t = M.snapshot(one), M.snapshot(cut), M.snapshot(twin)
    assert not M.identical(a, t) and not M.identical(b, t) and (t["dims"] == 11).all()
    close(one, cut, twin)


# ---- 3. chunk and LDS edges inside one tape ---------------------------------------------------------------------------------------------
def test_chunk_and_lds_edges_inside_one_tape():
    """72 landmarks of room, states of 70 uploaded, consecutive steps of nz = 3, 70, 0, 33, 64, 65: np changes from step to step and the
    launch's LDS is the largest step's"""
    one, nz, c = make(3, 72)
    twin, _, _ = make(3, 72)
    x0, P0 = synthetic_state(70, 17)
    rng = np.random.default_rng(70)
    for e in (one, twin):
        for b in range(3):
            e.upload(b, x0, P0)
    tape = []
    for k, n in enumerate((3, 70, 0, 33, 64, 65)):
        ids = rng.permutation(70)[:n].astype(np.int32)
        tape.append(M.step_dict(k, 0.4, 0.01, 0.1, nz["dt"], truth=x0[:3], observe=1, z_true=observations(x0, ids, rng).reshape(-1, 2), ids=ids))
    M.drive_run(one, tape, nz)
    M.drive_single(twin, tape, nz)
    a, t = M.snapshot(one), M.snapshot(twin)
    assert not M.identical(a, t), M.identical(a, t)
    assert not t["status"].any() and (t["dims"] == 143).all() and t["z"].shape == (3, 65, 2)
    for b in range(3):
        P = one.state(b)[1]
        assert symmetric(P) and not bits_equal(P, P0), b
    close(one, twin)


# ---- 4. a skipped chunk mid-tape ----------------------------------------------------------------------------------------------------------
def test_a_skipped_chunk_mid_tape():
    """test_edges' construction: landmark blocks of -4 I make the innovation covariance indefinite.  Step 2 of 5 sets
    SLAMGPU_EKF_STATUS_NOT_PD, steps 3 to 5 still run"""
    one, nz, c = make(3, 6, use_heading=False)
    twin, _, _ = make(3, 6, use_heading=False)
    part, _, _ = make(3, 6, use_heading=False)
    x0, P0 = synthetic_state(6, 3)
    Pbad = P0.copy()
    Pbad[3:, 3:] = -4.0 * np.eye(12, dtype=f32)
    z = observations(x0, np.arange(3), np.random.default_rng(11))
    for e in (one, twin, part):
        for b in range(3):
            e.upload(b, x0, Pbad)
    tape = [M.step_dict(k, 0.5, 0.02, 0.1, nz["dt"], truth=x0[:3]) for k in range(5)]
    tape[1].update(observe=1, z_true=z, ids=np.arange(3, dtype=np.int32))
    M.drive_run(one, tape, nz, noise=5)
    M.drive_single(twin, tape, nz, noise=5)
    M.drive_run(part, tape[:2], nz, noise=5)
    a, t = M.snapshot(one), M.snapshot(twin)
    assert not M.identical(a, t), M.identical(a, t)
    assert (t["status"] == 1).all() and (part.status() == 1).all() and (t["dims"] == 15).all()
    assert not bits_equal(part.slab(0)[1], one.slab(0)[1])  # the steps after the skipped chunk ran
    close(one, twin, part)


# ---- 5. invariance ----------------------------------------------------------------------------------------------------------------------
def test_a_member_does_not_depend_on_the_ensemble():
    """noise off: a member's slab depends on its state alone, not on the ensemble's size or its place in it (nine states; a three-member
    ensemble holds states 4, 0, 7).  Noise on: member b of three is member b of nine.  Two runs of one tape are identical"""
    nine, nz, c = make(9, 12, association_known=False)
    three, _, _ = make(3, 12, association_known=False)
    x0, P0 = synthetic_state(8, 21)
    rng = np.random.default_rng(6)
    states = []
    for b in range(9):
        x = x0.copy()
        x[:3] += rng.normal(0, 0.02, 3).astype(f32)
        states.append(x)
    pick = [4, 0, 7]
    for b in range(9):
        nine.upload(b, states[b], P0)
    for j, b in enumerate(pick):
        three.upload(j, states[b], P0)
    tape = []
    for k in range(6):
        idf = rng.permutation(8)[:5]
        tape.append(M.step_dict(k, 3.0, 0.03, 0.1, nz["dt"], truth=x0[:3], observe=int(k % 2), z_true=observations(x0, idf, rng), ids=idf.astype(np.int32)))
    M.drive_run(nine, tape, nz, noise=0)
    M.drive_run(three, tape, nz, noise=0)
    for j, b in enumerate(pick):
        (xa, Pa), (xb, Pb) = three.slab(j), nine.slab(b)
        assert bits_equal(xa, xb) and bits_equal(Pa, Pb), (j, b)
    assert not bits_equal(nine.slab(0)[0], nine.slab(1)[0])
    close(nine, three)
    runs = []
    for members in (9, 3, 9):
        e, _, _ = make(members, 12, association_known=False)
        for b in range(members):
            e.upload(b, states[b], P0)
        M.drive_run(e, tape, nz, noise=7)
        runs.append(M.snapshot(e))
        e.close()
    assert not M.identical(runs[0], runs[2])
    for b in range(3):
        assert M.same_bits(runs[1]["x%d" % b], runs[0]["x%d" % b]) and M.same_bits(runs[1]["P%d" % b], runs[0]["P%d" % b]), b
    assert not M.same_bits(runs[0]["x0"], runs[0]["x1"])


# ---- 6. steps without a truth ---------------------------------------------------------------------------------------------------------------
def test_steps_without_a_truth_leave_accumulators_and_trace_alone():
    one, nz, c = make(4, 8)
    twin, _, _ = make(4, 8)
    tape = M.world_tape(9, {4: [0, 1, 2]}, nz["dt"], c.WHEELBASE, LM, seed=5, truth_every=3)  # a truth at steps 0, 3, 6
    assert [d["truth"] is not None for d in tape] == [True, False, False] * 3
    for e in (one, twin):
        e.trace_enable(8)
    M.drive_run(one, tape, nz)
    M.drive_single(twin, tape, nz)
    a, t = M.snapshot(one), M.snapshot(twin)
    assert not M.identical(a, t), M.identical(a, t)
    assert list(a["trace_info"]) == [0, 3, 8] and list(a["tags"]) == [0, 3, 6]
    assert (a["acc"][:, 0] + a["acc"][:, 1] == 3).all() and (a["trace"][:, 0] + a["trace"][:, 1] == 4).all()
    close(one, twin)


# ---- 7. the trace against its model ---------------------------------------------------------------------------------------------------------
def test_trace_matches_its_model():
    """8 members, 12 steps from a fresh filter, set up as test_gpu_ekf_ens.py's accumulator test starts: no heading update, no control
    noise drawn (flags 6), the vehicle at rest at the very first step, so that Pvv = Gu Q Gu^T has rank 1 exactly and every member is
    "not counted".  On the twin the
    accumulators are zeroed before every step, so that consistency() after it holds the members' own values of that step; the model
    record is their float64 sum.  Counts are exact; a sum of `members` non-negative doubles is within (members - 1) 2^-53 of the true sum
    whatever the order, on both sides: members * 2^-52 relative between the two"""
    B = 8
    one, nz, c = make(B, 8, association_known=False, use_heading=False)
    twin, _, _ = make(B, 8, association_known=False, use_heading=False)
    tape = M.world_tape(12, {4: [0, 1, 2], 8: [0, 1, 2, 3], 9: [2, 3]}, nz["dt"], c.WHEELBASE, LM, seed=7)
    tape[0]["V"] = tape[0]["G"] = 0.0
    for e in (one, twin):
        e.trace_enable(16)
    vals = []
    for d in tape:
        twin.consistency_reset()
        M.drive_single(twin, [d], nz, noise=6)
        vals.append(twin.consistency())
    model = M.trace_records(vals)
    dev, tags = twin.trace_fetch(0, 12)
    assert list(tags) == list(range(12))
    print("ENS trace counted | not counted | inside per step:", dev[:, [0, 1, 3]].astype(int).tolist())
    assert np.array_equal(dev[:, [0, 1, 3]], model[:, [0, 1, 3]]) and (dev[:, 0] + dev[:, 1] == B).all()
    assert dev[0, 1] == B and dev[0, 0] == 0
    assert dev[1:, 0].sum() > 0
    for col in (2, 4, 5):
        assert (np.abs(dev[:, col] - model[:, col]) <= B * 2.0 ** -52 * np.abs(model[:, col])).all(), col
    M.drive_run(one, tape, nz, noise=6)
    rec, rtags = one.trace_fetch(0, 12)
    assert M.same_bits(rec, dev) and M.same_bits(rtags, tags)
    acc = one.consistency()
    assert rec[:, 0].sum() == acc[:, 0].sum() and rec[:, 1].sum() == acc[:, 1].sum() and rec[:, 3].sum() == acc[:, 3].sum()
    close(one, twin)


# ---- 8. the ring's rules ----------------------------------------------------------------------------------------------------------------------
def test_ring_rules():
    import slam_amd
    one, nz, c = make(3, 8)
    twin, _, _ = make(3, 8)
    tape = M.world_tape(12, {2: [0, 1], 6: [1, 2, 3], 10: [0, 4]}, nz["dt"], c.WHEELBASE, LM, seed=8)
    one.trace_enable(5)
    twin.trace_enable(64)
    M.drive_run(one, tape, nz, cuts=[4, 4, 4])
    M.drive_single(twin, tape, nz)
    assert one.trace_info() == (7, 12, 5) and twin.trace_info() == (0, 12, 64)
    rec, tags = one.trace_fetch(7, 5)
    want, wtags = twin.trace_fetch(7, 5)
    assert M.same_bits(rec, want) and M.same_bits(tags, wtags) and list(tags) == [7, 8, 9, 10, 11]
    out, st = np.full((2, 6), 777.25), np.full(2, 77, np.uint32)
    with pytest.raises(slam_amd.SlamGpuError) as ei:
        one.trace_fetch(6, 2, out=out, step=st)
    assert ei.value.code == INVALID and (out == 777.25).all() and (st == 77).all()
    # six traced steps in one call do not fit five records: refused before anything is applied
    more = M.world_tape(6, {1: [5, 6]}, nz["dt"], c.WHEELBASE, LM, seed=9)
    before = M.snapshot(one)
    with pytest.raises(slam_amd.SlamGpuError) as ei:
        M.drive_run(one, more, nz)
    assert ei.value.code == CAPACITY
    assert not M.identical(before, M.snapshot(one))
    # ... the table included: ids 5 and 6 are still new to both handles
    M.drive_run(one, more, nz, cuts=[3, 3])
    M.drive_single(twin, more, nz)
    a, t = M.snapshot(one), M.snapshot(twin)
    del a["trace_info"], a["trace"], a["tags"], t["trace_info"], t["trace"], t["tags"]
    assert not M.identical(a, t) and (t["dims"] == 3 + 2 * 7).all()
    assert one.trace_info() == (13, 18, 5)
    one.trace_enable(0)
    M.drive_run(one, more[:2], nz)
    assert one.trace_info() == (0, 0, 0)
    with pytest.raises(slam_amd.SlamGpuError):
        one.trace_fetch(0, 0)
    close(one, twin)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    import slam_amd
    from slam_amd import ekf_ens
    one, nz, c = make(3, 8)
    ref, _, _ = make(3, 8)
    pre = M.world_tape(3, {2: [0, 1]}, nz["dt"], c.WHEELBASE, LM, seed=10)
    M.drive_run(one, pre, nz)
    M.drive_run(ref, pre, nz)
    good = M.world_tape(5, {1: [0, 2], 2: [3, 4], 4: [1, 5]}, nz["dt"], c.WHEELBASE, LM, seed=11)
    steps, z_true, ids = slam_amd.pack_tape(good)

    def run(s=steps, z=z_true, i=ids, Q=nz["Q"], noise=7):
        one.run_noise(s, z, i, Q, nz["Re"], nz["R"], Qe=nz["Qe"], noise=noise)

    past = steps.copy()
    past["nz"][4] = 3  # first + nz > total
    far = ids.copy()
    far[2] = 1 << 20
    twice = ids.copy()
    twice[3] = twice[2]  # step 2 (the third of five) names an unseen id twice
    neg = steps.copy()
    neg["first"][1] = -1
    bad = (lambda: run(s=past), lambda: run(i=far), lambda: run(i=twice), lambda: run(noise=8), lambda: run(s=neg),
           lambda: run(s=np.zeros(4097, slam_amd.TAPE_STEP_DTYPE)), lambda: run(Q=np.zeros((2, 2), f32)), lambda: run(i=None), lambda: run(z=None, i=None))
    for k, call in enumerate(bad):
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            call()
        assert ei.value.code == INVALID, k
    L = ekf_ens._lib()
    assert L.slamgpu_ens_run_noise(one.h, None, 3, None, None, 0, nz["Q"].ctypes.data_as(C.c_void_p), None, None, None, 7) == INVALID
    run(s=steps[:0])  # K = 0: returns 0 and changes nothing
    assert not M.identical(M.snapshot(one), M.snapshot(ref))
    # the table has learnt nothing from the refused tapes: the good tape teaches both handles the same
    run()
    M.drive_single(ref, good, nz)
    assert not M.identical(M.snapshot(one), M.snapshot(ref)) and (one.dims() == 3 + 2 * 6).all()
    close(one, ref)


# ---- 10. buffers that grow ------------------------------------------------------------------------------------------------------------------
def test_grown_buffers_run_as_a_fresh_handle():
    """40 steps of 30 observations: a tape of 17 KB against the first pinned slot's 4 KB; then a small run on the grown handle"""
    one, nz, c = make(3, 30)
    twin, _, _ = make(3, 30)
    x0, P0 = synthetic_state(30, 5)
    rng = np.random.default_rng(12)
    for e in (one, twin):
        for b in range(3):
            e.upload(b, x0, P0)
        e.trace_enable(64)
    M.drive_run(one, [M.step_dict(0, 0.3, 0.0, 0.1, nz["dt"])], nz)  # a small run first: every buffer at its first size
    M.drive_single(twin, [M.step_dict(0, 0.3, 0.0, 0.1, nz["dt"])], nz)
    ids = np.arange(30, dtype=np.int32)
    big = [M.step_dict(1 + k, 0.3, 0.01, 0.1, nz["dt"], truth=x0[:3], observe=1, z_true=observations(x0, ids, rng), ids=ids) for k in range(40)]
    small = [M.step_dict(50 + k, 0.3, 0.01, 0.1, nz["dt"], truth=x0[:3], observe=k == 1, z_true=observations(x0, ids[:2], rng), ids=ids[:2]) for k in range(3)]
    M.drive_run(one, big, nz)
    M.drive_run(one, small, nz)
    M.drive_single(twin, big + small, nz)
    a, t = M.snapshot(one), M.snapshot(twin)
    assert not M.identical(a, t), M.identical(a, t)
    assert t["trace_info"][1] == 43 and not t["status"].any()
    close(one, twin)


# ---- 11. a whole run against the reference's numbers ------------------------------------------------------------------------------------------
def test_whole_run_against_the_reference():
    """The first 400 control steps of example_webmap seed 7 as the host run fed them to its filter (tests/test_gpu_ekf.py: host_run), taken
    as the noise-free tape with every noise off: each member gets exactly those inputs.  Four runs of 100, 4 members, known association.
    After every batch: every member is member 0 bit for bit, the dimension is the host filter's on the same steps (slamhost fed them), and
    the error rule of tests/test_gpu_ekf_ens.py holds against the float64 model, the host filter's error the yardstick (factor 4)"""
    import slam_amd
    import ekf_model
    import test_gpu_ekf as T
    from slam_amd import host
    run = T.host_run("webmap")
    c, nz = run["conf"], run["noise"]
    hsim = host.HostSim(["-m", os.path.join(DATA, "example_webmap.mat"), "-method", "EKF1", "-SWITCH_ASSOCIATION_KNOWN", 1])
    hekf = host.HostEkf(hsim)
    cfg = cfg_of(c, association_known=True)
    B = 4
    ens = slam_amd.EkfEnsemble(B, run["nlm"], **cfg)
    mdl = ekf_model.EkfModel(**cfg)
    nzq = dict(Q=nz["Q"], Qe=nz["Qe"], Re=nz["Re"], R=nz["R"])
    for batch in range(4):
        tape = []
        for k in range(100 * batch, 100 * batch + 100):
            s = run["steps"][k]
            tape.append(M.step_dict(k, s["V"], s["G"], s["phi"], nz["dt"], observe=int(s["ob"]), z_true=s["z"], ids=s["vis"]))
            args = (s["V"], s["G"], nz["Qe"], nz["dt"], s["phi"], s["z"], s["vis"], nz["Re"], nz["R"], int(s["ob"]))
            mdl.sim(*args)
            hekf.sim_step(*args)
        M.drive_run(ens, tape, nzq, noise=0)
        xh, Ph = hekf.state()
        x0, P0 = ens.slab(0)
        for b in range(1, B):
            xb, Pb = ens.slab(b)
            assert bits_equal(xb, x0) and bits_equal(Pb, P0), (batch, b)
        xd, Pd = ens.state(0)
        assert (ens.dims() == xh.shape[0]).all() and mdl.dim == xh.shape[0], batch
        hx, hP = errors(xh, Ph, mdl.x, mdl.P)
        dx, dP = errors(xd, Pd, mdl.x, mdl.P)
        print("ENS run batch %d: dim %d, device x %.3e P %.3e, host x %.3e P %.3e" % (batch, xh.shape[0], dx, dP, hx, hP))
        assert within(dx, hx) and within(dP, hP), (batch, dx, hx, dP, hP)
    assert not ens.status().any() and ens.dims()[0] > 3
    close(ens, hekf, hsim)


# ---- 12. slam-backend -----------------------------------------------------------------------------------------------------------------------
def test_backend_prints_the_same_for_every_batch_size(tmp_path):
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")

    def run(batch, trace=None):
        cmd = [exe, "-m", os.path.join(DATA, "example_loop1.mat"), "-method", "EKF1", "-ekf", "device", "-runs", "8", "-maxsteps", "300", "-RUNS_BATCH", str(batch)]
        if trace:
            cmd += ["-RUNS_TRACE", trace]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return re.sub(r"[0-9.e+]+ us per control step of the ensemble, [0-9.e+]+ filter-steps per second", "T us per control step, F filter-steps per second", r.stdout)

    tr = str(tmp_path / "trace.txt")
    outs = [run(1), run(7, tr), run(256)]
    assert outs[0].splitlines() == outs[1].splitlines() == outs[2].splitlines()
    assert "control steps 300," in outs[0] and "T us per control step" in outs[0]
    rows = np.loadtxt(tr).reshape(-1, 6)
    assert rows.shape[0] == 300 and list(rows[:, 0]) == list(range(300)) and (rows[:, 4] + rows[:, 5] == 8).all()
    counted = int(re.search(r"pose NEES over (\d+) member-steps", outs[0]).group(1))
    skipped = int(re.search(r"member-steps not counted \(.*\): (\d+)", outs[0]).group(1))
    assert rows[:, 4].sum() == counted and rows[:, 5].sum() == skipped and counted + skipped == 8 * 300
