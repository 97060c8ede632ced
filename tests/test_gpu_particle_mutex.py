"""Mutual exclusion for contested landmarks (slamgpu_set_particle_mutex, pp_mutex_kernel): a landmark slot two observations of a step
name goes, per particle, to the claimant with the smallest (class, nd, q); the losers are re-matched in ascending q or discarded, and
the step runs on the final labels.

Yardsticks: tests/mutex_model.py fed float64 gate values (constructed cases, whose decisions have margins of 0.01 and more against a
float32 error of about 1e-4); invariants that need no tolerance on the dense map; and, everywhere, a TWIN context with mutual exclusion
off that is stepped with slamgpu_update_labels(F) -- the state must stay bit for bit the same, because with no slot twice in F the first
claim rule has nothing left to decide.  Every check prints its figures before it asserts."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA
from mutex_model import COUNTERS, DISCARD, NEW, mutex_model
from test_gpu_particle_device import EXCL_OFF, EXCL_ON, EXE, ERR_INVALID, REPORT, _course, _ctx, _finish, _host_step, _opt, _same_state
from test_gpu_particle_lists import _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
LISTS, EXHAUSTIVE = 3, 1
GATE = 4.0
R_C = np.array([0.01, 0.0, 0.0, (np.pi / 180) ** 2], f32)
A, B = 0, 1


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _gate(d, i, j, z):
    """float64 (nis, nd) of observation z against slot j of particle i of a downloaded / uploaded state (NaN: absent)"""
    xv = np.asarray(d["xv"][i], f64)
    lx, ly = (float(v) for v in d["xf"][i, j])
    P = np.asarray(d["Pf"][i, j], f64)
    dx, dy = lx - xv[0], ly - xv[1]
    d2 = dx * dx + dy * dy
    r = np.sqrt(d2)
    H = np.array([[dx / r, dy / r], [-dy / d2, dx / d2]])
    S = H @ P @ H.T + R_C.astype(f64).reshape(2, 2)
    v = np.array([z[0] - r, z[1] - (np.arctan2(dy, dx) - xv[2])])
    v[1] = (v[1] + np.pi) % (2 * np.pi) - np.pi
    with np.errstate(invalid="ignore"):  # (an absent record: NaN throughout)
        nis = float(v @ np.linalg.solve(S, v))
        return nis, nis + float(np.log(np.linalg.det(S)))


def _stats_of(s):
    st = s.particle_mutex_stats()
    return np.array([st[k] for k in COUNTERS], np.int64)


# ---- 1. constructed contests ---------------------------------------------------------------------------------------------------------
NEAR = [(10.0, 0.0), (10.0, 0.03)]
FAR = [(10.0, 0.0), (10.0, 0.3)]
# slots, step-2 observations, exclusion rule, L0, wanted F, (contested, lost, rematched, overturned) per particle
CASES = {
    "overturn+rematch": (NEAR, [(10.0, 0.012), (10.0, 0.002)], EXCL_OFF, [A, A], [B, A], (1, 1, 1, 1)),
    "incumbent_keeps": (NEAR, [(10.0, 0.002), (10.0, 0.012)], EXCL_OFF, [A, A], [A, B], (1, 1, 1, 0)),
    "no_alternative": (NEAR, [(10.0, -0.03), (10.0, 0.002)], EXCL_OFF, [A, A], [DISCARD, A], (1, 1, 0, 1)),
    "gated_beats_rule": (FAR, [(10.5, 0.0), (10.0, 0.002)], EXCL_ON, [A, A], [DISCARD, A], (1, 1, 0, 1)),
}


def _constructed(sg, method, math, case, mode, mutex, labels=None):
    """step 1 opens A and B; step 2 is the case (labels given: through update_labels instead).  Returns labels, counters, state before
    step 2 and after it"""
    slots, obs, excl, _, _, _ = CASES[case]
    N = 256
    s = sg.SlamGpu(N, 16, method=method, n_effective=N // 2, resample=False, rng_mode=sg.RNG_PHILOX, seed=5, math_mode=math, particle_maps=True)
    if mutex:
        s.set_particle_mutex(1)
    opt = _opt(excl, 1, 0.0, mode)
    r1 = s.update_particle(np.array(slots, f32), R_C, **opt)
    assert r1["opened"] == 2, r1
    before = s.download()
    if labels is None:
        s.update_particle(np.array(obs, f32), R_C, **opt)
        lab = s.particle_labels()
    else:
        s.update_labels(np.array(obs, f32), R_C, np.tile(np.array(labels, np.int32), (N, 1)), new_share=0.0, p_new=0.05, census_every=1)
        lab = None
    st = _stats_of(s)
    after = s.download()
    s.close()
    return lab, st, before, after


def _same_download(a, b, what):
    assert a["nf"] == b["nf"], what
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("method,math", [(1, 1), (2, 1), (1, 0), (2, 0)], ids=["fs1_fast", "fs2_fast", "fs1_strict", "fs2_strict"])
def test_constructed_contests(sg, method, math, case):
    slots, obs, excl, L0, want, counts = CASES[case]
    N = 256
    lab, st, before, after = _constructed(sg, method, math, case, EXHAUSTIVE, True)
    lab_l, st_l, _, after_l = _constructed(sg, method, math, case, LISTS, True)
    lab_off, st_off, _, after_off = _constructed(sg, method, math, case, EXHAUSTIVE, False)
    # the model on the float64 gates of the state the step met gives the wanted labels (and says how wide the decisions are)
    g = np.array([[_gate(before, 0, j, z) for j in range(2)] for z in obs])
    Fm, cm = mutex_model(L0, g[:, :, 0], g[:, :, 1], [True, True], GATE)
    print("mutex constructed %s m%d math%d: nis %s nd %s; device labels %s (lists %s, off %s); counters %s; finite state %s" %
          (case, method, math, g[:, :, 0].round(3).tolist(), g[:, :, 1].round(3).tolist(), lab[0].tolist(), lab_l[0].tolist(), lab_off[0].tolist(),
           st.tolist(), bool(np.isfinite(after["xv"]).all())))
    assert Fm.tolist() == want and tuple(cm[k] for k in COUNTERS[1:]) == counts
    assert lab.shape == (N, 2) and np.all(lab == np.array(want, np.int32)[None, :])
    assert np.array_equal(lab_l, lab), "exhaustive and lists disagree"
    assert st.tolist() == [2] + [N * v for v in counts] and np.array_equal(st_l, st)
    # off: today's labels (the first claim keeps the slot, the second one pays p_new), nothing counted
    assert np.all(lab_off == np.array(L0, np.int32)[None, :]) and not st_off.any()
    _, _, _, first_claim = _constructed(sg, method, math, case, EXHAUSTIVE, False, labels=L0)
    _same_download(after_off, first_claim, "off vs update_labels(L0)")
    # on: bit for bit the twin (mutual exclusion off) stepped with update_labels(F)
    _, _, _, twin = _constructed(sg, method, math, case, EXHAUSTIVE, False, labels=want)
    _same_download(after, twin, "on vs twin with update_labels(F)")
    _same_download(after_l, twin, "on (lists) vs twin")
    if want != L0 and DISCARD not in want:
        assert not np.array_equal(after["xf"], after_off["xf"], equal_nan=True), "the re-match changed nothing in the map"


# ---- 2. particles that disagree ------------------------------------------------------------------------------------------------------
def test_particles_that_disagree(sg):
    """N = 4 096 at the origin with headings +-(0.002 .. 0.006): both observations are nearest to A for everybody, q1 wins where the
    heading is positive and q0 where it is negative, the loser goes to B where B is held and is discarded where it is absent"""
    N = 4096
    i = np.arange(N)
    th = (0.002 + 0.004 * (i % 512) / 512.0) * np.where(i % 2 == 0, 1.0, -1.0)
    xv = np.zeros((N, 3), f32)
    xv[:, 2] = th
    xf = np.zeros((N, 2, 2), f32)
    Pf = np.zeros((N, 2, 2, 2), f32)
    Rm = R_C.astype(f64).reshape(2, 2)
    for j, (r, b) in enumerate(NEAR):
        Gz = np.array([[np.cos(b), -r * np.sin(b)], [np.sin(b), r * np.cos(b)]])
        xf[:, j] = (r * np.cos(b), r * np.sin(b))
        Pf[:, j] = Gz @ Rm @ Gz.T
    absent = i % 4 == 3
    xf[absent, B] = np.nan
    st = dict(nf=2, xv=xv, Pv=np.zeros((N, 3, 3), f32), w=np.full(N, 1.0 / N, f32), xf=xf, Pf=Pf)
    obs = [(10.0, 0.008), (10.0, -0.008)]

    def run(mode, math):
        s = sg.SlamGpu(N, 16, method=sg.FASTSLAM1, n_effective=N // 2, resample=False, rng_mode=sg.RNG_PHILOX, seed=5, math_mode=math, particle_maps=True)
        s.upload(st)
        s.set_particle_mutex(1)
        s.update_particle(np.array(obs, f32), R_C, **_opt(EXCL_OFF, 1, 0.0, mode))
        lab, cnt = s.particle_labels(), _stats_of(s)
        s.close()
        return lab, cnt
    # float64 gates of the uploaded state, the nearest-neighbour labels from them, the model, and every decision's margin
    want = np.zeros((N, 2), np.int64)
    total = np.zeros(5, np.int64)
    margin = np.inf
    for k in range(N):
        g = np.array([[_gate(st, k, j, z) for j in range(2)] for z in obs])
        nis, nd = g[:, :, 0], g[:, :, 1]
        held = np.array([True, not absent[k]])
        L0 = []
        for q in range(2):
            cand = [j for j in range(2) if held[j] and nis[q, j] < GATE]
            L0.append(min(cand, key=lambda j: nd[q, j]))
            margin = min(margin, GATE - nis[q, A])                                  # q gates A ...
            if held[B]:
                margin = min(margin, nd[q, B] - nd[q, A])                           # ... and A is the nearer
        assert L0 == [A, A], (k, L0)
        margin = min(margin, abs(nd[0, A] - nd[1, A]))                              # the contest
        loser = 0 if nd[1, A] < nd[0, A] else 1
        if held[B]:
            margin = min(margin, GATE - nis[loser, B])                              # the re-match
        F, cnt = mutex_model(L0, np.where(held[None, :], nis, np.nan), nd, held, GATE)
        want[k] = F
        total += np.array([cnt[c] for c in COUNTERS])
    total[0] = 1
    print("mutex disagree: smallest float64 margin of any decision %.4f; wanted labels: q1 keeps A for %d, q0 for %d, losers to B %d, discarded %d; counters %s" %
          (margin, int((want[:, 1] == A).sum()), int((want[:, 0] == A).sum()), int((want == B).sum()), int((want == DISCARD).sum()), total.tolist()))
    assert margin >= 0.01, "the geometry leaves a decision within float32's reach: change the geometry"
    assert np.array_equal(want[:, 1] == A, th > 0) and np.array_equal((want == DISCARD).any(axis=1), absent)
    for mode, math in ((EXHAUSTIVE, 1), (LISTS, 1), (EXHAUSTIVE, 0)):
        lab, cnt = run(mode, math)
        bad = np.nonzero((lab != want).any(axis=1))[0]
        print("mutex disagree mode %d math %d: %d particles differ from the model %s; counters %s" % (mode, math, len(bad), bad[:5].tolist(), cnt.tolist()))
        assert len(bad) == 0 and np.array_equal(cnt, total)


# ---- 3. dense map: invariants that need no tolerance --------------------------------------------------------------------------------
def _derived(L0, F, nf):
    """the invariants of one step for every particle at once, and the counter increments (L0, F) imply"""
    N, nz = L0.shape
    rows = np.repeat(np.arange(N), nz).reshape(N, nz)
    qs = np.tile(np.arange(nz), (N, 1))

    def scatter_count(lab, mask):
        c = np.zeros((N, nf), np.int32)
        np.add.at(c, (rows[mask], lab[mask]), 1)
        return c
    named = L0 >= 0
    claims = scatter_count(L0, named)
    contested = claims >= 2
    assert scatter_count(F, F >= 0).max(initial=0) <= 1, "a slot twice in F"
    in_contest = np.zeros((N, nz), bool)
    in_contest[named] = contested[rows[named], L0[named]]
    changed = F != L0
    assert not (changed & ~in_contest).any(), "a label changed that was not a contested claim"
    kept = in_contest & ~changed
    keepers = scatter_count(L0, kept)
    assert np.array_equal(keepers[contested], np.ones(int(contested.sum()), np.int32)), "a contested slot not kept by exactly one of its claimants"
    assert not keepers[~contested & (claims == 0)].any()
    losers = in_contest & changed
    assert not (F[losers] == NEW).any(), "a loser became NEW"
    assert ((F[losers] >= 0) | (F[losers] == DISCARD)).all()
    first = np.full((N, nf), nz, np.int32)
    np.minimum.at(first, (rows[named], L0[named]), qs[named])
    keeper_q = np.full((N, nf), -1, np.int32)
    keeper_q[rows[kept], L0[kept]] = qs[kept]
    overturned = contested & (keeper_q != first)
    return np.array([1, contested.sum(), (claims - 1)[contested].sum(), (F[losers] >= 0).sum(), overturned.sum()], np.int64)


@pytest.mark.parametrize("method,math", [(2, 1), (1, 0)], ids=["fs2_fast", "fs1_strict"])
def test_dense_map_invariants(sg, tmp_path_factory, method, math):
    N, cap, steps = 4096, 960, 40
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2" if method == 2 else "FASTSLAM1", steps, max_range=20)
    opt = _opt(EXCL_OFF, 1, 0.02, EXHAUSTIVE)
    on, twin, off = (_ctx(sg, c, N, method, math, cap) for _ in range(3))
    on.set_particle_mutex(1)
    prev = _stats_of(on)
    assert not prev.any()
    for k in range(steps):
        for s in (on, twin):
            for V, G, phi in c["ctl"][k]:
                s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
        z = on.observe(c["xt"][k], c["max_range"], c["R"], noise=2)["z"]
        zt = twin.observe(c["xt"][k], c["max_range"], c["R"], noise=2)["z"]
        assert len(z) > 0 and np.array_equal(z, zt)
        nf = on.nf()
        L0 = on.associate(z, c["R"], mode=EXHAUSTIVE)[0]
        ra = on.update_particle(z, c["R"], **opt)
        F = on.particle_labels()
        rb = twin.update_labels(z, c["R"], F, new_share=0.02, p_new=0.05, census_every=1)
        assert ra == rb, (k, ra, rb)
        on.estimate_async()
        twin.estimate_async()
        now = _stats_of(on)
        want = _derived(L0, F, max(nf, 1))
        assert np.array_equal(now - prev, want), (k, (now - prev).tolist(), want.tolist())
        prev = now
        _host_step(off, c, k, opt)
    print("mutex dense m%d math%d: %d steps, counters %s, slots %d" % (method, math, steps, prev.tolist(), on.nf()))
    assert prev[1] > 0 and prev[3] > 0, "nothing was contested / re-matched on the dense map"
    a, b, o = _finish(on), _finish(twin), _finish(off)
    _same_state(a, b, "mutual exclusion vs its twin stepped with update_labels(F)")
    assert not (a[1]["nf"] == o[1]["nf"] and np.array_equal(a[1]["xv"], o[1]["xv"])), "mutual exclusion never changed the run"


# ---- 4. every path gives one run -----------------------------------------------------------------------------------------------------
def _dev(sg, c, N, method, math, opt, K, steps, cap, mutex, miss):
    d = _ctx(sg, c, N, method, math, cap)
    d.set_particle_mutex(mutex)
    if miss:
        d.set_particle_miss(0.5, 17.0, 3.0)
    for a in range(0, steps, K):
        d.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], c["xt"][a:a + K], c["max_range"], c["R"], noise=2, **opt)
    rep, st = d.particle_report_fetch(), _stats_of(d)
    missed = d.particle_miss_stats() if miss else None
    return _finish(d), rep, st, missed


def _host(sg, c, N, method, math, opt, steps, cap, mutex, miss):
    s = _ctx(sg, c, N, method, math, cap)
    s.set_particle_mutex(mutex)
    if miss:
        s.set_particle_miss(0.5, 17.0, 3.0)
    rep = np.array([_host_step(s, c, k, opt) for k in range(steps)])
    st = _stats_of(s)
    missed = s.particle_miss_stats() if miss else None
    return _finish(s), rep, st, missed


@pytest.mark.parametrize("miss", [False, True], ids=["plain", "miss"])
def test_paths_agree_on_the_dense_map(sg, tmp_path_factory, miss):
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2", 40, max_range=20)
    N, cap = 4096, 960
    ex, rex, sex, mex = _dev(sg, c, N, 2, 1, _opt(EXCL_OFF, 1, 0.02, EXHAUSTIVE), 20, 40, cap, 1, miss)
    li, rli, sli, mli = _dev(sg, c, N, 2, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 20, 40, cap, 1, miss)
    os.environ["SLAMGPU_ASSOC_LCAP"] = "1"
    try:
        lo, rlo, slo, mlo = _dev(sg, c, N, 2, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 20, 40, cap, 1, miss)
    finally:
        del os.environ["SLAMGPU_ASSOC_LCAP"]
    ho, rho, sho, mho = _host(sg, c, N, 2, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 40, cap, 1, miss)
    print("mutex paths miss=%s: counters %s %s %s %s; missed %s" % (miss, sex.tolist(), sli.tolist(), slo.tolist(), sho.tolist(), mex))
    assert rex[:, 3].sum() == 0, "slots ran out"
    for r, what in ((rli, "lists"), (rlo, "overflow"), (rho, "host")):
        assert np.array_equal(rex, r), (what, np.argwhere(rex != r)[:5])
    for s_, what in ((sli, "lists"), (slo, "overflow"), (sho, "host")):
        assert np.array_equal(sex, s_), what
    assert sex[1] > 0 and sex[3] > 0
    if miss:
        key = lambda m: (m["steps"], m["missed"], m["particles"])
        assert key(mex) == key(mli) == key(mlo) == key(mho) and mex["missed"] > 0
    _same_state(ex, li, "exhaustive vs lists")
    _same_state(li, lo, "lists vs overflow walk")
    _same_state(li, ho, "device vs host")


# ---- 5. where nothing is contested ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [EXHAUSTIVE, LISTS], ids=["exhaustive", "lists"])
def test_uncontested_run_is_todays(sg, mode):
    c = _course("FASTSLAM2", 150)
    opt = _opt(EXCL_OFF, 1, 0.02, mode)
    off, roff, _, _ = _dev(sg, c, 1000, 2, 1, opt, 50, 150, None, 0, False)
    on, ron, st, _ = _dev(sg, c, 1000, 2, 1, opt, 50, 150, None, 1, False)
    print("mutex uncontested mode %d: counters %s" % (mode, st.tolist()))
    assert st[0] > 100 and not st[1:].any()
    assert np.array_equal(roff, ron)
    _same_state(off, on, "mutual exclusion on vs off, nothing contested")


# ---- 6. off means off, refusals, launches --------------------------------------------------------------------------------------------
def test_off_refusals_and_launches(sg):
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, rng_mode=sg.RNG_PHILOX, particle_maps=True)
    assert not _stats_of(s).any()
    for bad in (2, -1):
        with pytest.raises(sg.SlamGpuError) as e:
            s.set_particle_mutex(bad)
        assert e.value.code == ERR_INVALID
    s.set_particle_assoc_sampling(1)
    with pytest.raises(sg.SlamGpuError) as e:
        s.set_particle_mutex(1)
    assert e.value.code == ERR_INVALID
    s.set_particle_assoc_sampling(0)
    s.set_particle_mutex(1)
    with pytest.raises(sg.SlamGpuError) as e:
        s.set_particle_assoc_sampling(1)
    assert e.value.code == ERR_INVALID
    s.set_particle_mutex(0)
    s.set_particle_assoc_sampling(1)
    s.close()
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, rng_mode=sg.RNG_PHILOX)
    with pytest.raises(sg.SlamGpuError) as e:
        s.set_particle_mutex(1)
    assert e.value.code == ERR_INVALID and "SLAMGPU_FLAG_PARTICLE_MAPS" in str(e.value)
    s.close()
    c = _course("FASTSLAM2", 40)
    opt = _opt(EXCL_ON, 1, 0.02, LISTS)
    for mutex in (0, 1):
        d = _ctx(sg, c, 1000, 2, 1)
        h = _ctx(sg, c, 1000, 2, 1)
        for s in (d, h):
            s.profile(True)
            if mutex:
                s.set_particle_mutex(1)
        d.run_particle(c["ctl"][:40], c["Q"], c["dt"], c["xt"][:40], c["max_range"], c["R"], noise=2, **opt)
        rep = d.particle_report_fetch()
        with_obs = int((rep[:, REPORT.index("need")] > 0).sum())
        hrep = np.array([_host_step(h, c, k, opt) for k in range(40)])
        got = (d.kernel_time("particle_mutex")[1], h.kernel_time("particle_mutex")[1])
        book = d.kernel_time("particle_book")[1]
        steps = (_stats_of(d)[0], _stats_of(h)[0])
        d.close()
        h.close()
        print("mutex launches: on=%d device %d host %d (iterations with observations %d, particle_book %d)" % (mutex, got[0], got[1], with_obs, book))
        assert with_obs == 40 and np.array_equal(rep, hrep)
        assert got == ((40, 40) if mutex else (0, 0)) and steps == ((40, 40) if mutex else (0, 0))


# ---- 7. slam-backend -----------------------------------------------------------------------------------------------------------------
def test_slam_backend_particle_mutex():
    base = [EXE, "-m", os.path.join(DATA, "example_loop1.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384", "-SWITCH_SEED_RANDOM", "7",
            "-assoc", "particle", "-observe", "device", "-rng", "philox", "-PARTICLE_ASSOC", "lists", "-maxsteps", "1500"]
    r = subprocess.run(base + ["-PARTICLE_MUTEX", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("mutual exclusion:")]
    print("slam-backend -PARTICLE_MUTEX 1:", line)
    assert len(line) == 1 and int(line[0].split()[2]) > 0
    r = subprocess.run(base + ["-PARTICLE_MUTEX", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "-PARTICLE_MUTEX" in r.stderr
