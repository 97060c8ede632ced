"""Data association sampling (slamgpu_set_particle_assoc_sampling): a (particle, observation) pair with two or more candidates C takes
the label argmax_{j in C} (-nd_j / 2 + g_j), g_j Gumbel noise from Philox stream 4 at (first_particle + i, step, 4 + 8 q, j), and a fresh
claim multiplies the weight factor by sum_k L_k / L_label.  Where nothing is ambiguous the run is the nearest neighbour's bit for bit; a
constructed ambiguous step shows the label frequencies, the documented draws and the marginal weights; on config 5's dense map every
path gives one run; refusals, launch counts and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_gpu_particle_device import (EXCL_OFF, EXE, ERR_INVALID, REPORT, _course, _ctx, _finish, _opt, _same_state)
from test_gpu_particle_lists import _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32 = np.float32
LISTS, EXHAUSTIVE = 3, 1
SEED = 5


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _dev(sg, c, N, method, math, opt, K, steps, cap, sample):
    d = _ctx(sg, c, N, method, math, cap)
    d.set_particle_assoc_sampling(sample)
    for a in range(0, steps, K):
        b = min(steps, a + K)
        d.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **opt)
    rep = d.particle_report_fetch()
    st = d.particle_sample_stats()
    return _finish(d), rep, st


def _host(sg, c, N, method, math, opt, steps, cap, sample):
    s = _ctx(sg, c, N, method, math, cap)
    s.set_particle_assoc_sampling(sample)
    reps = []
    for k in range(steps):
        for V, G, phi in c["ctl"][k]:
            s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
        o = s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)
        rep = np.zeros(8, np.int32)
        if len(o["z"]):
            r = s.update_particle(o["z"], c["R"], **opt)
            rep = np.array([r[f] for f in REPORT], np.int32)
        s.estimate_async()
        reps.append(rep)
    st = s.particle_sample_stats()
    return _finish(s), np.array(reps), st


@pytest.mark.parametrize("method,math", [(2, 1), (1, 0)], ids=["fs2_fast", "fs1_strict"])
def test_unambiguous_run_is_nearest_neighbour(sg, method, math):
    """example_webmap (landmarks 19.5 m apart or more), 150 iterations, N = 1 000: no pair has two candidates, and with sampling on the
    exhaustive scan and the lists give the nearest neighbour's reports and state bit for bit"""
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 150)
    for mode in (EXHAUSTIVE, LISTS):
        opt = _opt(EXCL_OFF, 1, 0.02, mode)
        ml, rml, _ = _dev(sg, c, 1000, method, math, opt, 50, 150, None, 0)
        sa, rsa, st = _dev(sg, c, 1000, method, math, opt, 50, 150, None, 1)
        assert st["steps"] > 0 and st["ambiguous"] == 0 and st["moved"] == 0, st
        assert np.array_equal(rml, rsa)
        _same_state(ml, sa, "sampling vs nearest neighbour, mode %d" % mode)


# ---- one constructed ambiguous step: every particle at the origin (FastSLAM 1 draws no pose in its update, no predict, no resample) ----
R_C = np.array([0.01, 0.0, 0.0, (np.pi / 180) ** 2], f32)
B_OFF = 0.03    # slot B's bearing (0.3 m to the side of A at 10 m)
B_OBS = 0.005   # the second step's bearing: between them, nearer A


def _ambiguous(sg, N, sample, mode=EXHAUSTIVE, logw=False):
    s = sg.SlamGpu(N, 16, method=sg.FASTSLAM1, n_effective=N // 2, resample=False, rng_mode=sg.RNG_PHILOX, seed=SEED, math_mode=sg.MATH_FAST,
                   particle_maps=True, log_weights=logw)
    s.set_particle_assoc_sampling(sample)
    opt = _opt(EXCL_OFF, 1, 0.0, mode)
    r1 = s.update_particle(np.array([[10.0, 0.0], [10.0, B_OFF]], f32), R_C, **opt)
    before = s.download()
    s.update_particle(np.array([[10.0, B_OBS]], f32), R_C, **opt)
    lab = s.particle_labels()
    st = s.particle_sample_stats()
    after = s.download()
    s.close()
    assert r1["opened"] == 2
    return before, lab, st, after


def _nd(d, i, j, z):
    """float64 nd = nis + ln det S of observation z against slot j of particle i"""
    xv = np.asarray(d["xv"][i], np.float64)
    lx, ly = (float(v) for v in d["xf"][i, j])
    P = np.asarray(d["Pf"][i, j], np.float64)
    dx, dy = lx - xv[0], ly - xv[1]
    d2 = dx * dx + dy * dy
    r = np.sqrt(d2)
    H = np.array([[dx / r, dy / r], [-dy / d2, dx / d2]])
    S = H @ P @ H.T + R_C.astype(np.float64).reshape(2, 2)
    v = np.array([z[0] - r, z[1] - (np.arctan2(dy, dx) - xv[2])])
    v[1] = (v[1] + np.pi) % (2 * np.pi) - np.pi
    return float(v @ np.linalg.solve(S, v) + np.log(np.linalg.det(S)))


def test_constructed_ambiguity_label_frequencies(sg):
    """two slots 0.3 m apart at 10 m, an observation between them: without sampling every particle takes A; with it the share of A is
    p_A = 1 / (1 + exp(-(nd_B - nd_A) / 2)) within 5 sigma, and the exhaustive scan and the lists draw the same labels"""
    N = 65536
    _, lab0, st0, _ = _ambiguous(sg, N, 0)
    assert lab0.shape == (N, 1) and np.all(lab0 == 0) and st0["steps"] == 0
    before, lab, st, _ = _ambiguous(sg, N, 1)
    _, lab_l, _, _ = _ambiguous(sg, N, 1, mode=LISTS)
    assert np.array_equal(lab, lab_l)
    z = (10.0, B_OBS)
    nda, ndb = _nd(before, 0, 0, z), _nd(before, 0, 1, z)
    pa = 1.0 / (1.0 + np.exp(-0.5 * (ndb - nda)))
    share = float(np.mean(lab[:, 0] == 0))
    sigma = np.sqrt(pa * (1 - pa) / N)
    print("p_A", pa, "share", share, "stats", st)
    assert np.all((lab == 0) | (lab == 1))
    assert abs(share - pa) < 5 * sigma, (share, pa, sigma)
    assert st["steps"] == 2 and st["ambiguous"] == N and st["moved"] == int(np.sum(lab[:, 0] == 1)), st


def test_the_documented_draws(sg):
    """every label is the host's argmax(-nd / 2 + g), g = -ln(-ln u) from the Philox integers at (i, step, 4 + 8 q, j), u = ((x >> 8) + 0.5)
    / 2^24; a pair whose two scores lie within 1e-4 may differ, at most 0.1 % of them"""
    from oracle import orc
    O = orc.Oracle()
    N = 8192
    before, lab, _, _ = _ambiguous(sg, N, 1)
    z = (10.0, B_OBS)
    nd = [_nd(before, 0, 0, z), _nd(before, 0, 1, z)]
    step = 2  # (the second update's own step: its association ran at obs_step 1)
    k = (SEED & 0xffffffff, SEED >> 32)
    sc = np.zeros((N, 2))
    for i in range(N):
        for j in range(2):
            x = int(O.philox((i, step, 4, j), k)[0])
            u = ((x >> 8) + 0.5) / 16777216.0
            sc[i, j] = -0.5 * nd[j] - np.log(-np.log(u))
    want = np.where(sc[:, 1] > sc[:, 0], 1, 0)
    bad = want != lab[:, 0]
    close = np.abs(sc[:, 1] - sc[:, 0]) < 1e-4
    assert np.all(close[bad]), np.argwhere(bad & ~close)[:5]
    assert bad.sum() <= 0.001 * N


@pytest.mark.parametrize("logw", [False, True], ids=["linear", "log"])
def test_marginal_weights(sg, logw):
    """resampling off: particles that drew A and particles that drew B end with the same weight (L_A rho_A = L_B rho_B = L_A + L_B), the
    geometry making L_A / L_B >= 1.5 so that a missing ratio would split them"""
    N = 4096
    before, lab, _, after = _ambiguous(sg, N, 1, logw=logw)
    z = (10.0, B_OBS)
    assert np.exp(-0.5 * (_nd(before, 0, 0, z) - _nd(before, 0, 1, z))) >= 1.5
    a, b = lab[:, 0] == 0, lab[:, 0] == 1
    assert a.any() and b.any()
    w = np.asarray(after["w"], np.float64)
    if logw:
        assert abs(w[a].mean() - w[b].mean()) <= 1e-5 * max(1.0, abs(w[a].mean())), (w[a][:3], w[b][:3])
    else:
        assert abs(w[a].mean() - w[b].mean()) <= 1e-5 * w[a].mean(), (w[a][:3], w[b][:3])
    for g in (a, b):
        assert np.all(w[g] == w[g][0])


@pytest.mark.parametrize("method", [2, 1], ids=["fs2", "fs1"])
def test_paths_agree_on_the_dense_map(sg, tmp_path_factory, method):
    """config 5's map at MAX_RANGE 20, N = 4 096, 40 iterations, sampling on: run_particle through the exhaustive scan, the lists and the
    lists with every list overflowing (SLAMGPU_ASSOC_LCAP=1), and the host twin through the lists, give one run; pairs were ambiguous,
    and the nearest neighbour's run ends elsewhere"""
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2" if method == 2 else "FASTSLAM1", 40, max_range=20)
    cap = 960  # (the exhaustive scan: particles x slots x map landmarks within its bound)
    ex, rex, sex = _dev(sg, c, 4096, method, 1, _opt(EXCL_OFF, 1, 0.02, EXHAUSTIVE), 20, 40, cap, 1)
    li, rli, sli = _dev(sg, c, 4096, method, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 20, 40, cap, 1)
    os.environ["SLAMGPU_ASSOC_LCAP"] = "1"
    try:
        lo, rlo, slo = _dev(sg, c, 4096, method, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 20, 40, cap, 1)
    finally:
        del os.environ["SLAMGPU_ASSOC_LCAP"]
    ho, rho, sho = _host(sg, c, 4096, method, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 40, cap, 1)
    print("sampling stats", sex, sli, slo, sho)
    assert rex[:, 3].sum() == 0, "slots ran out"
    for r, what in ((rli, "lists"), (rlo, "overflow"), (rho, "host")):
        assert np.array_equal(rex, r), (what, np.argwhere(rex != r)[:5])
    assert sex == sli == slo == sho, (sex, sli, slo, sho)
    assert sex["ambiguous"] > 0
    _same_state(ex, li, "exhaustive vs lists")
    _same_state(li, lo, "lists vs overflow walk")
    _same_state(li, ho, "device vs host")
    ml, _, _ = _dev(sg, c, 4096, method, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 20, 40, cap, 0)
    assert not (ml[1]["nf"] == li[1]["nf"] and np.array_equal(ml[1]["xv"], li[1]["xv"])), "sampling never changed a label"


def test_refusals_and_launch_counts(sg):
    """on outside {0, 1}, a context without per-particle maps and a TAPE context are refused; an iteration makes the same launches with
    sampling on as with it off"""
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, rng_mode=sg.RNG_PHILOX, particle_maps=True)
    for bad in (2, -1):
        with pytest.raises(sg.SlamGpuError) as e:
            s.set_particle_assoc_sampling(bad)
        assert e.value.code == ERR_INVALID
    s.close()
    for kw in (dict(rng_mode=sg.RNG_PHILOX), dict(rng_mode=sg.RNG_TAPE, particle_maps=True)):
        s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, **kw)
        with pytest.raises(sg.SlamGpuError) as e:
            s.set_particle_assoc_sampling(1)
        assert e.value.code == ERR_INVALID
        s.close()
    c = _course("FASTSLAM2", 40)
    names = ("resample", "gather", "predict", "observe", "excl_radii", "lmk_box", "assoc_geom_partial", "assoc_geom", "assoc_lists", "associate",
             "particle_book", "particle_resolve", "fs2_update", "finish", "estimate", "particle_census", "flatten", "scan")
    counts = []
    for mode in (LISTS, EXHAUSTIVE):
        for sample in (0, 1):
            opt = _opt(EXCL_OFF, 1, 0.02, mode)
            s = _ctx(sg, c, 1000, 2, 1)
            s.set_particle_assoc_sampling(sample)
            s.profile(True)
            s.run_particle(c["ctl"][:10], c["Q"], c["dt"], c["xt"][:10], c["max_range"], c["R"], noise=2, **opt)
            first = {n: s.kernel_time(n)[1] for n in names}
            s.run_particle(c["ctl"][10:40], c["Q"], c["dt"], c["xt"][10:40], c["max_range"], c["R"], noise=2, **opt)
            counts.append({n: s.kernel_time(n)[1] - first[n] for n in names})
            s.close()
    assert counts[0] == counts[1] and counts[2] == counts[3], counts
    assert counts[0]["associate"] == 30 and counts[2]["associate"] == 30


def test_slam_backend_option(tmp_path):
    """slam-backend -assoc particle -observe device -rng philox -PARTICLE_ASSOC lists -PARTICLE_ASSOC_SAMPLE 1 runs example_loop1 and prints
    its map and the counters; -PARTICLE_ASSOC_SAMPLE 2 is refused"""
    base = [EXE, "-m", os.path.join(DATA, "example_loop1.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
            "-SWITCH_SEED_RANDOM", "7", "-assoc", "particle", "-observe", "device", "-rng", "philox", "-PARTICLE_ASSOC", "lists"]
    r = subprocess.run(base + ["-PARTICLE_ASSOC_SAMPLE", "1", "-maxsteps", "3000", "-log", str(tmp_path / "a.csv")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("landmarks in map:") for ln in lines), r.stdout[-800:]
    assert any(ln.startswith("association sampling:") for ln in lines), r.stdout[-800:]
    bad = subprocess.run(base + ["-PARTICLE_ASSOC_SAMPLE", "2", "-maxsteps", "10"], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "PARTICLE_ASSOC_SAMPLE" in bad.stderr, bad.stderr[-400:]
