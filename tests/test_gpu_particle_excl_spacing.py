"""The exclusion rule's radius capped by the step's own observation spacing (slamgpu_set_particle_excl_spacing): observation q implies the
sensor-frame point p_q = r_q (cos b_q, sin b_q), s_q is its distance to the nearest other point of the step, and with a factor f > 0 the
rule's radius is min(excl_base + excl_per_m r_q, f s_q).  The radii are held to a float64 model of that definition, the device loop's
to its host twin's bit for bit; one constructed step shows the cap decide; every path (exhaustive scan, lists, host or device driven)
gives the same run; where the cap cannot bind the run is the fixed rule's; on a dense map the cap lets new landmarks in."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_gpu_particle_device import (EXCL_OFF, EXCL_ON, EXE, ERR_INVALID, REPORT, _course, _ctx, _finish, _opt, _same_state)
from test_gpu_particle_lists import _course_of, _synthetic, _visible

pytestmark = pytest.mark.gpu
f32 = np.float32
LISTS, EXHAUSTIVE = 3, 1


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _model(z, excl, f):
    """float64 model of the radii: rho_q = min(base + per_m r_q, f s_q), s_q the distance to the nearest other implied point"""
    z = np.asarray(z, f32).reshape(-1, 2).astype(np.float64)
    r, b = z[:, 0], z[:, 1]
    p = np.stack([r * np.cos(b), r * np.sin(b)], 1)
    s = np.full(len(p), np.inf)
    for a in range(0, len(p), 512):
        e = min(len(p), a + 512)
        d = np.sqrt(((p[a:e, None, :] - p[None, :, :]) ** 2).sum(-1))
        d[np.arange(e - a), np.arange(a, e)] = np.inf
        s[a:e] = d.min(1)
    return np.minimum(excl[0] + excl[1] * r, f * s)


def _spaced(s, f):
    s.set_particle_excl_spacing(f)
    return s


def _host_steps(s, c, opt, steps, radii=False):
    """the host twin: predicts, observe, update_particle, estimate per step; reports (and the radii fetched after each update)"""
    reps, rad = [], []
    for k in range(steps):
        for V, G, phi in c["ctl"][k]:
            s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
        o = s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)
        rep = np.zeros(8, np.int32)
        if len(o["z"]):
            r = s.update_particle(o["z"], c["R"], **opt)
            rep = np.array([r[f] for f in REPORT], np.int32)
            if radii:
                rad.append((np.array(o["z"]), s.particle_excl_radii()))
        s.estimate_async()
        reps.append(rep)
    return np.array(reps), rad


def _host(sg, c, N, method, math, opt, steps, cap, f):
    s = _spaced(_ctx(sg, c, N, method, math, cap), f)
    rep, _ = _host_steps(s, c, opt, steps)
    return _finish(s), rep


def _dev(sg, c, N, method, math, opt, K, steps, cap, f):
    d = _spaced(_ctx(sg, c, N, method, math, cap), f)
    for a in range(0, steps, K):
        b = min(steps, a + K)
        d.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **opt)
    rep = d.particle_report_fetch()
    return _finish(d), rep


@pytest.mark.parametrize("which", ["synthetic1000", "config5_range60"])
def test_radii_equal_the_definition(sg, tmp_path_factory, which):
    """the radii fetched after each host-driven step equal the float64 model within 1e-4 m (the 1 000-landmark map through the exhaustive
    scan, config 5's map at MAX_RANGE 60 through the lists)"""
    if which == "synthetic1000":
        c, mode, cap, steps = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 5), EXHAUSTIVE, 2000, 5
    else:
        c, mode, cap, steps = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2", 3, max_range=60), LISTS, 3000, 3
    f = 0.5
    s = _spaced(_ctx(sg, c, 256, 2, 1, cap), f)
    _, rad = _host_steps(s, c, _opt(EXCL_ON, 1, 0.02, mode), steps, radii=True)
    s.close()
    assert len(rad) == steps
    capped = 0
    for z, got in rad:
        want = _model(z, EXCL_ON, f)
        assert got.shape == want.shape and np.all(np.abs(got.astype(np.float64) - want) <= 1e-4), np.max(np.abs(got - want))
        capped += int(np.sum(want < EXCL_ON[0] + EXCL_ON[1] * np.asarray(z, np.float64)[:, 0]))
    assert capped > 0, "the cap never bound"
    if which == "config5_range60":
        assert min(len(z) for z, _ in rad) > 500


def test_radii_of_a_large_step_and_of_one_observation(sg):
    """5 000 observations in one update_particle (many blocks of the radius kernel), then a step of one observation (s = +inf: the
    fixed radius)"""
    rng = np.random.default_rng(3)
    z = np.stack([rng.uniform(1.0, 60.0, 5000), rng.uniform(-1.5, 1.5, 5000)], 1).astype(f32)
    R = np.array([0.01, 0.0, 0.0, 3e-4], f32)
    s = _spaced(sg.SlamGpu(256, 2000, method=sg.FASTSLAM1, n_effective=192, rng_mode=sg.RNG_PHILOX, seed=5, math_mode=sg.MATH_FAST,
                           particle_maps=True), 0.75)
    s.update_particle(z, R, **_opt(EXCL_ON, 1, 0.0, EXHAUSTIVE))
    got = s.particle_excl_radii()
    assert got.shape == (5000,) and np.all(np.abs(got.astype(np.float64) - _model(z, EXCL_ON, 0.75)) <= 1e-4)
    s.update_particle(np.array([[30.0, 0.2]], f32), R, **_opt(EXCL_ON, 1, 0.0, EXHAUSTIVE))
    one = s.particle_excl_radii()
    assert one.shape == (1,) and abs(float(one[0]) - (EXCL_ON[0] + EXCL_ON[1] * 30.0)) < 1e-5, one
    s.close()


def test_device_radii_equal_the_host_twin(sg, tmp_path_factory):
    """run_particle(LISTS) one iteration per call, the radii fetched after each: bit for bit the host twin's, and the same end state"""
    c = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 8)
    opt = _opt(EXCL_ON, 1, 0.02, LISTS)
    h = _spaced(_ctx(sg, c, 1024, 2, 1, 2000), 0.5)
    _, hrad = _host_steps(h, c, opt, 8, radii=True)
    host = _finish(h)
    d = _spaced(_ctx(sg, c, 1024, 2, 1, 2000), 0.5)
    drad = []
    for k in range(8):
        d.run_particle(c["ctl"][k:k + 1], c["Q"], c["dt"], c["xt"][k:k + 1], c["max_range"], c["R"], noise=2, **opt)
        if _visible(c, k):
            drad.append(d.particle_excl_radii())
    dev = _finish(d)
    assert len(hrad) == len(drad) == 8
    for (_, a), b in zip(hrad, drad):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _same_state(host, dev, "spacing rule, device vs host")


def _two_landmarks(sg, f):
    """all particles at the origin (no predict): a step opens landmarks at (10, 0) and (10, 3); the next step observes the first one
    1.2 m farther in range (the gates call that new: radial NIS ~ 72) together with the second"""
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, n_effective=192, rng_mode=sg.RNG_PHILOX, seed=5, math_mode=sg.MATH_FAST, particle_maps=True)
    if f is not None:
        s.set_particle_excl_spacing(f)
    R = np.array([0.01, 0.0, 0.0, (np.pi / 180) ** 2], f32)
    second = [np.hypot(10.0, 3.0), np.arctan2(3.0, 10.0)]
    opt = _opt(EXCL_ON, 1, 0.0, EXHAUSTIVE)
    r1 = s.update_particle(np.array([[10.0, 0.0], second], f32), R, **opt)
    r2 = s.update_particle(np.array([[11.2, 0.0], second], f32), R, **opt)
    rho = s.particle_excl_radii() if f else None
    d = s.download()
    s.close()
    return r1, r2, rho, d


def test_a_constructed_step_that_decides(sg):
    """fixed rule: the displaced observation lies 1.2 m from a mapped landmark, inside 2 + 0.05 x 11.2 m, and is matched (opened = 0);
    f = 0.3 caps the radius at 0.3 x 3.23 m < 1.2 m and it opens (opened = 1); f = 1 caps at 3.23 m, above the fixed radius: the
    fixed rule's state bit for bit"""
    r1, fixed, _, dfix = _two_landmarks(sg, None)
    assert r1["opened"] == 2 and fixed["opened"] == 0, (r1, fixed)
    _, small, rho, _ = _two_landmarks(sg, 0.3)
    assert small["opened"] == 1, small
    assert rho[0] < 1.2 and abs(rho[0] - 0.3 * np.hypot(1.2, 3.0)) < 1e-5, rho
    _, large, rho, dl = _two_landmarks(sg, 1.0)
    assert large == fixed and abs(rho[0] - (EXCL_ON[0] + EXCL_ON[1] * 11.2)) < 1e-5, (large, rho)
    assert dl["nf"] == dfix["nf"]
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(np.asarray(dl[k]), np.asarray(dfix[k]), equal_nan=True), k


@pytest.mark.parametrize("method,math", [(2, 1), (1, 1), (2, 0)], ids=lambda v: str(v))
def test_paths_agree(sg, tmp_path_factory, method, math):
    """the 1 000-landmark map, N = 4 096, capacity 2 000, 40 iterations, f = 0.5: run_particle through the exhaustive scan, through the
    lists and the host twin through the lists give one run bit for bit; the fixed rule's run ends elsewhere"""
    c = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2" if method == 2 else "FASTSLAM1", 40)
    ex, rex = _dev(sg, c, 4096, method, math, _opt(EXCL_ON, 1, 0.02, EXHAUSTIVE), 20, 40, 2000, 0.5)
    li, rli = _dev(sg, c, 4096, method, math, _opt(EXCL_ON, 1, 0.02, LISTS), 20, 40, 2000, 0.5)
    ho, rho = _host(sg, c, 4096, method, math, _opt(EXCL_ON, 1, 0.02, LISTS), 40, 2000, 0.5)
    assert np.array_equal(rex, rli), np.argwhere(rex != rli)[:5]
    assert np.array_equal(rli, rho), np.argwhere(rli != rho)[:5]
    _same_state(ex, li, "exhaustive vs lists")
    _same_state(li, ho, "device vs host")
    if method == 2 and math == 1:
        fx, _ = _dev(sg, c, 4096, method, math, _opt(EXCL_ON, 1, 0.02, LISTS), 20, 40, 2000, 0.0)
        assert not (fx[1]["nf"] == li[1]["nf"] and np.array_equal(fx[1]["xv"], li[1]["xv"])), "the cap never changed a label"


def test_webmap_run_is_the_fixed_rules(sg):
    """example_webmap (closest landmarks 19.5 m apart, radius at most 5 m): f = 0.5 cannot bind -- the fixed rule's run bit for bit"""
    c = _course("FASTSLAM2", 150)
    a, ra = _dev(sg, c, 1000, 2, 1, _opt(EXCL_ON, 1, 0.02, LISTS), 25, 150, None, 0.0)
    b, rb = _dev(sg, c, 1000, 2, 1, _opt(EXCL_ON, 1, 0.02, LISTS), 25, 150, None, 0.5)
    assert np.array_equal(ra, rb)
    _same_state(a, b, "webmap, f = 0.5 vs fixed")


def test_dense_map_opens_landmarks(sg, tmp_path_factory):
    """config 5's map at MAX_RANGE 20, N = 4 096, 60 iterations through the lists: with f = 0.5 the rule opens more slots than the fixed
    rule does, and at least 0.8 x what the gates alone open.  (Measured on an MI355X: gates 552, fixed 357, spacing 523.  The predicted
    "twice the fixed rule's" was not reached: in 60 steps of a first pass the map is still filling from the sensor's leading edge, so
    most new landmarks have no MAPPED neighbour inside the fixed radius yet; over the whole tape the fixed rule opens 4 667 slots
    against 10 343 -- profiles/particle_excl_spacing_c5.txt)"""
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2", 60, max_range=20)
    opened = {}
    for name, excl, f in (("gates", EXCL_OFF, 0.0), ("fixed", EXCL_ON, 0.0), ("spacing", EXCL_ON, 0.5)):
        _, rep = _dev(sg, c, 4096, 2, 1, _opt(excl, 1, 0.02, LISTS), 20, 60, 6000, f)
        assert rep[:, 3].sum() == 0, (name, "slots ran out")
        opened[name] = int(rep[:, 1].sum())
    print("dense map, slots opened:", opened)
    assert opened["spacing"] > opened["fixed"] and opened["spacing"] >= 0.8 * opened["gates"], opened


def test_launches_per_iteration(sg):
    """with the factor on, an iteration makes the launches of test_gpu_particle_lists' count plus the radius kernel"""
    c = _course("FASTSLAM2", 40)
    opt = _opt(EXCL_ON, 1, 0.02, LISTS)
    s = _spaced(_ctx(sg, c, 1000, 2, 1), 0.75)
    names = ("resample", "gather", "predict", "observe", "excl_radii", "lmk_box", "assoc_geom_partial", "assoc_geom", "assoc_lists", "associate",
             "particle_book", "particle_resolve", "fs2_update", "finish", "estimate", "particle_census", "flatten", "scan")
    s.profile(True)
    s.run_particle(c["ctl"][:10], c["Q"], c["dt"], c["xt"][:10], c["max_range"], c["R"], noise=2, **opt)
    first = {n: s.kernel_time(n)[1] for n in names}
    s.run_particle(c["ctl"][10:40], c["Q"], c["dt"], c["xt"][10:40], c["max_range"], c["R"], noise=2, **opt)
    got = {n: s.kernel_time(n)[1] - first[n] for n in names}
    s.close()
    assert all(1 <= len(x) <= 16 for x in c["ctl"][10:40])
    per_iteration = {n: 30 for n in ("gather", "predict", "observe", "excl_radii", "lmk_box", "assoc_geom_partial", "assoc_geom", "assoc_lists",
                                     "associate", "particle_book", "particle_resolve", "fs2_update")}
    expect = dict(per_iteration, resample=31, finish=1, estimate=0, particle_census=0, flatten=0, scan=0)
    expect["gather"] = 31
    assert got == expect, got
    assert (sum(got.values()) - 3) / 30 <= 13


def test_slam_backend_option(tmp_path):
    """slam-backend -assoc particle -observe device -PARTICLE_ASSOC lists -PARTICLE_EXCL_SPACING 0.75 runs example_loop1 and prints its
    map; a negative factor is refused"""
    base = [EXE, "-m", os.path.join(DATA, "example_loop1.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
            "-SWITCH_SEED_RANDOM", "7", "-assoc", "particle", "-observe", "device", "-rng", "philox", "-PARTICLE_ASSOC", "lists"]
    r = subprocess.run(base + ["-PARTICLE_EXCL_SPACING", "0.75", "-maxsteps", "3000", "-log", str(tmp_path / "a.csv")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    assert any(ln.startswith("landmarks in map:") for ln in r.stdout.splitlines()), r.stdout[-800:]
    bad = subprocess.run(base + ["-PARTICLE_EXCL_SPACING", "-1", "-maxsteps", "10"], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "PARTICLE_EXCL_SPACING" in bad.stderr, bad.stderr[-400:]


def test_refusals(sg):
    """a negative or non-finite factor is refused with ERR_INVALID"""
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, rng_mode=sg.RNG_PHILOX, particle_maps=True)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(sg.SlamGpuError) as e:
            s.set_particle_excl_spacing(bad)
        assert e.value.code == ERR_INVALID
    s.close()
