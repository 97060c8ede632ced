"""SLAMGPU_ASSOC_LISTS: the per-particle association through candidate lists built on the device from the slots' boxes, with the
exclusion rule folded into the lists.  Its labels are the exhaustive scan's, decision for decision, so every run here is held bit for
bit to a run that already has a reference: slamgpu_run_particle with the exhaustive scan, the host-driven twin slamgpu_update_particle
with the lists, or (beyond the exhaustive scan's limit) slamgpu_update_particle through the grid, whose labels are pinned to the scan."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_gpu_particle_device import (EXCL_OFF, EXCL_ON, EXE, ERR_CAPACITY, ERR_INVALID, REPORT, _course, _ctx, _finish, _host_step, _opt,
                                      _pair, _same_state)

pytestmark = pytest.mark.gpu
f32 = np.float32
LISTS, EXHAUSTIVE, GRID = 3, 1, 2


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


_MAPS = {}


def _synthetic(tmp_path_factory, n):
    """a map of n landmarks i.i.d. uniform over the webmap's bounding box (config 5's recipe), the webmap's waypoints and .ini"""
    if n not in _MAPS:
        from slam_amd import host
        from conftest import sim_args
        d = tmp_path_factory.mktemp("lists%d" % n)
        lm = host.synthetic_landmarks(12345 + n, n, -130, 100, -100, 90)
        h = host.HostSim(sim_args("example_webmap", "FASTSLAM2", 100, 7))
        _, wp = h.map()
        h.close()
        mp = str(d / ("synthetic%d.mat" % n))
        host.write_map(mp, lm, wp)
        open(str(d / ("synthetic%d.ini" % n)), "w").write(open(os.path.join(DATA, "example_webmap.ini")).read())
        _MAPS[n] = mp
    return _MAPS[n]


def _course_of(mp, method, steps, max_range=None):
    """_course for a map file (MAX_RANGE: the .ini's unless given)"""
    from slam_amd import host
    args = ["-m", mp, "-method", method, "-NPARTICLES", 100, "-NEFFECTIVE", 75, "-SWITCH_SEED_RANDOM", 7]
    if max_range is not None:
        args += ["-MAX_RANGE", max_range]
    tape = host.make_tape(args, max_obs=steps)
    sim = host.HostSim(args)
    lm, _ = sim.map()
    mr = float(sim.conf.MAX_RANGE)
    sim.close()
    ctl = [np.array(st["controls"], f32).reshape(-1, 3) for st in tape["steps"]]
    xt = [np.asarray(st["true"], f32) for st in tape["steps"]]
    return dict(ctl=ctl, xt=xt, lm=lm, max_range=mr, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]), nlm=tape["nlm"])


def _visible(c, k):
    """observations of step k (observe_kernel's visibility test, in numpy)"""
    lm = np.asarray(c["lm"], f32).reshape(2, -1)
    x, y, ph = (float(v) for v in c["xt"][k])
    dx, dy, r = lm[0] - f32(x), lm[1] - f32(y), c["max_range"]
    return int(np.sum((np.abs(dx) < r) & (np.abs(dy) < r) & (dx * np.cos(ph) + dy * np.sin(ph) > 0) & (dx.astype(float) ** 2 + dy.astype(float) ** 2 < r * r)))


def _device_run(sg, c, N, method, math, opt, K, steps, cap=None):
    """run_particle in calls of K: (history, download), reports, list counters"""
    d = _ctx(sg, c, N, method, math, cap)
    reps = []
    for a in range(0, steps, K):
        b = min(steps, a + K)
        d.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **opt)
    reps.append(d.particle_report_fetch())
    stats = d.particle_list_stats()
    return _finish(d), np.concatenate(reps), stats


def _host_run(sg, c, N, method, math, opt, steps, cap=None):
    h = _ctx(sg, c, N, method, math, cap)
    rep = np.array([_host_step(h, c, k, opt) for k in range(steps)])
    stats = h.particle_list_stats()
    return _finish(h), rep, stats


@pytest.mark.parametrize("method,excl,math", [(2, EXCL_OFF, 1), (2, EXCL_ON, 1), (1, EXCL_ON, 1), (1, EXCL_OFF, 1), (2, EXCL_ON, 0)],
                         ids=lambda v: str(v))
def test_lists_equal_the_exhaustive_scan_on_the_device(sg, method, excl, math):
    """example_webmap, N = 1 000, 150 iterations in calls of 25: run_particle through the lists equals run_particle through the exhaustive
    scan bit for bit -- histories, every report, the final state (NaN = absent); both methods, the rule on and off, one strict build"""
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 150)
    ex, rex, _ = _device_run(sg, c, 1000, method, math, _opt(excl, 1, 0.02, EXHAUSTIVE), 25, 150)
    li, rli, st = _device_run(sg, c, 1000, method, math, _opt(excl, 1, 0.02, LISTS), 25, 150)
    assert np.array_equal(rex, rli), np.argwhere(rex != rli)[:5]
    _same_state(ex, li, "lists vs exhaustive")
    assert st["steps"] > 100 and st["entries"] > 0 and st["overflowed"] == 0, st
    assert ex[1]["nf"] >= 6 and np.asarray(ex[0][2]).any(), "the run never opened landmarks / never resampled"


@pytest.mark.parametrize("method,excl,fetch_between", [(2, EXCL_ON, False), (1, EXCL_OFF, False), (2, EXCL_ON, True)], ids=lambda v: str(v))
def test_device_lists_equal_the_host_twin(sg, method, excl, fetch_between):
    """update_particle(LISTS) step by step equals run_particle(LISTS) bit for bit (the test_gpu_particle_device pattern, one case fetching
    history and reports between calls: the state goes back to the host and the boxes are refreshed at the next hand-over)"""
    host, hrep, dev, drep = _pair(sg, 1000, 150, method, 1, _opt(excl, 1, 0.02, LISTS), 25, fetch_between=fetch_between)
    assert np.array_equal(hrep, drep), np.argwhere(hrep != drep)[:5]
    _same_state(host, dev, "end of run")


def test_exclusion_rule_on_a_denser_map(sg, tmp_path_factory):
    """1 000 landmarks over the webmap's box, N = 4 096, capacity 2 000 (the exhaustive scan still allowed), 40 iterations with the rule
    on: lists equal the scan bit for bit; the lists pruned (entries per observation far below the slots in use); the rule acted (the run
    with it off ends elsewhere)"""
    c = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 40)
    steps = 40
    ex, rex, _ = _device_run(sg, c, 4096, 2, 1, _opt(EXCL_ON, 1, 0.02, EXHAUSTIVE), 20, steps, cap=2000)
    li, rli, st = _device_run(sg, c, 4096, 2, 1, _opt(EXCL_ON, 1, 0.02, LISTS), 20, steps, cap=2000)
    assert np.array_equal(rex, rli), np.argwhere(rex != rli)[:5]
    _same_state(ex, li, "lists vs exhaustive, rule on")
    nobs = sum(_visible(c, k) for k in range(steps))
    nf = li[1]["nf"]
    assert nobs > 20 * steps and nf > 100, (nobs, nf)
    assert st["steps"] == sum(1 for k in range(steps) if _visible(c, k) > 0) and st["overflowed"] == 0, st
    per_obs = st["entries"] / nobs
    assert 1.0 < per_obs < 0.05 * nf, (per_obs, nf)
    off, _, _ = _device_run(sg, c, 4096, 2, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 20, steps, cap=2000)
    assert not (off[1]["nf"] == nf and np.array_equal(off[1]["xv"], li[1]["xv"])), "the exclusion rule never changed a label"


def test_forced_overflow_walks_every_slot(sg, monkeypatch, tmp_path_factory):
    """SLAMGPU_ASSOC_LCAP=1 on the 1 000-landmark map: lists too short for many observations, which are walked over every slot instead
    -- the same states, on the device and on the host twin; the counters say which route answered"""
    c = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 30)
    opt = _opt(EXCL_ON, 1, 0.02, LISTS)
    ref, rref, st0 = _device_run(sg, c, 1000, 2, 1, opt, 10, 30, cap=2000)
    assert st0["overflowed"] == 0 and st0["steps"] > 0, st0
    monkeypatch.setenv("SLAMGPU_ASSOC_LCAP", "1")
    got, rgot, st1 = _device_run(sg, c, 1000, 2, 1, opt, 10, 30, cap=2000)
    assert np.array_equal(rref, rgot)
    _same_state(ref, got, "LCAP=1")
    assert st1["overflowed"] > 0, st1
    host, rhost, st2 = _host_run(sg, c, 1000, 2, 1, opt, 30, cap=2000)
    assert np.array_equal(rref, rhost)
    _same_state(ref, host, "LCAP=1, host twin")
    assert st2["overflowed"] > 0, st2


def test_beyond_the_exhaustive_limit(sg, tmp_path_factory):
    """10 000 particles, a 2 000-landmark map, capacity 2 500: the exhaustive scan is refused (5e10 gate evaluations a step); the lists
    run, and with the rule off equal the host-driven update_particle through the grid bit for bit over 20 iterations"""
    c = _course_of(_synthetic(tmp_path_factory, 2000), "FASTSLAM2", 20)
    s = _ctx(sg, c, 10000, 2, 1, 2500)
    with pytest.raises(sg.SlamGpuError) as e:
        s.run_particle(c["ctl"][:1], c["Q"], c["dt"], c["xt"][:1], c["max_range"], c["R"], noise=2, **_opt(EXCL_OFF, 1, 0.02, EXHAUSTIVE))
    assert e.value.code == ERR_CAPACITY
    s.close()
    li, rli, st = _device_run(sg, c, 10000, 2, 1, _opt(EXCL_OFF, 1, 0.02, LISTS), 10, 20, cap=2500)
    gr, rgr, _ = _host_run(sg, c, 10000, 2, 1, _opt(EXCL_OFF, 1, 0.02, GRID), 20, cap=2500)
    assert np.array_equal(rli, rgr), np.argwhere(rli != rgr)[:5]
    _same_state(gr, li, "lists vs host grid")
    assert st["steps"] == 20 and li[1]["nf"] > 100, (st, li[1]["nf"])


def test_config5_scale(sg, tmp_path_factory):
    """10^5 particles on the 10^4-landmark map at its MAX_RANGE (~1.3 k observations a step), a few iterations: the device run equals
    its host twin (both LISTS), and the reports are sane"""
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2", 4)
    opt = _opt(EXCL_OFF, 1, 0.02, LISTS)
    dev, rdev, st = _device_run(sg, c, 100000, 2, 1, opt, 4, 4, cap=3000)
    host, rhost, _ = _host_run(sg, c, 100000, 2, 1, opt, 4, cap=3000)
    assert np.array_equal(rdev, rhost), np.argwhere(rdev != rhost)[:5]
    _same_state(host, dev, "config 5")
    rep = dict(zip(REPORT, rdev[-1]))
    nobs = [_visible(c, k) for k in range(4)]
    assert min(nobs) > 500 and st["steps"] == 4 and st["overflowed"] == 0, (nobs, st)
    assert 0 < rep["slots"] <= 3000 and all(r[0] + r[1] <= 3000 for r in rdev), rdev
    assert np.all(np.isfinite(np.asarray(dev[0][0])))


def test_refusals_apply_nothing(sg, tmp_path_factory):
    """an iteration whose observations may exceed 4 096 is refused with ERR_CAPACITY; mode 3 on slamgpu_associate_ex is ERR_INVALID;
    both leave the state, the reports and the history as they were"""
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2", 3, max_range=400)
    assert _visible(c, 1) > 4096
    small = _course("FASTSLAM2", 3)
    s = _ctx(sg, c, 256, 2, 1, 10000)
    opt = _opt(EXCL_OFF, 1, 0.02, LISTS)
    xt_near = [small["xt"][0], c["xt"][1]]  # (the first iteration sees the webmap's few, the second the whole map)
    before = s.download()
    with pytest.raises(sg.SlamGpuError) as e:
        s.run_particle(c["ctl"][:2], c["Q"], c["dt"], xt_near, c["max_range"], c["R"], noise=2, **opt)
    assert e.value.code == ERR_CAPACITY
    with pytest.raises(sg.SlamGpuError) as e:
        s.associate(np.array([[5.0, 0.1]], f32), c["R"], mode=LISTS)
    assert e.value.code == ERR_INVALID
    assert len(s.particle_report_fetch()) == 0 and len(s.history_fetch()[0]) == 0
    after = s.download()
    assert before["nf"] == after["nf"]
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), k
    s.close()


def test_launches_per_iteration(sg):
    """steady state: every per-iteration kernel once per iteration, at most 12 launches per iteration (the exhaustive path's 8 with the
    association launch replaced by the box refresh, the two geometry launches, the lists and the walk)"""
    c = _course("FASTSLAM2", 40)
    opt = _opt(EXCL_ON, 1, 0.02, LISTS)
    s = _ctx(sg, c, 1000, 2, 1)
    names = ("resample", "gather", "predict", "observe", "lmk_box", "assoc_geom_partial", "assoc_geom", "assoc_lists", "associate", "particle_book",
             "particle_resolve", "fs2_update", "finish", "estimate", "particle_census", "flatten", "scan")
    s.profile(True)
    s.run_particle(c["ctl"][:10], c["Q"], c["dt"], c["xt"][:10], c["max_range"], c["R"], noise=2, **opt)
    first = {n: s.kernel_time(n)[1] for n in names}
    s.run_particle(c["ctl"][10:40], c["Q"], c["dt"], c["xt"][10:40], c["max_range"], c["R"], noise=2, **opt)
    got = {n: s.kernel_time(n)[1] - first[n] for n in names}
    s.close()
    assert all(1 <= len(x) <= 16 for x in c["ctl"][10:40])
    per_iteration = {n: 30 for n in ("gather", "predict", "observe", "lmk_box", "assoc_geom_partial", "assoc_geom", "assoc_lists", "associate",
                                     "particle_book", "particle_resolve", "fs2_update")}
    expect = dict(per_iteration, resample=31, finish=1, estimate=0, particle_census=0, flatten=0, scan=0)
    expect["gather"] = 31
    assert got == expect, got
    assert (sum(got.values()) - 3) / 30 <= 12


def _cli(mp, extra, tmp_path, tag, maxsteps):
    log = str(tmp_path / ("%s.csv" % tag))
    r = subprocess.run([EXE, "-m", mp, "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384", "-SWITCH_SEED_RANDOM", "7", "-assoc",
                        "particle", "-observe", "device", "-rng", "philox", "-maxsteps", str(maxsteps), "-log", log, *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    lines = r.stdout.splitlines()
    final = [ln for ln in lines if "final estimate" in ln][0]
    mapline = [ln for ln in lines if ln.startswith("landmarks in map:")][0]
    return final[final.index("final estimate"):], mapline, np.loadtxt(log, delimiter=",", skiprows=1)


def test_slam_backend_particle_lists(tmp_path, tmp_path_factory):
    """slam-backend -assoc particle -observe device -PARTICLE_ASSOC lists prints the run without the key (same labels: the same run);
    on a 2 000-landmark map the lists run reaches the end"""
    web = os.path.join(DATA, "example_webmap.mat")
    a = _cli(web, (), tmp_path, "auto", 3000)
    b = _cli(web, ("-PARTICLE_ASSOC", "lists"), tmp_path, "lists", 3000)
    assert a[0] == b[0] and a[1] == b[1]
    assert a[2].shape[0] > 100 and np.array_equal(a[2][:, :7], b[2][:, :7])  # (the last column is wall time)
    _cli(_synthetic(tmp_path_factory, 2000), ("-PARTICLE_ASSOC", "lists"), tmp_path, "syn", 1500)
