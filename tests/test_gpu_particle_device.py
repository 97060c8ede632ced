"""The per-particle association driven by the device (slamgpu_run_particle / slamgpu_particle_report_fetch): K iterations of the
wrapper's loop per call -- predicts, the observation made on the device, the per-particle update, the estimate -- with every
decision of slamgpu_update_particle's host block (census, dead slots, new slots, genealogy) taken on the device.  Held bit for bit
to its host-driven twin: slamgpu_predict + slamgpu_observe + slamgpu_update_particle + slamgpu_estimate_async on a context created
the same way."""
import os
import subprocess

import numpy as np
import pytest

from conftest import sim_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
ERR_INVALID, ERR_CAPACITY = -1, -3

pytestmark = pytest.mark.gpu
f32 = np.float32
EXCL_ON = (2.0, 0.05, 2.0)   # slam-backend's -PARTICLE_EXCL_BASE / _PER_M / _UNIQUE_RATIO
EXCL_OFF = (0.0, 0.0, 2.0)
REPORT = ("rewritten", "opened", "reused", "dropped", "slots", "dead", "need", "census")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


_TAPES = {}


def _course(method, steps, mapname="example_webmap"):
    """controls / true poses of `steps` observation steps of a map, the map and the sensor's range"""
    key = (method, steps, mapname)
    if key not in _TAPES:
        from slam_amd import host
        args = sim_args(mapname, method, 100, 7)
        tape = host.make_tape(args, max_obs=steps)
        sim = host.HostSim(args)
        lm, _ = sim.map()
        max_range = float(sim.conf.MAX_RANGE)
        sim.close()
        ctl = [np.array(st["controls"], f32).reshape(-1, 3) for st in tape["steps"]]
        xt = [np.asarray(st["true"], f32) for st in tape["steps"]]
        _TAPES[key] = dict(ctl=ctl, xt=xt, lm=lm, max_range=max_range, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]), nlm=tape["nlm"])
    return _TAPES[key]


def _ctx(sg, c, N, method, math, cap=None, logw=False, n_effective=None):
    s = sg.SlamGpu(N, cap or c["nlm"] * 4, method=method, n_effective=int(0.75 * N) if n_effective is None else n_effective, rng_mode=sg.RNG_PHILOX,
                   seed=5, math_mode=math,
                   device_observe=True, particle_maps=True, log_weights=logw)
    s.set_map(c["lm"])
    return s


def _host_step(s, c, k, opt, xt=None):
    for V, G, phi in c["ctl"][k]:
        s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
    o = s.observe(c["xt"][k] if xt is None else xt, c["max_range"], c["R"], noise=2)
    rep = np.zeros(8, np.int32)
    if len(o["z"]):
        r = s.update_particle(o["z"], c["R"], **opt)
        rep = np.array([r[f] for f in REPORT], np.int32)
    s.estimate_async()
    return rep


def _finish(s):
    hist = s.history_fetch()
    d = s.download()
    s.close()
    return hist, d


def _same_state(a, b, what):
    (ha, da), (hb, db) = a, b
    for x, y in zip(ha, hb):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), what
    assert da["nf"] == db["nf"], (what, da["nf"], db["nf"])
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        x, y = np.asarray(da[k]), np.asarray(db[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, k)


def _opt(excl, census_every, new_share, mode=0):
    return dict(gate_reject=4.0, gate_augment=25.0, mode=mode, new_share=new_share, p_new=0.05, census_every=census_every, excl=excl)


def _pair(sg, N, steps, method, math, opt, K, cap=None, xt_override=None, fetch_between=False):
    """(host twin, device run in calls of K iterations): states and reports.  fetch_between: the device run's history and reports are
    fetched after every call (the host takes the state back and runs the outstanding stage, the next call hands it over again)"""
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", steps)
    xts = list(c["xt"])
    if xt_override:
        for k, x in xt_override.items():
            xts[k] = x
    h = _ctx(sg, c, N, method, math, cap)
    hrep = np.array([_host_step(h, c, k, opt, xts[k]) for k in range(steps)])
    host = _finish(h)
    d = _ctx(sg, c, N, method, math, cap)
    hists, reps = [], []
    for a in range(0, steps, K):
        b = min(steps, a + K)
        d.run_particle(c["ctl"][a:b], c["Q"], c["dt"], xts[a:b], c["max_range"], c["R"], noise=2, **opt)
        if fetch_between:
            reps.append(d.particle_report_fetch())
            hists.append(d.history_fetch())
    reps.append(d.particle_report_fetch())
    hist, dl = _finish(d)
    hists.append(hist)
    dev = (tuple(np.concatenate([np.asarray(h[q]) for h in hists]) for q in range(len(hist))), dl)
    return host, hrep, dev, np.concatenate(reps)


@pytest.mark.parametrize("method,excl,census_every,new_share,math", [
    (2, EXCL_OFF, 1, 0.0, 1), (1, EXCL_OFF, 3, 0.02, 1), (2, EXCL_ON, 3, 0.02, 1), (1, EXCL_ON, 1, 0.0, 1),
    (2, EXCL_ON, 1, 0.02, 1), (1, EXCL_OFF, 1, 0.02, 1), (2, EXCL_OFF, 3, 0.0, 1), (1, EXCL_ON, 3, 0.02, 1),
    (2, EXCL_OFF, 1, 0.02, 0)], ids=lambda v: str(v))
def test_device_driven_equals_host_twin(sg, method, excl, census_every, new_share, math):
    """N = 1 000, 150 observation steps of example_webmap in calls of 25: histories (estimate, Neff, decision), every report and the
    final state (NaN = absent) bit for bit; both methods, exclusion rule on / off, census every step / every third, new_share 0 /
    0.02, fast build and one strict-build case."""
    host, hrep, dev, drep = _pair(sg, 1000, 150, method, math, _opt(excl, census_every, new_share), 25)
    assert np.array_equal(hrep, drep), np.argwhere(hrep != drep)[:5]
    _same_state(host, dev, "end of run")
    assert host[1]["nf"] >= 6 and np.asarray(host[0][2]).any(), "the run never opened landmarks / never resampled"


@pytest.mark.parametrize("method,excl,new_share", [(2, EXCL_ON, 0.02), (1, EXCL_OFF, 0.0)])
def test_history_fetch_between_calls(sg, method, excl, new_share):
    """history and reports fetched after every call of 25 (a fetch hands the state back: the host runs the last update's resampling stage
    and leaves its gather pending; the next call takes both over): still the twin's run bit for bit"""
    host, hrep, dev, drep = _pair(sg, 1000, 150, method, 1, _opt(excl, 1, new_share), 25, fetch_between=True)
    assert np.array_equal(hrep, drep), np.argwhere(hrep != drep)[:5]
    _same_state(host, dev, "end of run")


def test_device_driven_equals_host_twin_large(sg):
    """10^5 particles, 20 steps"""
    host, hrep, dev, drep = _pair(sg, 100000, 20, 2, 1, _opt(EXCL_ON, 1, 0.02), 10)
    assert np.array_equal(hrep, drep)
    _same_state(host, dev, "end of run")


def test_slot_pressure_reuses_and_drops(sg):
    """a slot capacity far below what the run opens (8 slots; every observation one particle calls new opens one): dead slots
    are reused and observations dropped, as the host decides"""
    host, hrep, dev, drep = _pair(sg, 1000, 150, 2, 1, _opt(EXCL_OFF, 1, 0.0), 30, cap=8)
    assert np.array_equal(hrep, drep), np.argwhere(hrep != drep)[:5]
    _same_state(host, dev, "end of run")
    assert hrep[:, 3].sum() > 0, "no slot pressure: nothing dropped"


def test_iteration_with_nothing_visible(sg):
    """an iteration from a pose a kilometre away sees nothing: no update (report all zeros, steps do not advance), and the later
    iterations stay those of the twin"""
    far = np.array([1000.0, 1000.0, 0.0], f32)
    host, hrep, dev, drep = _pair(sg, 1000, 60, 2, 1, _opt(EXCL_ON, 1, 0.02), 20, xt_override={30: far})
    assert not hrep[30].any() and not drep[30].any()
    assert np.array_equal(hrep, drep)
    _same_state(host, dev, "end of run")


def test_mixed_driving_equals_all_host(sg):
    """device calls, host steps, device calls: the all-host twin's run; num_landmarks / download read mid-run agree with it"""
    N, steps, opt = 1000, 90, _opt(EXCL_ON, 3, 0.02)
    c = _course("FASTSLAM2", steps)
    h = _ctx(sg, c, N, 2, 1)
    d = _ctx(sg, c, N, 2, 1)
    hrep, drep = [], []
    for k in range(steps):
        hrep.append(_host_step(h, c, k, opt))
        if 30 <= k < 60:
            drep.append(_host_step(d, c, k, opt))
        elif k in (29, 89):
            lo = 0 if k == 29 else 60
            d.run_particle(c["ctl"][lo:k + 1], c["Q"], c["dt"], c["xt"][lo:k + 1], c["max_range"], c["R"], noise=2, **opt)
            drep.extend(d.particle_report_fetch())
            assert d.nf() == h.nf()
            a, b = h.download(), d.download()
            for f in ("xv", "w", "xf"):
                assert np.array_equal(np.asarray(a[f]), np.asarray(b[f]), equal_nan=True), (k, f)
    assert np.array_equal(np.array(hrep), np.array(drep))
    _same_state(_finish(h), _finish(d), "end of run")


def test_host_step_fetch_then_device(sg):
    """host steps, a history fetch (the last host update's stage runs, its gather stays pending), then device calls: the all-host twin"""
    N, steps, opt = 1000, 80, _opt(EXCL_ON, 1, 0.02)
    c = _course("FASTSLAM2", steps)
    h = _ctx(sg, c, N, 2, 1)
    d = _ctx(sg, c, N, 2, 1)
    hrep = [_host_step(h, c, k, opt) for k in range(steps)]
    drep = [_host_step(d, c, k, opt) for k in range(20)]
    hists = [d.history_fetch()]
    for lo, hi in ((20, 50), (50, 80)):
        d.run_particle(c["ctl"][lo:hi], c["Q"], c["dt"], c["xt"][lo:hi], c["max_range"], c["R"], noise=2, **opt)
        drep.extend(d.particle_report_fetch())
        hists.append(d.history_fetch())
    assert np.array_equal(np.array(hrep), np.array(drep))
    (hh, dh), (hd, dd) = _finish(h), _finish(d)
    hd = tuple(np.concatenate([np.asarray(x[q]) for x in hists + [hd]]) for q in range(len(hd)))
    _same_state((hh, dh), (hd, dd), "end of run")


def _partial_slots(d):
    """slots some particles hold and others do not (what the holders census counts)"""
    xf = np.asarray(d["xf"]).reshape(len(d["w"]), -1, 2)[:, :, 0]
    held = ~np.isnan(xf)
    return int((held.any(axis=0) & ~held.all(axis=0)).sum())


def test_census_cap_after_hand_back(sg):
    """a map of 117 landmarks (a census table of 234 words for the device-driven path) and more than 64 partial slots: the holders census
    counts the first pp_nz_cap of them (max(64, 2 x the most observations of a step), pp_reserve's rule) in the twin, in the device
    calls and in host steps after a hand-back alike"""
    N, steps, opt = 1000, 320, _opt(EXCL_OFF, 1, 0.0)
    c = _course("FASTSLAM2", steps, "example_loop902")
    cap = 6 * c["nlm"]
    # (no resampling: the particles that opened a slot and those that did not both live on, and the partial slots pile up)
    h = _ctx(sg, c, N, 2, 1, cap, n_effective=0)
    d = _ctx(sg, c, N, 2, 1, cap, n_effective=0)
    hrep = [_host_step(h, c, k, opt) for k in range(steps)]
    drep, hists = [], []
    for lo, hi, dev in ((0, 120, True), (120, 200, False), (200, 320, True)):
        if dev:
            d.run_particle(c["ctl"][lo:hi], c["Q"], c["dt"], c["xt"][lo:hi], c["max_range"], c["R"], noise=2, **opt)
            drep.extend(d.particle_report_fetch())
        else:
            drep.extend(_host_step(d, c, k, opt) for k in range(lo, hi))
        hists.append(d.history_fetch())
    hrep, drep = np.array(hrep), np.array(drep)
    assert np.array_equal(hrep, drep), np.argwhere(hrep != drep)[:5]
    (hh, dh), (hd, dd) = _finish(h), _finish(d)
    hd = tuple(np.concatenate([np.asarray(x[q]) for x in hists + [hd]]) for q in range(len(hd)))
    _same_state((hh, dh), (hd, dd), "end of run")
    assert _partial_slots(dh) > 64, _partial_slots(dh)   # (the census had more than its cap to count)


def test_split_of_the_calls(sg):
    """one call of K = 40 = 40 calls of K = 1 = 8 calls of K = 5"""
    c = _course("FASTSLAM2", 40)
    opt = _opt(EXCL_ON, 1, 0.02)
    out = []
    for K in (40, 1, 5):
        s = _ctx(sg, c, 1000, 2, 1)
        for a in range(0, 40, K):
            s.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], c["xt"][a:a + K], c["max_range"], c["R"], noise=2, **opt)
        rep = s.particle_report_fetch()
        out.append((_finish(s), rep))
    for (st, rep) in out[1:]:
        assert np.array_equal(rep, out[0][1])
        _same_state(out[0][0], st, "split")


def test_refusals_apply_nothing(sg):
    c = _course("FASTSLAM2", 10)
    opt = _opt(EXCL_OFF, 1, 0.0)
    run = lambda s, K=3, noise=2, **kw: s.run_particle(c["ctl"][:K], c["Q"], c["dt"], c["xt"][:K], c["max_range"], c["R"], noise=noise,
                                                       **dict(opt, **kw))

    def refused(code, fn, *a, **kw):
        with pytest.raises(sg.SlamGpuError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
    # contexts that cannot take it
    for kw in (dict(particle_maps=True), dict(device_observe=True)):
        s = sg.SlamGpu(500, 140, rng_mode=sg.RNG_PHILOX, **kw)
        s.set_map(c["lm"])
        refused(ERR_INVALID, run, s)
        s.close()
    s = sg.SlamGpu(500, 140, rng_mode=sg.RNG_PHILOX, device_observe=True, particle_maps=True)
    refused(ERR_INVALID, run, s)   # no map
    s.close()
    s = sg.SlamGpu(500, 140, rng_mode=sg.RNG_TAPE, device_observe=True, particle_maps=True)
    s.set_map(c["lm"])
    refused(ERR_INVALID, run, s)
    s.close()
    s = _ctx(sg, c, 500, 2, 1)
    run(s, K=2)
    before = (s.download(), s.nf())
    bad = [dict(noise=1), dict(mode=2), dict(p_new=0.0), dict(new_share=1.5), dict(census_every=-1)]
    for kw in bad:
        refused(ERR_INVALID, run, s, **kw)
    # more than the history holds
    refused(ERR_CAPACITY, s.run_particle, [np.zeros((0, 3), f32)] * 4095, c["Q"], c["dt"], [c["xt"][0]] * 4095, c["max_range"], c["R"], noise=2, **opt)
    after = (s.download(), s.nf())
    assert before[1] == after[1]
    for f in ("xv", "w", "xf"):
        assert np.array_equal(np.asarray(before[0][f]), np.asarray(after[0][f]), equal_nan=True)
    assert len(s.particle_report_fetch()) == 2 and len(s.history_fetch()[0]) == 2
    s.close()
    # N x capacity x map above the exhaustive scan's limit
    s = sg.SlamGpu(10000, 2500, rng_mode=sg.RNG_PHILOX, device_observe=True, particle_maps=True)
    s.set_map(np.tile(c["lm"], (1, 2000 // c["lm"].shape[1] + 1))[:, :2000])
    refused(ERR_CAPACITY, run, s)
    s.close()
    # more than the report ring holds (the history has room: it was fetched, the reports were not)
    s = _ctx(sg, c, 500, 2, 1)
    far = [np.array([1000.0, 1000.0, 0.0], f32)] * 4090
    s.run_particle([np.zeros((0, 3), f32)] * 4090, c["Q"], c["dt"], far, c["max_range"], c["R"], noise=2, **opt)
    assert len(s.history_fetch()[0]) == 4090
    refused(ERR_CAPACITY, run, s, K=7)
    assert len(s.particle_report_fetch()) == 4090
    run(s, K=7)
    assert len(s.particle_report_fetch()) == 7
    s.close()


def test_launches_per_iteration(sg):
    """steady state: 8 kernel launches per iteration (slamgpu_kernel_time's counts): the previous update's resampling stage, the
    gather (+ its estimate), the fused predicts, the observation, the association (+ census), the bookkeeping, resolve, the update.
    (Reading the counts hands the state back to the host, which runs the last iteration's outstanding stage itself: one resample
    and one finish per read; the next call runs the gather that leaves pending.)"""
    c = _course("FASTSLAM2", 40)
    opt = _opt(EXCL_ON, 1, 0.02)
    s = _ctx(sg, c, 1000, 2, 1)
    names = ("resample", "gather", "predict", "observe", "associate", "particle_book", "particle_resolve", "fs2_update", "finish", "estimate",
             "particle_census", "flatten", "scan")
    s.profile(True)
    s.run_particle(c["ctl"][:10], c["Q"], c["dt"], c["xt"][:10], c["max_range"], c["R"], noise=2, **opt)
    first = {n: s.kernel_time(n)[1] for n in names}
    s.run_particle(c["ctl"][10:40], c["Q"], c["dt"], c["xt"][10:40], c["max_range"], c["R"], noise=2, **opt)
    got = {n: s.kernel_time(n)[1] - first[n] for n in names}
    s.close()
    assert all(1 <= len(x) <= 16 for x in c["ctl"][10:40])   # (one fused predict launch per iteration)
    per_iteration = {n: 30 for n in ("gather", "predict", "observe", "associate", "particle_book", "particle_resolve", "fs2_update")}
    # (+ the hand-back of the first read and the hand-over of the second call: the host's resample + finish, and the gather it left
    # pending, which the hand-over runs)
    expect = dict(per_iteration, resample=31, finish=1, estimate=0, particle_census=0, flatten=0, scan=0)
    expect["gather"] = 31
    assert got == expect, got
    assert (sum(got.values()) - 3) / 30 <= 8


def test_slam_backend_particle_device(tmp_path):
    """slam-backend -assoc particle -observe device: the batched loop (256 iterations per slamgpu_run_particle) and -loop step (one per
    call) print the same final estimate and the same map; -observe device with -rng parity is still refused"""
    outs = []
    for extra in ((), ("-loop", "step")):
        log = str(tmp_path / ("run%d.csv" % len(outs)))
        r = subprocess.run([EXE, "-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
                            "-SWITCH_SEED_RANDOM", "7", "-assoc", "particle", "-observe", "device", "-rng", "philox", "-maxsteps", "3000", "-log", log, *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        assert "slamgpu_run_particle" in r.stdout
        lines = r.stdout.splitlines()
        final = [ln for ln in lines if "final estimate" in ln][0]
        mapline = [ln for ln in lines if ln.startswith("landmarks in map:")][0]
        outs.append((final[final.index("final estimate"):], mapline, np.loadtxt(log, delimiter=",", skiprows=1)))
    (fa, ma, la), (fb, mb, lb) = outs
    assert fa == fb and ma == mb, (fa, fb, ma, mb)
    assert la.shape[0] > 100 and np.array_equal(la[:, :7], lb[:, :7])
    held = int(ma.split()[3])
    assert held >= 6, ma
    r = subprocess.run([EXE, "-m", os.path.join(ROOT, "data", "example_webmap.mat"), "-method", "FASTSLAM2", "-assoc", "particle", "-observe", "device",
                        "-rng", "parity"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-observe device needs" in r.stderr
