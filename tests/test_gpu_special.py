"""The update launch's specialised instantiations (kernels.h: UpdateModes; kernels.hip: update_kernel_special) against the general one
(SLAMGPU_NO_SPECIAL=1, read when the context is created): the same operations on the same values, so the whole state and the
recorded history agree BIT FOR BIT -- both builds, both methods, over launches that open landmarks, stage four and eight records,
apply a resample and do not.  Log-weight and device-observe contexts have no specialised instantiation: they guard the selection."""
import numpy as np
import pytest

from conftest import sim_args

pytestmark = pytest.mark.gpu
f32 = np.float32
KEYS = ("xv", "Pv", "w", "xf", "Pf")
K_STAGE = 8  # kernels.hip: kStage


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


_tapes = {}


def tape_of(mapname, method, nobs):
    """one tape per map and method, made once, read-only"""
    from slam_amd import host
    key = (mapname, method, nobs)
    if key not in _tapes:
        _tapes[key] = host.make_tape(sim_args(mapname, "FASTSLAM2" if method == 2 else "FASTSLAM1", 100, 7), max_obs=nobs)
    return _tapes[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def run(sg, monkeypatch, general, tape, N, every=10, observe=None, **kw):
    """the tape through slamgpu_step (or slamgpu_step_observe); peek() after every `every`-th step and at the end, and the history"""
    if general:
        monkeypatch.setenv("SLAMGPU_NO_SPECIAL", "1")
    else:
        monkeypatch.delenv("SLAMGPU_NO_SPECIAL", raising=False)
    s = sg.SlamGpu(N, tape["nlm"], n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7, device_observe=observe is not None, **kw)
    monkeypatch.delenv("SLAMGPU_NO_SPECIAL", raising=False)  # (read at creation: the context keeps what it found)
    if observe is not None:
        s.set_map(observe[0])
    snaps = []
    steps = tape["steps"]
    for k, st in enumerate(steps):
        ctl = np.array(st["controls"], f32).reshape(-1, 3)
        if observe is not None:
            s.step_observe(ctl, tape["Q"], float(tape["dt"]), st["true"], observe[1], tape["R"], noise=2)
        else:
            s.step(ctl, tape["Q"], float(tape["dt"]), st["zf"], st["idf"], st["zn"], tape["R"])
        if (k + 1) % every == 0 or k + 1 == len(steps):
            snaps.append(s.peek())
    hist = s.history_fetch()
    special = s.special_launches()
    s.close()
    return snaps, hist, special, len(steps)


def assert_same(a, b):
    (sa, ha), (sb, hb) = a[:2], b[:2]
    assert len(sa) == len(sb) and len(sa) >= 2
    for k, (x, y) in enumerate(zip(sa, sb)):
        assert x["nf"] == y["nf"]
        for key in KEYS:
            assert np.array_equal(bits(x[key]), bits(y[key])), (k, key)
    for x, y in zip(ha, hb):  # estimate, Neff, resampled
        assert np.array_equal(bits(np.asarray(x)), bits(np.asarray(y)))
    assert len(ha[0]) > 0


def assert_selected(a, b, special):
    """a ran as selected, b under SLAMGPU_NO_SPECIAL: b never takes a specialised instantiation.  a takes none either where there is
    no such instantiation (FastSLAM 1, log-weights, the device's own observation); where there is (special: FastSLAM 2 through
    slamgpu_step composes its queued predicts or observes the heading, scans block-locally at these sizes) it takes one at every launch
    that carries the previous step's resampling stage: all but the first and, at most, the one after each peek()"""
    steps, peeks = a[3], len(a[0])
    print("specialised launches: %d of %d as selected, %d under SLAMGPU_NO_SPECIAL" % (a[2], steps, b[2]))
    assert b[2] == 0
    if special:
        assert steps - 1 - peeks <= a[2] <= steps, (a[2], steps, peeks)
    else:
        assert a[2] == 0, a[2]


def assert_tape_covers(tape, hist):
    """what the run must contain to mean anything: launches that open landmarks, that stage kStage / 2 and kStage records, that apply
    a resample and that do not (the resample decided in step k is applied by the launch of step k + 1)"""
    ms = [np.asarray(st["zf"]).reshape(-1, 2).shape[0] for st in tape["steps"]]
    ns = [np.asarray(st["zn"]).reshape(-1, 2).shape[0] for st in tape["steps"]]
    assert any(n > 0 for n in ns)
    assert any(0 < m <= K_STAGE // 2 for m in ms) and any(m > K_STAGE // 2 for m in ms), ms
    res = np.asarray(hist[2])[:-1]
    assert res.any() and not res.all(), res


@pytest.mark.parametrize("method", [1, 2], ids=["fs1", "fs2"])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_webmap_special_equals_general(sg, monkeypatch, math_mode, method):
    """example_webmap, 1 024 particles (four tiles: more than one source block per ancestor window), the first 60 observation steps"""
    tape = tape_of("example_webmap", method, 60)
    assert np.asarray(tape["steps"][0]["zn"]).reshape(-1, 2).shape[0] == 6
    a = run(sg, monkeypatch, False, tape, 1024, method=method, math_mode=math_mode)
    b = run(sg, monkeypatch, True, tape, 1024, method=method, math_mode=math_mode)
    assert_tape_covers(tape, a[1])
    assert_same(a, b)
    assert_selected(a, b, method == 2)


@pytest.mark.parametrize("method", [1, 2], ids=["fs1", "fs2"])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_loop902_heading_special_equals_general(sg, monkeypatch, math_mode, method):
    """example_loop902: the heading is observed at every predict (PredictArgs::use_heading); 512 particles, 40 observation steps"""
    tape = tape_of("example_loop902", method, 40)
    conf = tape["conf"]
    assert bool(conf.SWITCH_HEADING_KNOWN)
    kw = dict(method=method, math_mode=math_mode, use_heading=True, wheel_base=float(conf.WHEELBASE), sigma_phi=float(conf.sigmaT))
    a = run(sg, monkeypatch, False, tape, 512, **kw)
    b = run(sg, monkeypatch, True, tape, 512, **kw)
    assert_same(a, b)
    assert_selected(a, b, method == 2)


def test_log_weight_context_takes_the_general_instantiation(sg, monkeypatch):
    tape = tape_of("example_webmap", 2, 60)
    a = run(sg, monkeypatch, False, tape, 1024, method=2, math_mode=1, log_weights=True)
    b = run(sg, monkeypatch, True, tape, 1024, method=2, math_mode=1, log_weights=True)
    assert_same(a, b)
    assert_selected(a, b, False)


def test_device_observe_context_takes_the_general_instantiation(sg, monkeypatch):
    from slam_amd import host
    tape = tape_of("example_webmap", 2, 60)
    sim = host.HostSim(sim_args("example_webmap", "FASTSLAM2", 100, 7))
    lm, _ = sim.map()
    obs = (lm, float(sim.conf.MAX_RANGE))
    sim.close()
    a = run(sg, monkeypatch, False, tape, 1024, method=2, math_mode=1, observe=obs)
    b = run(sg, monkeypatch, True, tape, 1024, method=2, math_mode=1, observe=obs)
    assert_same(a, b)
    assert_selected(a, b, False)
