"""Who allocates and frees what in the observation layer (slamgpu_ctx::fe and ::ps, observe_release): contexts that set a map, made
their observations on the device or ran the persistent step loop close cleanly in every state their buffers can be in, a map set
again keeps nothing of the one before, the loop's queue grows between launches, and a later context is unaffected.  256 particles on
example_webmap, 12 observation steps (259 where the queue has to grow past its first 256 entries); every sequence here is a legal one."""
import numpy as np
import pytest

from conftest import sim_args

pytestmark = pytest.mark.gpu
f32 = np.float32
N, NOBS, GROW = 256, 12, 259
KEYS = ("xv", "Pv", "w", "xf", "Pf")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


@pytest.fixture(scope="module")
def tape():
    from slam_amd import host
    args = sim_args("example_webmap", "FASTSLAM2", N, 7)
    tp = host.make_tape(args, max_obs=GROW)
    sim = host.HostSim(args)
    tp["lm"], _ = sim.map()
    tp["mr"] = float(sim.conf.MAX_RANGE)
    sim.close()
    tp["ctl"] = [np.array(st["controls"], f32).reshape(-1, 3) for st in tp["steps"]]
    tp["xt"] = [np.asarray(st["true"], f32) for st in tp["steps"]]
    assert len(tp["steps"]) == GROW
    return tp


def context(sg, tp):
    return sg.SlamGpu(N, tp["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1, device_observe=True)


def stepped(s, tp, nobs=NOBS):
    for k in range(nobs):
        s.step_observe(tp["ctl"][k], tp["Q"], float(tp["dt"]), tp["xt"][k], tp["mr"], tp["R"], noise=2)


def result(s):
    """history and state, and the context closed"""
    hist, d = s.history_fetch(), s.download()
    s.close()
    return hist, d


def same(a, b):
    (ha, da), (hb, db) = a, b
    assert len(ha[0]) == len(hb[0])
    for x, y in zip(ha, hb):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert da["nf"] == db["nf"]
    for k in KEYS:
        assert da[k].shape == db[k].shape and da[k].tobytes() == db[k].tobytes(), k


def finite(r, nobs=NOBS):
    hist, d = r
    assert len(hist[0]) == nobs and np.isfinite(hist[0]).all()
    assert all(np.isfinite(d[k]).all() for k in KEYS)
    assert d["nf"] > 0 and float(d["w"].sum(dtype=np.float64)) > 0.0


@pytest.fixture(scope="module")
def reference(sg, tape):
    """a fresh compact context on the whole map, stepped through the tape (shared; nobody changes it)"""
    s = context(sg, tape)
    s.set_map(tape["lm"])
    stepped(s, tape)
    r = result(s)
    finite(r)
    return r


def test_context_with_a_map_and_no_step_closes(sg, tape, reference):
    s = context(sg, tape)
    s.set_map(tape["lm"])  # (the front end's buffers, and the persistent loop's: the context qualifies)
    s.close()
    s = context(sg, tape)
    s.set_map(tape["lm"])
    stepped(s, tape)
    same(result(s), reference)


@pytest.mark.parametrize("order", ["larger_then_smaller", "smaller_then_larger"])
@pytest.mark.parametrize("rows", ["compact", "plain_rows"])
def test_map_set_again_is_the_last_map_only(sg, tape, monkeypatch, rows, order):
    """slamgpu_set_map twice before the first step, the second map smaller or larger than the first: the run that follows is, bit for
    bit, the run of a fresh context that was given the second map only"""
    if rows == "plain_rows":
        monkeypatch.setenv("SLAMGPU_NO_COMPACT", "1")
    large = tape["lm"]
    near = np.argsort(np.hypot(large[0] - tape["xt"][0][0], large[1] - tape["xt"][0][1]), kind="stable")
    small = np.ascontiguousarray(large[:, np.sort(near[:20])])  # (the 20 landmarks nearest to the start: some are in view at once)
    assert small.shape[1] < large.shape[1]
    first, last = (large, small) if order == "larger_then_smaller" else (small, large)
    out = []
    for maps in ((first, last), (last,)):
        s = context(sg, tape)
        for lm in maps:
            s.set_map(lm)
        stepped(s, tape)
        out.append(result(s))
    finite(out[1])
    same(out[0], out[1])


def test_context_that_only_stepped_closes(sg, tape, monkeypatch):
    """plain rows: slamgpu_step_observe allocates the book's staging and its stream; the persistent loop's buffers never exist"""
    monkeypatch.setenv("SLAMGPU_NO_COMPACT", "1")
    s = context(sg, tape)
    s.set_map(tape["lm"])
    stepped(s, tape)
    assert s.persist_info(cross=True) == (0, 0, 0) and s.persist_status() is None
    r = result(s)
    finite(r)
    monkeypatch.delenv("SLAMGPU_NO_COMPACT")
    s = context(sg, tape)
    s.set_map(tape["lm"])
    stepped(s, tape)
    finite(result(s))


def test_queue_grows_between_two_launches(sg, tape):
    """slamgpu_run_observe with K = 2, then K = 257 (the queue's first 256 entries do not hold it) on one compact context, against 259
    slamgpu_step_observe calls on a twin"""
    a = context(sg, tape)
    a.set_map(tape["lm"])
    for lo, hi in ((0, 2), (2, GROW)):
        a.run_observe(tape["ctl"][lo:hi], tape["Q"], float(tape["dt"]), tape["xt"][lo:hi], tape["mr"], tape["R"], noise=2)
    assert a.persist_info() == (2, GROW)
    ra = result(a)
    b = context(sg, tape)
    b.set_map(tape["lm"])
    stepped(b, tape, GROW)
    rb = result(b)
    finite(rb, GROW)
    same(ra, rb)


def test_context_closed_behind_a_launch_it_never_waited_for(sg, tape, reference):
    s = context(sg, tape)
    s.set_map(tape["lm"])
    s.run_observe(tape["ctl"][:NOBS], tape["Q"], float(tape["dt"]), tape["xt"][:NOBS], tape["mr"], tape["R"], noise=2)
    assert s.persist_info() == (1, NOBS)
    s.close()  # (no sync, no fetch: the launch has only just been enqueued)
    s = context(sg, tape)
    s.set_map(tape["lm"])
    stepped(s, tape)
    same(result(s), reference)
