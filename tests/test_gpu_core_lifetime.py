"""Who allocates and frees what in the core and the posterior layer (slamgpu_create / slamgpu_destroy, slamgpu_ctx::own and ::po,
posterior_release): contexts close cleanly in every state their buffers, rings and staging slots can be in -- untouched, a ring enabled,
enabled again at another capacity with appends in flight and disabled, the pinned packet of slamgpu_innovation_summary grown with slots
in flight, both label pieces reused, slamgpu_peek's staging grown -- and a later context is unaffected: bit for bit a fresh twin.
256 particles on example_webmap, 12 observation steps; every sequence here is a legal one.  (The caller's totals buffer of
slamgpu_shard_set_totals_buffer: tests/test_gpu_multigpu_lifetime.py.)"""
import numpy as np
import pytest

from conftest import sim_args

pytestmark = pytest.mark.gpu
f32 = np.float32
N, NOBS = 256, 12
KEYS = ("xv", "Pv", "w", "xf", "Pf")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


@pytest.fixture(scope="module")
def tape():
    from slam_amd import host
    tp = host.make_tape(sim_args("example_webmap", "FASTSLAM2", N, 7), max_obs=NOBS)
    tp["ctl"] = [np.array(st["controls"], f32).reshape(-1, 3) for st in tp["steps"]]
    assert len(tp["steps"]) == NOBS
    return tp


def context(sg, tp, rng_mode=None, **kw):
    return sg.SlamGpu(N, tp["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX if rng_mode is None else rng_mode,
                      seed=5, math_mode=1, **kw)


def stepped(s, tp, lo=0, hi=NOBS):
    for k in range(lo, hi):
        st = tp["steps"][k]
        s.step(tp["ctl"][k], tp["Q"], float(tp["dt"]), st["zf"], st["idf"], st["zn"], tp["R"])


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


@pytest.fixture(scope="module")
def reference(sg, tape):
    """a fresh context stepped through the tape (shared; nobody changes it)"""
    s = context(sg, tape)
    stepped(s, tape)
    hist, d = r = result(s)
    assert len(hist[0]) == NOBS and np.isfinite(hist[0]).all()
    assert all(np.isfinite(d[k]).all() for k in KEYS)
    assert d["nf"] > 0 and float(d["w"].sum(dtype=np.float64)) > 0.0
    return r


def later_context_is_the_reference(sg, tape, reference):
    s = context(sg, tape)
    stepped(s, tape)
    same(result(s), reference)


def reobserved(tape, least=1):
    """the first step of the tape that re-observes at least `least` landmarks, and its packet"""
    k = next(k for k, st in enumerate(tape["steps"]) if len(st["idf"]) >= least)
    st = tape["steps"][k]
    return k, np.asarray(st["zf"], f32).reshape(-1, 2), np.asarray(st["idf"], np.int32)


@pytest.mark.parametrize("rng", ["PHILOX", "TAPE"])
def test_untouched_context_closes(sg, tape, reference, rng):
    context(sg, tape, rng_mode=getattr(sg, "RNG_" + rng)).close()
    later_context_is_the_reference(sg, tape, reference)


def test_pose_ring_enabled_again_and_disabled(sg, tape, reference):
    s = context(sg, tape)
    s.pose_history_enable(4)
    stepped(s, tape, 0, 5)  # (every step appends; nothing waits for the device)
    assert s.pose_history_info() == (1, 5, 4)
    s.pose_history_enable(7)  # appends in flight
    assert s.pose_history_info() == (0, 0, 7)
    stepped(s, tape, 5, 9)
    ring = s.pose_history_fetch()
    assert ring.shape == (4, 18) and np.isfinite(ring).all() and ring[-1].tobytes() == s.pose_summary().tobytes()
    stepped(s, tape, 9, 10)
    s.pose_history_enable(0)
    assert s.pose_history_info() == (0, 0, 0)
    stepped(s, tape, 10, NOBS)
    s.close()
    later_context_is_the_reference(sg, tape, reference)


def test_innovation_ring_enabled_again_and_disabled(sg, tape, reference):
    s = context(sg, tape)
    s.innovation_history_enable(256)
    stepped(s, tape, 0, 5)  # (every step appends its packet's entries)
    assert s.innovation_history_info()[2:] == (256, 5)
    s.innovation_history_enable(128)  # appends in flight
    assert s.innovation_history_info() == (0, 0, 128, 0)
    stepped(s, tape, 5, 9)
    k, zf, idf = reobserved(tape)
    assert k < 9, "no landmark to measure against yet"
    s.innovation_record(zf[:1], idf[:1], tape["R"])
    first, nxt, cap, records = s.innovation_history_info()
    assert cap == 128 and records == 5 and 0 < nxt - first <= 128
    last = s.innovation_history_fetch(nxt - 1, 1)
    assert last[0].tobytes() == s.innovation_summary(zf[:1], idf[:1], tape["R"])[0].tobytes() and int(last[2][0]) == int(idf[0])
    s.innovation_history_enable(0)
    assert s.innovation_history_info() == (0, 0, 0, 0)
    stepped(s, tape, 9, NOBS)
    s.close()
    later_context_is_the_reference(sg, tape, reference)


def test_path_ring_enabled_again_and_disabled(sg, tape, reference):
    s = context(sg, tape)
    s.path_enable(4)
    stepped(s, tape, 0, 5)
    assert s.path_info()[2] == 4 and s.path_info()[1] >= 4
    s.path_trace()  # (the traces' staging exists: it goes with the ring)
    s.path_enable(7)  # appends in flight
    assert s.path_info() == (0, 0, 7)
    stepped(s, tape, 5, 9)
    first, nxt, _ = s.path_info()
    assert nxt - first >= 4
    xyt, parent = s.path_fetch(nxt - 1)
    assert xyt.tobytes() == s.peek(landmarks=False)["xv"].tobytes() and ((parent >= 0) & (parent < N)).all()
    assert np.isfinite(s.path_summary()["mean"]).all()
    s.path_enable(0)
    assert s.path_info() == (0, 0, 0)
    stepped(s, tape, 9, NOBS)
    s.close()
    later_context_is_the_reference(sg, tape, reference)


def test_innovation_summary_packet_grows_with_slots_in_flight(sg, tape, reference):
    """m = 3, then m = 65: the smallest count past the pinned packet's first 64 (repeated slots are allowed)"""
    k, zf, idf = reobserved(tape, 3)
    R = tape["R"]
    small = zf[:3], idf[:3]
    large = np.resize(zf, (65, 2)).astype(f32), np.resize(idf, 65).astype(np.int32)
    fresh = []
    for z, i in (small, large):  # each call alone on a fresh context
        t = context(sg, tape)
        stepped(t, tape, 0, k + 1)
        fresh.append(t.innovation_summary(z, i, R))
        t.close()
    s = context(sg, tape)
    stepped(s, tape, 0, k + 1)
    got = [s.innovation_summary(*p, R) for p in (small, small, large, small)]
    for g, f in zip(got, (fresh[0], fresh[0], fresh[1], fresh[0])):
        assert g[0].tobytes() == f[0].tobytes() and np.array_equal(g[1], f[1])
    assert np.isfinite(got[2][0][:, 0]).all() and (got[2][1] > 0).all()
    stepped(s, tape, k + 1, NOBS)
    s.close()
    later_context_is_the_reference(sg, tape, reference)


def test_innovation_summary_labels_reuses_both_pieces(sg, tape):
    k, zf, idf = reobserved(tape, 2)
    lab = np.tile(idf, (N, 1)).astype(np.int32)
    t = context(sg, tape, particle_maps=True)
    stepped(t, tape, 0, k + 1)
    fresh = t.innovation_summary_labels(zf, lab, tape["R"])
    t.close()
    s = context(sg, tape, particle_maps=True)
    stepped(s, tape, 0, k + 1)
    for _ in range(4):  # (a call of this size takes one piece: the third and the fourth find theirs used)
        got = s.innovation_summary_labels(zf, lab, tape["R"])
        assert got[0].tobytes() == fresh[0].tobytes() and np.array_equal(got[1], fresh[1])
    assert (fresh[1] > 0).all() and np.isfinite(fresh[0][:, 0]).all()
    s.close()
    t = context(sg, tape, particle_maps=True)
    stepped(t, tape, 0, k + 1)
    again = t.innovation_summary_labels(zf, lab, tape["R"])
    t.close()
    assert again[0].tobytes() == fresh[0].tobytes()


def test_peek_staging_grows(sg, tape, reference):
    s = context(sg, tape)
    stepped(s, tape, 0, 9)
    few, all_ = s.peek(landmarks=False, first=3, count=4), s.peek()
    assert all_["nf"] > 0
    d4, d = s.download(landmarks=False, first=3, count=4), s.download()
    for k in ("xv", "Pv", "w"):
        assert few[k].tobytes() == d4[k].tobytes(), k
    for k in KEYS:
        assert all_[k].shape == d[k].shape and all_[k].tobytes() == d[k].tobytes(), k
    stepped(s, tape, 9, NOBS)
    s.close()
    later_context_is_the_reference(sg, tape, reference)
