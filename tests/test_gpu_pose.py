"""Pose posterior on the device (slamgpu_pose_summary, slamgpu_pose_history_*): the weighted mean pose, the scatter about it, the mean
within-particle covariance and sum w^2, reduced over ALL particles by pose_summary_kernel / pose_finish_kernel.

The yardstick is tests/pose_model.py (float64, math.fsum, math.remainder) evaluated on peek(first=0, stride=1, count=N) of the same
context taken immediately before the call.  The tolerances are rounding bounds, derived as tests/test_gpu_map_summary.py derives its
own.  With u = 2^-53, N the particle count, D the larger coordinate range of the cloud (x or y), |mu| the larger coordinate of the
model mean, P = max |Pv entry|: any order of summing n terms in double errs by at most (n - 1) u sum |t_i|, and the weights are
non-negative and sum to 1; terms about a pivot inside the cloud are bounded by D and D^2; every merge of two partial means rounds once
at the size of the mean (u |mu|) and carries that into M2 through delta^2, |delta| <= D; no path from a particle to an output has more
than N such steps; a factor 8 covers the division by the weight sum, the final pivot shift and (log-weights, cos, sin) the few ulps
between two correctly working exp / cos / sin.  The heading deviations u_i are the SAME doubles in the model and on the device (a
float32 difference taken in double and an IEEE remainder are exact or identically rounded), they lie in [-pi, pi] whatever the cloud, so
the scale of a u-term is pi where that of an x-term is D, and the mean of u is carried at a size of at most pi:
    [0] sum w^2        8 N u [0]                          (positive terms: a relative bound)
    [1..2] mean x, y   8 N u (D + |mu|)
    [3] mean heading   8 N u (pi + |[3]|)                 (the sum of w u at scale pi, then one addition of theta_p)
    [4..5] cos, sin    8 N u + 4 u                        (terms of size <= 1; slamgpu_path_summary's bound for the same sums)
    xx, xy, yy         8 N u D (D + |mu|)
    xu, yu             8 N u pi (2 D + |mu|)              (delta_x delta_u: delta_x errs by u |mu| at |delta_u| <= pi, delta_u by u pi at |delta_x| <= D; the terms themselves D pi)
    uu                 16 N u pi^2
    [12..17] mean Pv   8 N u P
and NaN exactly where the model says NaN.  A bound of 0 (N = 1: D = 0) asks for the exact value.  Every check prints its worst
error / bound ratio before it asserts."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pose_model
from conftest import DATA
from test_gpu_particle_assoc import _tape
from test_gpu_particle_device import EXCL_ON, EXE, ERR_INVALID, _course, _ctx, _finish, _host_step, _opt, _same_state

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
KBLOCK, TILE = 256, 1024   # kernels.h: kBlock, kPoseTile
GROUPS = (("sum w^2", slice(0, 1)), ("mean xy", slice(1, 3)), ("mean heading", slice(3, 4)), ("cos sin", slice(4, 6)), ("scatter xy", slice(6, 9)),
          ("scatter xu yu", slice(9, 11)), ("scatter uu", slice(11, 12)), ("mean Pv", slice(12, 18)))


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _compare(got, exp, bound, tag):
    """a summary against the model within the rounding bounds; prints the worst error / bound of each group first"""
    report, bad = [], []
    with np.errstate(all="ignore"):
        err = np.abs(got - exp)
        ratio = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
    for name, sl in GROUPS:
        report.append("%s %.3g (err %.3g)" % (name, np.nanmax(ratio[sl]) if not np.isnan(exp[sl]).all() else 0.0,
                                               np.nanmax(err[sl]) if not np.isnan(exp[sl]).all() else 0.0))
        if not np.array_equal(np.isnan(got[sl]), np.isnan(exp[sl])):
            bad.append(name + ": NaN pattern")
        elif not np.all(err[sl][~np.isnan(exp[sl])] <= bound[sl][~np.isnan(exp[sl])]):
            bad.append(name + ": outside its bound")
    print("pose_summary %s: worst error / bound: %s" % (tag, ", ".join(report)))
    assert not bad, (tag, bad)


def _check(s, logw, tag):
    pk = s.peek(landmarks=False)
    got = s.pose_summary()
    exp = pose_model.summary(pk["xv"], pk["Pv"], pk["w"], logw)
    _compare(got, exp, pose_model.bounds(pk["xv"], pk["Pv"], exp), "%s N %d" % (tag, s.N))
    return got, exp, pk


def _known(sg, c, N, math, logw=False, method=2):
    s = sg.SlamGpu(N, c["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=math, device_observe=True,
                   log_weights=logw)
    s.set_map(c["lm"])
    return s


def _run(s, c, a, b):
    s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)


def _step(s, c, k):
    s.step_observe(c["ctl"][k], c["Q"], c["dt"], c["xt"][k], c["max_range"], c["R"], noise=2)


def _constructed(sg, N, math, logw=False, x0=0.0, heading=None, seed=1):
    """a set built by hand and uploaded: a 1 m cloud about (x0, -3), non-uniform weights with some zeros, non-zero Pv"""
    rng = np.random.default_rng(seed + N)
    s = sg.SlamGpu(N, 4, method=2, rng_mode=sg.RNG_PHILOX, seed=2, math_mode=math, log_weights=logw)
    d = s.download()
    assert d["nf"] == 0
    th = rng.normal(0.7, 0.2, N) if heading is None else heading(rng, N)
    d["xv"] = np.stack([x0 + rng.normal(0.0, 1.0, N), -3.0 + rng.normal(0.0, 0.5, N), th], axis=1).astype(f32)
    A = rng.normal(0.0, 0.2, (N, 3, 3))
    d["Pv"] = (A @ A.transpose(0, 2, 1)).astype(f32)
    if logw:
        w = rng.normal(-700.0, 1.5, N) + np.where(np.arange(N) < TILE, 0.0, -3.0)   # (the tiles' maxima differ)
    else:
        w = rng.uniform(0.0, 1.0, N)
        if N > 2:
            w[1::5] = 0.0
    d["w"] = w.astype(f32)
    s.upload(d)
    return s, d


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_model_on_example_webmap(sg, mm):
    """FastSLAM 2, N = 1 000, after 20 steps: one step at a time, a checked summary after each, until one was taken with a gather pending
    and one with none (the history's resampled flag of the step just made)"""
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, 1000, mm)
    _run(s, c, 0, 20)
    s.history_fetch()
    seen = set()
    for k in range(20, 100):
        _step(s, c, k)
        got, exp, pk = _check(s, False, "webmap math%d step %d" % (mm, k))
        seen.add(bool(s.history_fetch()[2][-1]))
        assert 1.0 <= 1.0 / got[0] <= 1000.0 * (1 + 1e-9) and _healthy(got)
        if len(seen) == 2:
            break
    assert seen == {False, True}, "no summary was taken %s a pending gather" % ("without" if True in seen else "with")
    s.close()


def _healthy(o):
    """what holds of every healthy summary: a resultant length of at most 1, a positive semi-definite scatter diagonal"""
    return math.hypot(o[4], o[5]) <= 1.0 + 1e-12 and o[6] >= 0.0 and o[8] >= 0.0 and o[11] >= 0.0


@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("N", [1, KBLOCK - 1, KBLOCK, KBLOCK + 1, TILE + 1])
def test_constructed_sets(sg, N, mm):
    """uploaded sets: non-uniform weights with zeros, non-zero Pv ([12..17]); one particle, a workgroup less one / exactly / plus one, one
    particle more than a tile of pose_summary_kernel (a second tile of one particle)"""
    s, d = _constructed(sg, N, mm)
    got, exp, pk = _check(s, False, "constructed math%d" % mm)
    assert np.array_equal(pk["xv"], d["xv"]) and np.array_equal(pk["w"], d["w"])
    assert np.abs(got[12:18]).min() > 0.0
    if N == 1:
        assert np.all(got[6:12] == 0.0) and got[0] == 1.0 and got[1] == float(d["xv"][0, 0]) and got[3] == float(d["xv"][0, 2])
    s.close()


@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_far_from_the_origin(sg, mm):
    """a 1 m cloud at x = 1e5 m: D stays the cloud's, |mu| is 1e5.  Raw second moments would cancel ~ u x^2 = 1e-6 m^2 of noise per term
    into a scatter whose bound is ~ 1e-7 m^2"""
    N = TILE + 1
    s, d = _constructed(sg, N, mm, x0=1.0e5)
    got, exp, pk = _check(s, False, "far from the origin math%d" % mm)
    b = pose_model.bounds(pk["xv"], pk["Pv"], exp)
    print("far from the origin: model scatter xx %.3g yy %.3g m^2, bound %.3g m^2" % (exp[6], exp[8], b[6]))
    assert abs(exp[1]) > 9e4 and exp[6] > 100.0 * b[6], "the case would pass vacuously"
    s.close()


@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_headings_at_plus_minus_pi(sg, mm):
    """headings at +-(pi - 0.01) with a little spread: uu is the small spread squared, the resultant length stays near 1"""
    def heading(rng, N):
        side = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        return side * (np.pi - 0.01) + rng.normal(0.0, 0.002, N)
    for N in (KBLOCK + 1, TILE + 1):
        s, d = _constructed(sg, N, mm, heading=heading)
        got, exp, pk = _check(s, False, "headings at +-pi math%d" % mm)
        assert 5e-5 < got[11] < 5e-4 and _healthy(got) and np.hypot(got[4], got[5]) > 0.999, got
        assert abs(abs(np.arctan2(got[5], got[4])) - np.pi) < 0.01 and abs(abs(math.remainder(got[3], 2 * np.pi)) - np.pi) < 0.01
        s.close()


@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_log_weight_context(sg, mm):
    """log-weights far below what exp() can hold unshifted, in two tiles with different maxima; then a webmap run with log-weights"""
    s, d = _constructed(sg, TILE + KBLOCK + 1, mm, logw=True)
    got, exp, pk = _check(s, True, "log-weights constructed math%d" % mm)
    assert 1.0 < 1.0 / got[0] < s.N
    s.close()
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, 1000, mm, logw=True)
    _run(s, c, 0, 25)
    _check(s, True, "log-weights webmap math%d" % mm)
    s.close()


@pytest.mark.parametrize("logw", [False, True], ids=["linear", "log"])
def test_odd_tiles_pending_gather(sg, logw):
    """N = 9 222 (ten tiles of 1 024 particles with six in the last: waves without a particle, finishing stretches without a tile), linear
    and log weights: a checked summary after every step until one was taken straight after an update that resampled, its gather pending"""
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, 9222, 1, logw=logw)
    _run(s, c, 0, 20)
    s.history_fetch()
    for k in range(20, 100):
        _step(s, c, k)
        _check(s, logw, "odd tiles %s step %d" % ("log" if logw else "linear", k))
        if s.history_fetch()[2][-1]:
            break
    else:
        raise AssertionError("no step resampled: no summary was taken with a gather pending")
    s.close()


def test_degenerate_weights_give_nan(sg):
    """all-zero weights, and weights that sum to nothing finite: every entry NaN, return 0 (SLAMGPU_STATUS_DEGENERATE's convention)"""
    N = KBLOCK + 1
    s, d = _constructed(sg, N, 1)
    for w in (np.zeros(N, f32), np.where(np.arange(N) == 7, np.inf, d["w"]).astype(f32), np.where(np.arange(N) == 3, np.nan, d["w"]).astype(f32)):
        s.upload(dict(d, w=w))
        assert np.isnan(s.pose_summary()).all()
    s.upload(d)
    _check(s, False, "after the degenerate uploads")
    s.close()
    s, d = _constructed(sg, N, 1, logw=True)
    s.upload(dict(d, w=np.full(N, -np.inf, f32)))
    assert np.isnan(s.pose_summary()).all()
    s.close()


# ---- determinism, read-only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_deterministic_and_read_only(sg, mm):
    """two calls: the same bits; a pending gather and the state slamgpu_download settles it into: the same bits; a twin that never calls
    the summary ends 30 steps later in the bit-identical state, with the same history"""
    c = _course("FASTSLAM2", 100)

    def run(observe):
        s = _known(sg, c, 1000, mm)
        _run(s, c, 0, 20)
        s.history_fetch()
        pending, hist = 0, []
        for k in range(20, 50):
            _step(s, c, k)
            if observe:
                a, b = s.pose_summary(), s.pose_summary()
                assert a.tobytes() == b.tobytes(), "two summaries of one state differ"
                hist.append(s.history_fetch())
                if hist[-1][2][-1] and pending < 2:  # (this step resampled: its gather is pending)
                    pending += 1
                    d = s.download(landmarks=False)
                    assert s.pose_summary().tobytes() == a.tobytes(), "pending and settled: different bits"
                    assert np.all(d["w"] == d["w"][0])
        if observe:
            assert pending > 0, "no summary was taken with a gather pending"
            hist = tuple(np.concatenate([h[q] for h in hist]) for q in range(3))
        else:
            hist = s.history_fetch()
        d = s.download()
        s.close()
        return hist, d
    _same_state(run(True), run(False), "summaries between the steps")


# ---- the ring -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["step_observe", "run_observe", "step"])
def test_ring_entries_are_the_synchronous_summaries(sg, entry):
    """the ring's entries equal the synchronous summaries a twin (ring off) takes at the same moments, bit for bit; the twin's history
    and final state are the ring context's; no persistent launch while the ring is on"""
    N, steps = 512, 40
    if entry == "step":
        tape = _tape("FASTSLAM2", N, steps)

        def make():
            return sg.SlamGpu(N, tape["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1)

        def drive(s, a, b, each):
            for k in range(a, b):
                st = tape["steps"][k]
                s.step(np.array(st["controls"], f32).reshape(-1, 3), tape["Q"], float(tape["dt"]), np.array(st["zf"], f32).reshape(-1, 2),
                       np.array(st["idf"], np.int32), np.array(st["zn"], f32).reshape(-1, 2), tape["R"])
                each()
    else:
        c = _course("FASTSLAM2", 100)

        def make():
            return _known(sg, c, N, 1)

        def drive(s, a, b, each):
            if entry == "run_observe" and each is _nothing:
                for x in range(a, b, 8):
                    _run(s, c, x, min(b, x + 8))
            else:
                for k in range(a, b):
                    _step(s, c, k) if entry == "step_observe" else _run(s, c, k, k + 1)
                    each()
    r, t = make(), make()
    drive(r, 0, 5, _nothing)
    drive(t, 0, 5, _nothing)
    p0 = r.persist_info()
    r.pose_history_enable(64)
    assert r.pose_history_info() == (0, 0, 64)
    drive(r, 5, steps, _nothing)
    sync = []
    drive(t, 5, steps, lambda: sync.append(t.pose_summary()))
    assert r.pose_history_info() == (0, steps - 5, 64)
    ring = r.pose_history_fetch()
    assert ring.shape == (steps - 5, 18) and ring.tobytes() == np.stack(sync).tobytes(), "ring entries differ from the synchronous summaries"
    assert ring.tobytes() == r.pose_history_fetch().tobytes(), "the fetch consumed something"
    assert r.persist_info() == p0, "the persistent loop ran while the ring was on"
    hr, ht = r.history_fetch(), t.history_fetch()
    assert np.any(hr[2]) and not np.all(hr[2]), "the window holds no resampling step, or nothing else"
    _same_state((hr, r.download()), (ht, t.download()), "ring on / off (%s)" % entry)
    r.close()
    t.close()


def _nothing():
    pass


def test_ring_no_persistent_launch(sg):
    """slamgpu_run_observe on a context the persistent loop would take: with the ring on it takes its loop of launches"""
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, 512, 1)
    s.pose_history_enable(32)
    _run(s, c, 0, 16)
    assert s.persist_info() == (0, 0), "the persistent loop ran while the ring was on"
    assert s.pose_history_info() == (0, 16, 32)
    s.pose_history_enable(0)
    _run(s, c, 16, 32)
    assert s.persist_info()[0] == 1 and s.pose_history_info() == (0, 0, 0), "off means off: the persistent loop is back"
    s.close()


def test_ring_on_run_particle(sg):
    """slamgpu_run_particle, N = 512: entry k is bit for bit what slamgpu_pose_summary returns after the equivalent host-driven sequence of
    k + 1 iterations; the filter does not notice the ring (a device-driven twin with it off: same history, reports and state)"""
    N, steps, K = 512, 30, 10
    c = _course("FASTSLAM2", 150)
    opt = _opt(EXCL_ON, 1, 0.02)
    far = np.array([1000.0, 1000.0, 0.0], f32)   # iteration 12 sees nothing: no update, an entry all the same
    xts = [far if k == 12 else c["xt"][k] for k in range(steps)]
    r, t, h = _ctx(sg, c, N, 2, 1), _ctx(sg, c, N, 2, 1), _ctx(sg, c, N, 2, 1)
    r.pose_history_enable(64)
    for a in range(0, steps, K):
        for x in (r, t):
            x.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], xts[a:a + K], c["max_range"], c["R"], noise=2, **opt)
    sync = []
    for k in range(steps):
        _host_step(h, c, k, opt, xts[k])
        sync.append(h.pose_summary())
    assert r.pose_history_info() == (0, steps, 64)
    ring = r.pose_history_fetch()
    same = [ring[k].tobytes() == sync[k].tobytes() for k in range(steps)]
    print("run_particle ring: entries equal to the host-driven summaries:", sum(same), "of", steps)
    assert all(same), [k for k in range(steps) if not same[k]]
    rep_r, rep_t = r.particle_report_fetch(), t.particle_report_fetch()
    assert np.array_equal(rep_r, rep_t) and not np.asarray(rep_r)[12].any()
    fr, ft, fh = _finish(r), _finish(t), _finish(h)
    assert np.any(fr[0][2]), "the run never resampled"
    _same_state(fr, ft, "run_particle, ring on / off")
    _same_state(fr, fh, "run_particle with the ring / host-driven twin")


def test_ring_capacity_upload_and_launch_counts(sg):
    """capacity 4 with 10 records: first = 6; entries outside the retained range are refused, outputs untouched; entries survive
    slamgpu_upload; with the ring never enabled and no summary asked for, no launch of the new kernels"""
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, 512, 1)
    s.profile(True)
    _run(s, c, 0, 10)
    for k in range(10, 14):
        _step(s, c, k)
    s.peek(landmarks=False)
    s.download()
    for name in ("pose_summary", "pose_finish"):
        assert s.kernel_time(name)[1] == 0, name
    assert s.pose_history_info() == (0, 0, 0)
    assert s.pose_history_fetch(0, 0).shape == (0, 18)
    with pytest.raises(sg.SlamGpuError) as e:
        s.pose_history_record()
    assert e.value.code == ERR_INVALID
    s.pose_history_enable(4)
    sync = []
    for k in range(14, 24):
        _step(s, c, k)
        sync.append(s.pose_summary())
    assert s.pose_history_info() == (6, 10, 4)
    for name in ("pose_summary", "pose_finish"):
        assert s.kernel_time(name)[1] == 20, name   # ten entries, ten synchronous summaries
    got = s.pose_history_fetch()
    assert got.tobytes() == np.stack(sync[6:]).tobytes()
    assert s.pose_history_fetch(8, 2).tobytes() == np.stack(sync[8:]).tobytes() and s.pose_history_fetch(7, 1).tobytes() == sync[7].tobytes()
    out = np.full((4, 18), -1.0)
    vp = C.c_void_p
    for first, count in ((5, 1), (5, 5), (9, 2), (10, 1), (6, -1), (-1, 1)):
        assert s.L.slamgpu_pose_history_fetch(s.h, first, count, out.ctypes.data_as(vp)) == ERR_INVALID, (first, count)
    assert s.L.slamgpu_pose_history_fetch(s.h, 6, 4, None) == ERR_INVALID
    assert s.L.slamgpu_pose_history_fetch(s.h, 10, 0, None) == 0
    assert np.all(out == -1.0)
    # explicit records (callers of slamgpu_update and its kin record themselves), and slamgpu_upload keeps the entries
    s.pose_history_record()
    assert s.pose_history_info() == (7, 11, 4) and s.pose_history_fetch(10, 1).tobytes() == sync[9].tobytes()
    before = s.pose_history_fetch()
    s.upload(s.download())
    assert s.pose_history_info() == (7, 11, 4) and s.pose_history_fetch().tobytes() == before.tobytes()
    s.pose_history_record()
    assert s.pose_history_fetch(11, 1).tobytes() == s.pose_summary().tobytes()
    # a restart drops the entries and numbers from 0; 0 stops
    s.pose_history_enable(8)
    assert s.pose_history_info() == (0, 0, 8)
    s.pose_history_enable(0)
    assert s.pose_history_info() == (0, 0, 0)
    s.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(sg):
    c = _course("FASTSLAM2", 100)
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    out = np.full(18, -1.0)
    p = out.ctypes.data_as(C.c_void_p)
    assert shard.L.slamgpu_pose_summary(shard.h, p) == ERR_INVALID and b"single contexts only" in shard.L.slamgpu_last_error()
    assert shard.L.slamgpu_pose_history_enable(shard.h, 8) == ERR_INVALID
    assert shard.pose_history_info() == (0, 0, 0)
    assert shard.L.slamgpu_pose_history_record(shard.h) == ERR_INVALID
    assert shard.L.slamgpu_pose_history_fetch(shard.h, 0, 1, p) == ERR_INVALID
    assert np.all(out == -1.0)
    shard.close()
    s = _known(sg, c, 512, 1)
    _run(s, c, 0, 10)
    pk0 = s.peek(landmarks=False)
    assert s.L.slamgpu_pose_summary(s.h, None) == ERR_INVALID
    assert s.L.slamgpu_pose_history_enable(s.h, -1) == ERR_INVALID and s.pose_history_info() == (0, 0, 0)
    pk1 = s.peek(landmarks=False)
    for k in ("xv", "Pv", "w"):
        assert np.array_equal(pk0[k], pk1[k]), k
    s.close()


# ---- the path recorder ----------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_path_recorder(sg):
    """with both on, the newest record's slamgpu_path_summary mean (x, y) is this summary's [1..2]: within the sum of the two documented
    bounds -- the path summary's 8 N u (D + |mu|) and its fixed-point term N 2^-63 D, plus this summary's 8 N u (D + |mu|)"""
    c = _course("FASTSLAM2", 100)
    N = 1000
    s = _known(sg, c, N, 1)
    s.path_enable(16)
    s.pose_history_enable(16)
    _run(s, c, 0, 30)
    a, b, _ = s.path_info()
    assert s.pose_history_info()[:2] == (a, b) == (14, 30)
    ps = s.path_summary(b - 1, 1)
    got, exp, pk = _check(s, False, "beside the path recorder")
    D = max(np.ptp(pk["xv"][:, 0].astype(f64)), np.ptp(pk["xv"][:, 1].astype(f64)))
    mu = max(abs(exp[1]), abs(exp[2]))
    tol = 2.0 * 8.0 * N * U * (D + mu) + N * 2.0 ** -63 * D
    err = np.abs(ps["mean"][0] - got[1:3])
    print("path recorder: |path mean - pose mean| %.3g, %.3g; tolerance %.3g; ratio %.3g" % (err[0], err[1], tol, err.max() / tol))
    assert np.all(err <= tol)
    assert s.pose_history_fetch(b - 1, 1).tobytes() == got.tobytes()
    s.close()


# ---- slam-backend ---------------------------------------------------------------------------------------------------------------------
def test_slam_backend_pose_posterior():
    """slam-backend -NPARTICLES 512 -pose posterior: the line parses, the mean NEES is finite, the share lies in [0, 1]; everything else
    is the output without the option"""
    def run(extra):
        r = subprocess.run([EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
                            "-SWITCH_SEED_RANDOM", "7", "-rng", "philox", "-maxsteps", "2000", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        return [re.sub(r"-?\d+\.\d+ us", "T us", re.sub(r"= \d+ % of", "= T % of", ln)) for ln in r.stdout.splitlines()]
    plain, post = run(()), run(("-pose", "posterior"))
    lines = [ln for ln in post if ln.startswith("pose posterior:")]
    assert len(lines) == 1 and [ln for ln in post if not ln.startswith("pose posterior:")] == plain
    m = re.match(r"pose posterior: (\d+) entries kept, mean distance to the true position (\S+) m \(filtered estimates of the same steps: (\S+) m\); "
                 r"mean NEES (\S+), NEES <= 7.8147 in (\S+) of the steps \((\d+) entries without a NEES\); median effective sample size (\S+)$", lines[0])
    assert m, lines[0]
    print("slam-backend -pose posterior:", lines[0])
    n, dw, df, nees, share, bad, ess = int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)), int(m.group(6)), float(m.group(7))
    assert n > 0 and math.isfinite(nees) and nees >= 0.0 and 0.0 <= share <= 1.0 and 1.0 <= ess <= 512.0 and bad < n
    assert math.isfinite(dw) and math.isfinite(df)
