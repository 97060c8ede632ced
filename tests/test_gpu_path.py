"""Path posterior on the device (slamgpu_path_*): recorded ancestry, traces and the smoothed path.

The yardstick for the records is a TWIN CONTEXT: same configuration and seed, recording off, driven one step at a time, read through
the existing API after every step -- peek() gives the poses of the step's set, ancestors() (the identity when stats() says the step
did not resample) its parents.  The twin's per-step poses and ancestor arrays ARE the expected records; nothing is compared with the
recorder's own output.  Traces are checked against a host walk over those records, the summary against the float64 model of
tests/path_model.py evaluated on them and on the twin's weights.

Tolerances of the summary are rounding bounds of the same derivation as tests/test_gpu_map_summary.py, with u = 2^-53, N the particle
count, D_r the larger coordinate range of the ancestors' poses in record r and |mu| the larger coordinate of the model mean: any order
of summing n terms in double errs by at most (n - 1) u sum |t_i|; terms about a pivot inside the cloud are bounded by D and D^2; every
merge of two partial means rounds once at the size of the mean and carries that into M2 through delta^2, |delta| <= D; no path from a
record to an output has more than N such steps; a factor 8 for the division by the weight sum and the final pivot shift:
    mean 8 N u (D + |mu|) | scatter 8 N u D (D + |mu|) | cos / sin sums 8 N u + 4 u (one double cos / sin on each side) | distinct exact
    | NaN pattern exact.
(The library pushes the descendants' weights down the records in fixed point, units of 2^-62 of the normalised weight: at most
N 2^-63 of weight per record is misplaced, N u / 1024 -- inside every bound above.)  Every check prints its worst error / bound first.

Not covered: distributed (slamgpu_dist_connect) contexts -- every one of them is also a shard (n_particles_global != n_particles), which
is; and the reference-order resampling of small strict TAPE contexts (the twin method needs Philox).
Wall time of this file on an MI355X: not measured on its own yet."""
import os
import re
import subprocess

import numpy as np
import pytest

import path_model
from conftest import DATA
from test_gpu_particle_assoc import _predicts, _tape
from test_gpu_particle_device import EXCL_ON, EXE, ERR_INVALID, _course, _ctx, _opt
from test_gpu_particle_lists import _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
KERNELS = ("path_compose", "path_record", "path_trace", "path_seed", "path_push", "path_finish")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _known(sg, c, N, method, math, logw=False):
    s = sg.SlamGpu(N, c["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=math, device_observe=True,
                   log_weights=logw)
    s.set_map(c["lm"])
    return s


def _run(s, c, a, b):
    s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _twin_read(t, made=True):
    """what the existing API says about the step the twin has just made: (poses, parents, resampled, weights).  made = False: the step
    made no update (no observation): nothing was resampled, whatever ancestors() and stats() still say about the update before it"""
    pk = t.peek(landmarks=False)
    if not made:
        return pk["xv"], np.arange(t.N, dtype=np.int32), False, pk["w"]
    return pk["xv"], t.ancestors(), bool(t.stats()[1]), pk["w"]


def _ps_bits(ps):
    return b"".join(_bits(ps[q]) for q in ("mean", "scatter", "cs", "distinct"))


def _pp_step(x, c, k, opt):
    """one host-driven per-particle step (observation made on the device, fetched, slamgpu_update_particle): was an update made?"""
    for V, G, phi in c["ctl"][k]:
        x.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
    o = x.observe(c["xt"][k], c["max_range"], c["R"], noise=2)
    made = len(o["z"]) > 0
    if made:
        x.update_particle(o["z"], c["R"], **opt)
    x.estimate_async()
    return made


def _tape_step(x, tape, k):
    """one host-driven known-association step of a tape (slamgpu_update): was an update made?"""
    st = tape["steps"][k]
    _predicts(x, st, tape)
    zf, zn = np.array(st["zf"], f32).reshape(-1, 2), np.array(st["zn"], f32).reshape(-1, 2)
    made = len(zf) + len(zn) > 0
    if made:
        x.update(zf, np.array(st["idf"], np.int32), zn, tape["R"])
    x.estimate_async()
    return made


def _twin_steps(t, c, a, b):
    out = []
    for k in range(a, b):
        _run(t, c, k, k + 1)
        out.append(_twin_read(t))
    return out


def _same_records(s, exp, first, what):
    """records first .. of the recorded context against the twin's steps exp[first ..], bit for bit"""
    a, b, _ = s.path_info()
    assert (a, b) == (first, len(exp)), (what, a, b)
    for r in range(first, len(exp)):
        xyt, parent = s.path_fetch(r)
        assert _bits(xyt) == _bits(exp[r][0]), (what, "pose of record %d" % r)
        want = exp[r][1] if r > 0 else np.arange(s.N, dtype=np.int32)
        assert np.array_equal(parent, want), (what, "parents of record %d" % r, int((parent != want).sum()))


def _same_final(s, t, what):
    hs, ht = s.history_fetch(), t.history_fetch()
    for x, y in zip(hs, ht):
        assert _bits(np.asarray(x)) == _bits(np.asarray(y)), (what, "history")
    assert _bits(s.last_history_status) == _bits(t.last_history_status), what
    ds, dt = s.download(), t.download()
    assert ds["nf"] == dt["nf"], what
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert _bits(ds[k]) == _bits(dt[k]), (what, k)


def _walk(recs, origin, i):
    """host walk over records (oldest first): (xyt, index) of present particle i"""
    a = int(origin[i])
    xyt, idx = [], []
    for pose, parent in reversed(recs):
        xyt.append(pose[a])
        idx.append(a)
        a = int(parent[a])
    return np.array(xyt[::-1], f32).reshape(-1, 3), np.array(idx[::-1], np.int32)


def _recs(exp, first=0):
    N = len(exp[-1][1])
    return [(exp[r][0], exp[r][1] if r > 0 else np.arange(N, dtype=np.int32)) for r in range(first, len(exp))]


CUTS = (0, 1, 8, 9, 30, 47, 64)


@pytest.mark.parametrize("method,math,N", [(2, 1, 1000), (1, 1, 1000), (2, 0, 1000), (1, 0, 1000), (2, 1, 100000), (1, 1, 100000), (2, 0, 100000),
                                           (1, 0, 100000)])
def test_records_compact(sg, method, math, N):
    """example_webmap (compact rows), run_observe in uneven batches: every record equals the twin's step; the filter does not notice"""
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 100)
    s, t = _known(sg, c, N, method, math), _known(sg, c, N, method, math)
    assert s.genealogy_rows()[1] <= 40, "not the compact layout"
    s.path_enable(CUTS[-1])
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        _run(s, c, a, b)
    exp = _twin_steps(t, c, 0, CUTS[-1])
    rs = [e[2] for e in exp]
    print("records compact m%d math%d N%d: %d of %d steps resampled" % (method, math, N, sum(rs), len(rs)))
    assert any(rs) and not all(rs), "the window holds no resampling step, or nothing else"
    if N <= 2048:
        assert s.persist_info() == (0, 0), "the persistent loop ran while the path was recorded"
    what = "compact m%d math%d N%d" % (method, math, N)
    _same_records(s, exp, 0, what)
    _same_final(s, t, what)
    s.close()
    t.close()


def test_records_plain_rows(sg, tmp_path_factory):
    """a 1 000-landmark map (plain genealogy rows, observation packets in device memory), log-weights, N not a multiple of 256"""
    c = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 40)
    N = 3000
    s, t = _known(sg, c, N, 2, 1, logw=True), _known(sg, c, N, 2, 1, logw=True)
    assert s.genealogy_rows()[1] > 40, "not the plain layout"
    s.path_enable(64)
    for a, b in ((0, 3), (3, 4), (4, 29), (29, 40)):
        _run(s, c, a, b)
    exp = _twin_steps(t, c, 0, 40)
    rs = [e[2] for e in exp]
    assert any(rs) and not all(rs), "the window holds no resampling step, or nothing else"
    _same_records(s, exp, 0, "plain rows")
    _same_final(s, t, "plain rows")
    s.close()
    t.close()


def test_composition_of_unrecorded_updates(sg):
    """three updates, then one record: its parents are the composition of the twin's three ancestor arrays; a call that makes no
    update in between (update_particle without observations) changes nothing"""
    N = 1024
    c = _course("FASTSLAM2", 40)
    opt = _opt(EXCL_ON, 1, 0.02)
    s, t = _ctx(sg, c, N, 2, 1, n_effective=N), _ctx(sg, c, N, 2, 1, n_effective=N)  # (NEFFECTIVE N: every step resamples)
    for x in (s, t):
        for k in range(10):
            _pp_step(x, c, k, opt)
    s.path_enable(4)
    s.path_record()
    anc = []
    for k in (10, 11, 12):
        for x in (s, t):
            assert _pp_step(x, c, k, opt), "step %d has no observation" % k
            rep = x.update_particle(np.zeros((0, 2), f32), c["R"], **opt)  # no observation, no update: Ctrl.resampled keeps its value
            assert rep["rewritten"] == 0 and rep["opened"] == 0
        anc.append((t.ancestors(), bool(t.stats()[1])))
    assert sum(r for _, r in anc) >= 2, "fewer than two of the three updates resampled"
    s.path_record()
    want = anc[0][0][anc[1][0][anc[2][0]]]
    xyt, parent = s.path_fetch(1)
    assert np.array_equal(parent, want), int((parent != want).sum())
    assert not np.array_equal(want, anc[2][0]), "the composition is the last array alone: the case shows nothing"
    assert _bits(xyt) == _bits(t.peek(landmarks=False)["xv"])
    assert np.array_equal(s.path_fetch(0)[1], np.arange(N))
    _same_final(s, t, "composition")
    s.close()
    t.close()


def test_trace(sg):
    """ten particles and -1: xyt and index equal a host walk over the twin's records, bit for bit -- right after a record (origin the
    identity) and with one un-recorded update behind it (origin the twin's ancestors of that update)"""
    N = 1000
    c = _course("FASTSLAM2", 100)
    s, t = _known(sg, c, N, 2, 1), _known(sg, c, N, 2, 1)
    s.path_enable(128)
    _run(s, c, 0, 40)
    exp = _twin_steps(t, c, 0, 40)
    k, seen = 40, set()
    who = [0, 1, 63, 64, 255, 256, 500, 777, 998, 999]
    while len(seen) < 2 and k < 100:  # until -1 has been asked for after a step that resampled and after one that did not
        _run(s, c, k, k + 1)
        exp += _twin_steps(t, c, k, k + 1)
        k += 1
        recs, ident = _recs(exp), np.arange(N)
        for i in who:
            xyt, idx = s.path_trace(i)
            wx, wi = _walk(recs, ident, i)
            assert _bits(xyt) == _bits(wx) and np.array_equal(idx, wi), (k, i)
        resampled, w = exp[-1][2], exp[-1][3]
        best = int(np.argmax(w))  # (numpy: the first of the largest)
        xyt, idx = s.path_trace(-1)
        if not resampled:
            assert idx[-1] == best and _bits(xyt) == _bits(_walk(recs, ident, best)[0]), k
        else:
            assert idx[-1] == 0, "under a pending gather every weight is 1 / N: the first particle"
        seen.add(resampled)
    assert seen == {False, True}
    # a window of the records: the same rows
    xyt, idx = s.path_trace(5)
    wx, wi = s.path_trace(5, first=7, count=20)
    assert _bits(wx) == _bits(xyt[7:27]) and np.array_equal(wi, idx[7:27])
    # one update that is not recorded: present particle i descends from the newest record's particle ancestors[i]
    origin = None
    while k < 100 and (origin is None or np.array_equal(origin, np.arange(N))):  # (until such an update resampled)
        assert origin is None, "composing two un-recorded updates is test_composition's business"
        for x in (s, t):
            x.step_observe(c["ctl"][k], c["Q"], c["dt"], c["xt"][k], c["max_range"], c["R"], noise=2, record_estimate=False)
        k += 1
        if t.stats()[1]:
            origin = t.ancestors()
        else:
            for x in (s, t):  # not this one: record it and try the next
                x.estimate_async()
            s.path_record()
            exp.append(_twin_read(t))
    assert origin is not None
    assert s.path_info()[1] == len(exp)
    for i in who:
        xyt, idx = s.path_trace(i)
        wx, wi = _walk(_recs(exp), origin, i)
        assert _bits(xyt) == _bits(wx) and np.array_equal(idx, wi), ("unrecorded update", i)
    _same_final(s, t, "trace")
    s.close()
    t.close()


def _compare(ps, m, N, tag):
    """the summary against the model within the rounding bounds; prints the worst error / bound of each quantity first"""
    k = 8.0 * N * U
    bounds = dict(mean=k * (m["D"] + m["mu"]), scatter=k * m["D"] * (m["D"] + m["mu"]), cs=np.full(len(m["D"]), k + 4.0 * U))
    report, bad = [], []
    for q in ("mean", "scatter", "cs"):
        got, exp, bound = ps[q], m[q], bounds[q][:, None]
        err = np.abs(got - exp)
        some = ~np.isnan(exp)
        ratio = np.where(some & (err > 0), err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
        report.append("%s %.3g (err %.3g)" % (q, ratio.max() if ratio.size else 0.0, np.nanmax(err) if some.any() else 0.0))
        if not np.array_equal(np.isnan(got), np.isnan(exp)):
            bad.append(q + ": NaN pattern")
        elif not np.all(err[some] <= np.broadcast_to(bound, err.shape)[some]):
            bad.append(q + ": outside its bound")
    print("path_summary %s: N %d, %d records, distinct %d .. %d; worst error / bound: %s" %
          (tag, N, len(m["D"]), int(m["distinct"].min()), int(m["distinct"].max()), ", ".join(report)))
    assert np.array_equal(ps["distinct"], m["distinct"]), (tag, "distinct")
    assert not bad, (tag, bad)


def _summaries_both_states(s, t, step, exp, first, k, last, logw, tag):
    """steps k .. one at a time (step(x, k): one recorded step of context x; was an update made?), a checked summary after each, until
    one was taken with a gather pending and one with none"""
    seen = set()
    N = s.N
    while len(seen) < 2 and k < last:
        step(s, k)
        exp.append(_twin_read(t, step(t, k)))
        k += 1
        ps = s.path_summary()
        # (the weights of the present set: the twin's peek -- 1 / N behind a step that resampled, as peek shows them)
        m = path_model.summary(_recs(exp, first), np.arange(N), exp[-1][3], logw)
        _compare(ps, m, N, "%s step %d (%s)" % (tag, k - 1, "gather pending" if exp[-1][2] else "no gather pending"))
        assert _ps_bits(ps) == _ps_bits(s.path_summary()), "two summaries of one state differ"
        seen.add(exp[-1][2])
    assert seen == {False, True}, "no summary was taken %s a pending gather" % ("without" if True in seen else "with")
    return k, m


# (N = 9 222: 37 tiles of 256 particles with six in the last, waves without a particle; linear and log weights)
@pytest.mark.parametrize("method,math,N,logw", [(2, 1, 100000, False), (1, 0, 1000, False), (2, 1, 3000, True), (2, 1, 9222, False), (2, 1, 9222, True)])
def test_summary(sg, method, math, N, logw):
    """against tests/path_model.py on the twin's records and weights; with a gather pending and with none; linear and log-weights"""
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 100)
    s, t = _known(sg, c, N, method, math, logw), _known(sg, c, N, method, math, logw)
    s.path_enable(128)
    _run(s, c, 0, 60)
    exp = _twin_steps(t, c, 0, 60)
    k, m = _summaries_both_states(s, t, lambda x, k: _run(x, c, k, k + 1) or True, exp, 0, 60, 100, logw,
                                  "m%d math%d N%d logw%d" % (method, math, N, logw))
    assert m["distinct"][-1] == N or exp[-1][2], "every present particle is its own ancestor in a record just made without a resample"
    assert m["distinct"][0] < N, "nothing has coalesced in %d steps: the case shows little" % k
    # windows are the rows of the full call, bit for bit
    full = s.path_summary()
    for first, count in ((0, 1), (k - 1, 1), (7, 20), (k // 2, k - k // 2)):
        win = s.path_summary(first, count)
        for q in ("mean", "scatter", "cs", "distinct"):
            assert _bits(win[q]) == _bits(full[q][first:first + count]), (first, count, q)
    _same_final(s, t, "summary")
    s.close()
    t.close()


def test_summary_far_from_the_origin(sg):
    """the state moved to (1e5, -1e5) m through upload (poses and landmarks alike: the observations, made from the true pose, fit as
    before): the retained records are dropped, the numbering goes on, and the fresh records are summarised at |mu| = 1e5 with D the
    cloud's own size (raw second moments would cancel ~ u x^2 = 1e-6 m^2 into a scatter whose bound is far below that).  Driven by
    slamgpu_update (known association from a tape) + estimate_async + path_record.
    Three fresh records: the uploaded set itself, then two filter steps.  Not more, and not "until a step has not resampled" as the
    other summary cases do: in float32 at 1e5 m (7.8 mm to the next pose) the FILTER does not last -- on an MI355X the twin, which
    records nothing, keeps 3 and then 1 distinct ancestors after the first steps there and its weights are NaN from the fifth on -- and
    a degenerate state (every double NaN, test_summary_degenerate_weights) says nothing about sums far from the origin.  Both states
    of the gather are test_summary's business."""
    N = 100000
    tape = _tape("FASTSLAM2", 100, 60, seed=7)
    kw = dict(method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1)
    s, t = sg.SlamGpu(N, tape["nlm"], **kw), sg.SlamGpu(N, tape["nlm"], **kw)
    s.path_enable(32)

    def step(x, k):
        made = _tape_step(x, tape, k)
        if x is s:
            s.path_record()
        return made
    exp = []
    for k in range(30):
        step(s, k)
        exp.append(_twin_read(t, step(t, k)))
    _same_records(s, exp, 0, "before the upload")
    d = t.download()
    shift = np.array([1e5, -1e5])
    d["xv"] = d["xv"].copy()
    d["xv"][:, :2] = (d["xv"][:, :2].astype(f64) + shift).astype(f32)
    d["xf"] = (d["xf"].astype(f64) + shift).astype(f32)
    for x in (s, t):
        x.upload(d)
    assert s.path_info() == (30, 30, 32)
    with pytest.raises(sg.SlamGpuError) as e:
        s.path_fetch(29)
    assert e.value.code == ERR_INVALID
    s.path_record()
    exp.append(_twin_read(t, False))
    for k in (None, 30, 31):
        if k is not None:
            step(s, k)
            exp.append(_twin_read(t, step(t, k)))
        ps = s.path_summary()
        m = path_model.summary(_recs(exp, 30), np.arange(N), exp[-1][3])
        _compare(ps, m, N, "far from the origin, %d fresh records" % (len(exp) - 30))
        assert np.all(m["mu"] > 9e4) and not np.isnan(ps["mean"]).any(), "the weights are degenerate: the case shows nothing"
    _same_records(s, exp, 30, "far from the origin")
    assert m["distinct"][0] < N, "no step at the far state resampled: the lineage is the identity"
    bound = 8.0 * N * U * m["D"] * (m["D"] + m["mu"])
    trace = m["scatter"][:, 0] + m["scatter"][:, 2]
    print("far from the origin: model scatter trace %.3g .. %.3g m^2, bound %.3g .. %.3g m^2, D %.3g .. %.3g m" %
          (trace.min(), trace.max(), bound.min(), bound.max(), m["D"].min(), m["D"].max()))
    assert np.all(trace[-1:] > 10.0 * bound[-1:]), "the case would pass vacuously"
    _same_final(s, t, "far from the origin")
    s.close()
    t.close()


def test_summary_degenerate_weights(sg):
    """weights that sum to zero, or to nothing finite: every double NaN and no error; distinct still exact"""
    N = 1000
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, N, 2, 1)
    s.path_enable(16)
    _run(s, c, 0, 12)
    d = s.download()
    for w in (np.zeros(N, f32), np.where(np.arange(N) == 7, np.inf, d["w"]).astype(f32), np.where(np.arange(N) == 3, np.nan, d["w"]).astype(f32)):
        s.upload(dict(d, w=w))
        s.path_record()
        s.path_record()
        ps = s.path_summary()
        assert len(ps["distinct"]) == 2 and all(np.isnan(ps[q]).all() for q in ("mean", "scatter", "cs")) and np.all(ps["distinct"] == N)
    s.upload(d)
    s.path_record()
    ps = s.path_summary()
    m = path_model.summary([(d["xv"], np.arange(N, dtype=np.int32))], np.arange(N), d["w"])
    _compare(ps, m, N, "after the degenerate uploads")
    s.close()


def test_read_only_and_deterministic(sg, monkeypatch):
    """a context that was fetched, traced and summarised after every batch (the records through the partials' table five at a time, too:
    the same bits) ends in the same bits as one that never was; both record"""
    N = 1000
    c = _course("FASTSLAM2", 100)
    cuts = (0, 12, 24, 31, 45)

    def run(observe):
        s = _known(sg, c, N, 2, 1)
        s.path_enable(64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            _run(s, c, a, b)
            if observe:
                x, y = s.path_summary(), s.path_summary()
                monkeypatch.setenv("SLAMGPU_PATH_CHUNK", "5")
                z = s.path_summary()
                monkeypatch.delenv("SLAMGPU_PATH_CHUNK")
                for q in ("mean", "scatter", "cs", "distinct"):
                    assert _bits(x[q]) == _bits(y[q]), "two summaries of one state differ"
                    assert _bits(x[q]) == _bits(z[q]), "the records in chunks of 5: different bits"
                s.path_fetch(b - 1)
                s.path_trace(-1)
                s.path_trace(N - 1, first=1, count=3)
        recs = [s.path_fetch(r) for r in range(cuts[-1])]
        h, d = s.history_fetch(), s.download()
        s.close()
        return recs, h, d
    (ra, ha, da), (rb, hb, db) = run(True), run(False)
    for (xa, pa), (xb, pb) in zip(ra, rb):
        assert _bits(xa) == _bits(xb) and np.array_equal(pa, pb)
    for x, y in zip(ha, hb):
        assert _bits(np.asarray(x)) == _bits(np.asarray(y))
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert _bits(da[k]) == _bits(db[k]), k


def test_ring(sg):
    """capacity 8, 20 records: the oldest are dropped, never a step refused"""
    N = 1000
    c = _course("FASTSLAM2", 100)
    s, t = _known(sg, c, N, 2, 1), _known(sg, c, N, 2, 1)
    s.path_enable(8)
    _run(s, c, 0, 20)
    exp = _twin_steps(t, c, 0, 20)
    assert s.path_info() == (12, 20, 8)
    _same_records(s, exp, 12, "ring")
    for r in (11, 20, -1):
        with pytest.raises(sg.SlamGpuError) as e:
            s.path_fetch(r)
        assert e.value.code == ERR_INVALID, r
    recs = _recs(exp, 12)
    for i in (0, 400, 999):
        xyt, idx = s.path_trace(i, 12, 8)
        wx, wi = _walk(recs, np.arange(N), i)
        assert _bits(xyt) == _bits(wx) and np.array_equal(idx, wi), i
    ps = s.path_summary()
    _compare(ps, path_model.summary(recs, np.arange(N), exp[-1][3]), N, "ring")
    _same_final(s, t, "ring")
    s.close()
    t.close()


def test_per_particle_maps(sg):
    """update_particle + estimate_async + path_record per step (host-made observations): records equal the twin's; run_particle is
    refused while the path is recorded, applies nothing, and works again after path_enable(0)"""
    N, steps = 512, 40
    c = _course("FASTSLAM2", 60)
    opt = _opt(EXCL_ON, 1, 0.02)
    s, t = _ctx(sg, c, N, 2, 1), _ctx(sg, c, N, 2, 1)
    s.path_enable(64)
    exp = []
    for k in range(steps):
        _pp_step(s, c, k, opt)
        s.path_record()
        # (a step without observations makes no update: its parents are the identity, whatever Ctrl.resampled still says)
        exp.append(_twin_read(t, _pp_step(t, c, k, opt)))
    rs = [e[2] for e in exp]
    assert any(rs) and not all(rs)
    _same_records(s, exp, 0, "per-particle maps")
    before = s.peek()
    with pytest.raises(sg.SlamGpuError) as e:
        s.run_particle(c["ctl"][steps:steps + 4], c["Q"], c["dt"], c["xt"][steps:steps + 4], c["max_range"], c["R"], noise=2, **opt)
    assert e.value.code == ERR_INVALID and "path" in str(e.value)
    after = s.peek()
    for q in ("xv", "Pv", "w", "xf", "Pf"):
        assert _bits(before[q]) == _bits(after[q]), q
    assert s.path_info() == (0, steps, 64)
    s.path_enable(0)
    assert s.path_info() == (0, 0, 0)
    for x in (s, t):
        x.run_particle(c["ctl"][steps:steps + 4], c["Q"], c["dt"], c["xt"][steps:steps + 4], c["max_range"], c["R"], noise=2, **opt)
    _same_final(s, t, "per-particle maps")
    s.close()
    t.close()


def test_errors(sg):
    c = _course("FASTSLAM2", 100)
    N = 512
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    with pytest.raises(sg.SlamGpuError) as e:
        shard.path_enable(8)
    assert e.value.code == ERR_INVALID and "single contexts only" in str(e.value)
    assert shard.path_info() == (0, 0, 0)
    shard.close()
    s = _known(sg, c, N, 2, 1)
    for call in (s.path_record, lambda: s.path_fetch(0), lambda: s.path_trace(0, 0, 0), lambda: s.path_summary(0, 0)):
        with pytest.raises(sg.SlamGpuError) as e:  # recording off
            call()
        assert e.value.code == ERR_INVALID
    with pytest.raises(sg.SlamGpuError) as e:
        s.path_enable(-1)
    assert e.value.code == ERR_INVALID and s.path_info() == (0, 0, 0)
    s.path_enable(16)
    _run(s, c, 0, 10)
    pk0 = s.peek()
    assert len(s.path_trace(0, 10, 0)[1]) == 0 and len(s.path_summary(3, 0)["distinct"]) == 0  # count 0 does nothing
    for first, count in ((-1, 2), (0, -1), (0, 11), (10, 1), (2, 9), (2 ** 40, 1)):
        for call in (lambda: s.path_trace(0, first, count), lambda: s.path_summary(first, count)):
            with pytest.raises(sg.SlamGpuError) as e:
                call()
            assert e.value.code == ERR_INVALID, (first, count)
    for particle in (-2, N, 2 ** 31 - 1):
        with pytest.raises(sg.SlamGpuError) as e:
            s.path_trace(particle)
        assert e.value.code == ERR_INVALID, particle
    # outputs untouched by a refused call
    import ctypes as C
    out, idx, xyt = np.full((4, 7), 3.0), np.full(4, 9, np.int32), np.full((4, 3), 2.0, f32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert s.L.slamgpu_path_summary(s.h, 8, 4, p(out), p(idx)) == ERR_INVALID and np.all(out == 3.0) and np.all(idx == 9)
    assert s.L.slamgpu_path_trace(s.h, N, 0, 4, p(xyt), p(idx)) == ERR_INVALID and np.all(xyt == 2.0) and np.all(idx == 9)
    assert s.L.slamgpu_path_fetch(s.h, 10, p(xyt), p(idx)) == ERR_INVALID and np.all(xyt == 2.0) and np.all(idx == 9)
    pk1 = s.peek()
    for q in ("xv", "Pv", "w", "xf", "Pf"):
        assert _bits(pk0[q]) == _bits(pk1[q]), q
    # a restart drops the records and numbers from 0 again
    s.path_enable(4)
    assert s.path_info() == (0, 0, 4)
    _run(s, c, 10, 12)
    assert s.path_info() == (0, 2, 4)
    s.close()


def test_off_means_off(sg):
    """a context that never enabled recording launches none of the new kernels (and one that did launches every one of them: the names
    asked for are the names used)"""
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, 1000, 2, 1)
    s.profile(True)
    for a in range(0, 50, 10):
        _run(s, c, a, a + 10)
    s.peek()
    for name in KERNELS:
        assert s.kernel_time(name)[1] == 0, name
    assert s.path_info() == (0, 0, 0)
    s.path_enable(8)
    _run(s, c, 50, 55)
    s.path_trace(-1)
    s.path_summary()
    for name in KERNELS:
        assert s.kernel_time(name)[1] > 0, name
    s.close()


def test_slam_backend_path_smoothed():
    """slam-backend -path smoothed, three drivers of the step (run_observe, slamgpu_step, slamgpu_update_particle): the smoothed-path
    line, with everything else the output of the run without it (wall-clock figures aside)"""
    def run(extra):
        r = subprocess.run([EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
                            "-SWITCH_SEED_RANDOM", "7", "-rng", "philox", "-maxsteps", "2000", *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        return [re.sub(r"-?\d+\.\d+ us", "T us", re.sub(r"= \d+ % of", "= T % of", ln)) for ln in r.stdout.splitlines()]
    for drive in (("-observe", "device"), (), ("-assoc", "particle")):
        plain, path = run(drive), run(drive + ("-path", "smoothed", "-PATH_RECORDS", "128"))
        lines = [ln for ln in path if ln.startswith("smoothed path:")]
        assert len(lines) == 1 and [ln for ln in path if not ln.startswith("smoothed path:")] == plain, drive
        m = re.match(r"smoothed path: (\d+) records kept, mean distance to the true path (\d+\.\d+) m \(filtered estimates of the same steps: (\d+\.\d+) m\); "
                     r"distinct ancestors 1 / 10 / 100 records back (\d+) / (\d+) / (\d+), at the oldest record (\d+)$", lines[0])
        assert m, lines[0]
        print("slam-backend %s -path smoothed: %s" % (" ".join(drive), lines[0]))
        kept, back1, back10, back100, oldest = (int(m.group(i)) for i in (1, 4, 5, 6, 7))
        assert kept == 128 and 512 >= back1 >= back10 >= back100 >= oldest >= 1
        assert float(m.group(2)) < 5.0 and float(m.group(3)) < 5.0
