"""Posterior map summary on the device (slamgpu_map_summary): per landmark slot the share of the weight that holds it, the holders'
weighted mean, their scatter and their mean covariance, reduced over ALL particles by map_summary_kernel / map_finish_kernel.

The yardstick is a float64 numpy model evaluated on peek(first=0, stride=1, count=N) of the same context taken immediately before
the call (float32 records and weights promoted to float64, the header's definitions, numpy's pairwise sums).  The tolerances are
rounding bounds: with u = 2^-53, N the particle count and per slot D = the larger coordinate range of the holders' xf, |mu| the larger
coordinate of the model mean, P = max |Pf entry| over the holders: any order of summing n terms in double errs by at most
(n - 1) u sum |t_i|; terms about a pivot inside the cloud are bounded by D and D^2; every merge of two partial means rounds once at
the size of the mean (u |mu|) and carries that into M2 through delta^2, |delta| <= D; no path from a record to an output has more
than N such steps.  With a factor 8 for the division by the weight sum and the final pivot shift:
    share 8 N u | mean 8 N u (D + |mu|) | scatter 8 N u D (D + |mu|) | mean Pf 8 N u P | holders exact | NaN where nobody holds.
Every check prints its worst error / bound ratio before it asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_gpu_particle_assoc import DISCARD, NEW, _predicts, _tape
from test_gpu_particle_device import EXCL_ON, EXE, ERR_INVALID, _course, _ctx, _finish, _opt, _same_state
from test_gpu_particle_lists import _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
_STATE = {}   # the N = 100 000 state of the known-association case, for the far-from-origin case


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _psum(a):
    """sum over the particles (axis 0) of [N, nf], by numpy's pairwise summation (which runs along the contiguous axis)"""
    return np.ascontiguousarray(a.T).sum(axis=1)


def _model(pk, logw):
    w = pk["w"].astype(f64)
    if logw:
        w = np.exp(w - w.max())
    with np.errstate(all="ignore"):
        wh = w / w.sum()
        xf, Pf = pk["xf"].astype(f64), pk["Pf"].astype(f64)
        held = ~np.isnan(xf[:, :, 0])
        W = np.where(held, wh[:, None], 0.0)
        share = _psum(W)
        x, y = np.where(held, xf[:, :, 0], 0.0), np.where(held, xf[:, :, 1], 0.0)
        mean = np.stack([_psum(W * x) / share, _psum(W * y) / share], axis=1)
        dx, dy = np.where(held, x - mean[None, :, 0], 0.0), np.where(held, y - mean[None, :, 1], 0.0)
        scatter = np.stack([_psum(W * dx * dx) / share, _psum(W * dx * dy) / share, _psum(W * dy * dy) / share], axis=1)
        P = [np.where(held, Pf[:, :, a, b], 0.0) for a, b in ((0, 0), (1, 0), (1, 1))]
        pf = np.stack([_psum(W * p) / share for p in P], axis=1)
        holders = held.sum(axis=0).astype(np.int32)
        big = np.where(held, 0.0, -np.inf)
        D = np.maximum((x + big).max(0) - (x - big).min(0), (y + big).max(0) - (y - big).min(0))
        Pmax = np.max([np.abs(p).max(0) for p in P] + [np.abs(np.where(held, Pf[:, :, 0, 1], 0.0)).max(0)], axis=0)
    return dict(share=share, mean=mean, scatter=scatter, pf=pf, holders=holders, D=D, mu=np.abs(mean).max(axis=1), P=Pmax)


def _bounds(m, N):
    k = 8.0 * N * U
    with np.errstate(all="ignore"):
        return dict(share=np.full_like(m["share"], k), mean=k * (m["D"] + m["mu"]), scatter=k * m["D"] * (m["D"] + m["mu"]), pf=k * m["P"])


def _compare(ms, m, N, tag):
    """the summary against the model within the rounding bounds; prints the worst error / bound of each quantity first"""
    b = _bounds(m, N)
    nobody = m["holders"] == 0
    report, bad = [], []
    for q in ("share", "mean", "scatter", "pf"):
        got, exp = ms[q], m[q]
        err = np.abs(got - exp)
        bound = b[q] if got.ndim == 1 else b[q][:, None]
        some = ~np.isnan(exp)
        ratio = np.where(some & (err > 0), err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
        report.append("%s %.3g (err %.3g)" % (q, ratio.max() if ratio.size else 0.0, np.nanmax(err) if some.any() else 0.0))
        if not np.array_equal(np.isnan(got), np.isnan(exp)):
            bad.append(q + ": NaN pattern")
        elif not np.all(err[some] <= np.broadcast_to(bound, err.shape)[some]):
            bad.append(q + ": outside its bound")
    print("map_summary %s: N %d, %d slots, %d unheld; worst error / bound: %s" % (tag, N, len(m["share"]), int(nobody.sum()), ", ".join(report)))
    assert np.array_equal(ms["holders"], m["holders"]), tag
    assert not bad, (tag, bad)
    assert np.all(ms["share"][nobody] == 0.0) and np.isnan(ms["mean"][nobody]).all() and np.isnan(ms["scatter"][nobody]).all() and \
        np.isnan(ms["pf"][nobody]).all(), tag


def _check(s, logw, tag):
    pk = s.peek()
    ms = s.map_summary()
    m = _model(pk, logw)
    _compare(ms, m, s.N, tag)
    return ms, m


def _bits(ms):
    return tuple(np.ascontiguousarray(ms[q]).view(np.uint8).tobytes() for q in ("share", "mean", "scatter", "pf", "holders"))


def _known(sg, c, N, method, math, logw=False, cap=None, device_observe=True):
    s = sg.SlamGpu(N, cap or c["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=math,
                   device_observe=device_observe, log_weights=logw)
    if device_observe:
        s.set_map(c["lm"])
    return s


def _run(s, c, a, b):
    s.run_observe(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2)


def _both_states(s, c, logw, tag, first, last):
    """steps first .. one at a time, a checked summary after each, until one was taken with a lazy gather pending and one with none
    (the history's resampled flag of the step just made); returns the last summary and model"""
    seen = set()
    out = None
    for k in range(first, last):
        _run(s, c, k, k + 1)
        out = _check(s, logw, "%s step %d" % (tag, k))
        seen.add(bool(s.history_fetch()[2][-1]))
        if len(seen) == 2:
            break
    assert seen == {False, True}, "no summary was taken %s a pending gather" % ("without" if True in seen else "with")
    return out


@pytest.mark.parametrize("method,math,N", [(2, 0, 1000), (1, 0, 1000), (2, 1, 1000), (1, 1, 1000), (2, 1, 100000), (1, 0, 100000)])
def test_known_association_compact(sg, method, math, N):
    """example_webmap (compact genealogy), after >= 60 observation steps: the model, every share 1, every particle a holder"""
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 100)
    s = _known(sg, c, N, method, math)
    assert s.genealogy_rows()[1] <= 40, "not the compact layout"
    _run(s, c, 0, 60)
    s.history_fetch()
    ms, m = _both_states(s, c, False, "known compact m%d math%d" % (method, math), 60, 100)
    assert s.nf() >= 3 and len(ms["share"]) == s.nf()
    assert np.all(np.abs(ms["share"] - 1.0) <= 8.0 * N * U) and np.all(ms["holders"] == N)
    if N == 100000 and method == 2:
        _STATE["far"] = s.download()
    s.close()


@pytest.mark.parametrize("N", [4096, 3000])
def test_plain_layout_log_weights(sg, tmp_path_factory, N):
    """a 1 000-landmark map (plain genealogy rows), log-weights, N a multiple of 256 and not: the padding lanes contribute nothing"""
    key = "c1000"
    if key not in _STATE:
        _STATE[key] = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 40)
    c = _STATE[key]
    s = _known(sg, c, N, 2, 1, logw=True)
    assert s.genealogy_rows()[1] > 40, "not the plain layout"
    _run(s, c, 0, 25)
    s.history_fetch()
    ms, m = _both_states(s, c, True, "plain logw N%d" % N, 25, 40)
    assert s.nf() >= 30 and np.all(ms["holders"] == N) and np.all(np.abs(ms["share"] - 1.0) <= 8.0 * N * U)
    s.close()


def test_constructed_labels_shares_of_disjoint_sets(sg):
    """per-particle maps: two disjoint sets of particles open one slot each in one step, nobody else holds them: the shares are the
    sets' shares of the (uneven) weight, the means the holders' only; and a slot whose holders all died in a resample is share 0 /
    NaN / holders 0"""
    N = 1024
    tape = _tape("FASTSLAM2", N, 40)

    def grown(n_effective):
        s = sg.SlamGpu(N, 64, method=2, n_effective=n_effective, rng_mode=sg.RNG_PHILOX, seed=3, math_mode=1, particle_maps=True)
        for st in tape["steps"][:20]:
            _predicts(s, st, tape)
            zf, zn = np.array(st["zf"], f32).reshape(-1, 2), np.array(st["zn"], f32).reshape(-1, 2)
            if len(zf) + len(zn):
                s.update(zf, np.array(st["idf"], np.int32), zn, tape["R"])
        return s
    # (NEFFECTIVE 0: never resamples -- the weights stay uneven and nobody's hypothesis dies)
    s = grown(0)
    nf = s.nf()
    A, B = np.arange(0, 300), np.arange(300, 700)
    z = np.array([[25.0, 0.3], [18.0, -0.6]], f32)
    lab = np.full((N, 2), DISCARD, np.int32)
    lab[A, 0] = NEW
    lab[B, 1] = NEW
    rep = s.update_labels(z, tape["R"], lab, new_share=0.0, p_new=1.0, census_every=1)
    assert rep["opened"] == 2 and rep["slots"] == nf + 2, rep
    pk = s.peek()
    ms, m = _check(s, False, "disjoint sets")
    w = pk["w"].astype(f64)
    wh = w / w.sum()
    assert np.ptp(pk["w"]) > 0, "the weights are even: the shares would be head counts"
    for slot, who in ((nf, A), (nf + 1, B)):
        assert ms["holders"][slot] == len(who) and 0.0 < ms["share"][slot] < 1.0
        assert abs(ms["share"][slot] - wh[who].sum()) <= 8.0 * N * U
        xs = pk["xf"][who, slot].astype(f64)
        assert np.all(ms["mean"][slot] >= xs.min(0)) and np.all(ms["mean"][slot] <= xs.max(0))
        assert np.isnan(pk["xf"][np.setdiff1d(np.arange(N), who), slot, 0]).all()
    assert np.all(ms["holders"][:nf] == N) and np.all(np.abs(ms["share"][:nf] - 1.0) <= 8.0 * N * U)
    s.close()
    # (NEFFECTIVE N: every step resamples) a weightless minority opens a slot and dies in the step's resample: read through the pending gather
    s = grown(N)
    d = s.download()
    nf = d["nf"]
    d["w"] = d["w"].copy()
    d["w"][:10] = 0.0
    d["w"] /= d["w"].sum()
    s.upload(d)
    lab = np.full((N, 1), DISCARD, np.int32)
    lab[:10, 0] = NEW
    rep = s.update_labels(z[:1], tape["R"], lab, new_share=0.0, p_new=1.0, census_every=1)
    assert rep["opened"] == 1 and rep["slots"] == nf + 1, rep
    ms, m = _check(s, False, "dead slot")
    assert s.stats()[1], "the step did not resample: no gather is pending"
    assert ms["holders"][nf] == 0 and ms["share"][nf] == 0.0 and np.isnan(ms["mean"][nf]).all() and np.isnan(ms["scatter"][nf]).all() and \
        np.isnan(ms["pf"][nf]).all()
    assert np.all(ms["holders"][:nf] == N)
    s.close()


def test_whole_run_segment_per_particle(sg):
    """slamgpu_run_particle (exclusion rule on, census every step), 150 steps in calls of 30: the model after every call, and the run
    with summaries in between is the run without them, bit for bit"""
    N, steps, K = 2048, 150, 30
    c = _course("FASTSLAM2", steps)
    opt = _opt(EXCL_ON, 1, 0.02)

    def run(observe):
        d = _ctx(sg, c, N, 2, 1)
        seen = []
        for a in range(0, steps, K):
            d.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], c["xt"][a:a + K], c["max_range"], c["R"], noise=2, **opt)
            if observe:
                ms, m = _check(d, False, "run_particle after %d" % (a + K))
                seen.append(ms)
        rep = d.particle_report_fetch()
        return _finish(d), rep, seen
    with_, rep_w, seen = run(True)
    without, rep_o, _ = run(False)
    _same_state(with_, without, "summaries between the calls")
    assert np.array_equal(rep_w, rep_o)
    resampled = np.asarray(with_[0][2])
    assert len(resampled) == steps
    pending = {bool(resampled[a + K - 1]) for a in range(0, steps, K)}
    print("map_summary run_particle: summaries with a gather pending / without:", sorted(pending),
          "; slots with 0 < share < 1 per summary:", [int(((ms["share"] > 0) & (ms["share"] < 1 - 1e-9)).sum()) for ms in seen])
    assert len(seen) == steps // K and all(len(ms["share"]) >= 1 for ms in seen)


@pytest.mark.parametrize("layout", ["compact", "plain"])
def test_read_only_and_deterministic(sg, tmp_path_factory, monkeypatch, layout):
    """two summaries of one state: the same bits; the slots taken through the partials' table eight at a time (SLAMGPU_MAP_CHUNK, a
    diagnostic: a large map is chunked by the table's size): the same bits; summary, download (materialise + flatten), summary: the
    same bits; and a twin stepped identically without any summary ends in the same state, bit for bit"""
    if layout == "compact":
        c, N, logw = _course("FASTSLAM2", 100), 1000, False
    else:
        if "c1000" not in _STATE:
            _STATE["c1000"] = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 40)
        c, N, logw = _STATE["c1000"], 1280, True
    cuts = (0, 12, 24, 31, 40)

    def run(observe):
        s = _known(sg, c, N, 2, 1, logw=logw)
        assert (s.genealogy_rows()[1] <= 40) == (layout == "compact")
        for a, b in zip(cuts[:-1], cuts[1:]):
            _run(s, c, a, b)
            if observe:
                x, y = s.map_summary(), s.map_summary()
                assert _bits(x) == _bits(y), "two summaries of one state differ"
                monkeypatch.setenv("SLAMGPU_MAP_CHUNK", "8")
                y = s.map_summary()
                monkeypatch.delenv("SLAMGPU_MAP_CHUNK")
                assert _bits(x) == _bits(y), "the slots in chunks of 8: different bits"
        if observe:
            before = s.map_summary()
            d = s.download()
            after = s.map_summary()
            assert _bits(before) == _bits(after), "through the genealogy and flattened: different bits"
            _compare(after, _model(d, logw), N, "%s flattened" % layout)
        return _finish(s)
    _same_state(run(True), run(False), "summaries between the steps (%s)" % layout)


# ---- the shapes at which the code the summaries share can go wrong (test_gpu_map_pairs.py and test_gpu_joint.py use them too) ----------
ODD_N = 9222   # ten tiles of 1 024 particles with six in the last: waves without a particle, and the finishing pass's eight stretches
               # get two tiles each where they get any (three of them get none)
ODD_CASES = [(layout, logw) for layout in ("compact", "plain") for logw in (False, True)]


def _uneven(nf):
    """a number of slots, pairs or observations that is no multiple of the group of 8 and needs a second chunk of 8"""
    count = 11 if nf >= 11 else nf - (nf % 8 == 0)
    assert count > 8, "the map holds %d slots: too few for two chunks of 8" % nf
    return count


def _odd_pending(sg, layout, logw, check):
    """example_webmap (at most 16 slots in use) at ODD_N particles, in compact rows or in plain ones (a capacity past the compact
    layouts'), with linear or log weights: check(s, tag) after every step from 170 on, until one was made straight after an update that
    resampled, with its gather pending and nothing fetched in between"""
    c = _course("FASTSLAM2", 200)
    s = _known(sg, c, ODD_N, 2, 1, logw=logw, cap=None if layout == "compact" else 64)
    assert (s.genealogy_rows()[1] <= 40) == (layout == "compact")
    _run(s, c, 0, 170)
    s.history_fetch()
    for k in range(170, 200):
        _run(s, c, k, k + 1)
        assert s.nf() <= 16
        check(s, "odd tiles %s %s step %d" % (layout, "log" if logw else "linear", k))
        if s.history_fetch()[2][-1]:
            s.close()
            return
    raise AssertionError("no step from 170 on resampled: no call was made with a gather pending")


@pytest.mark.parametrize("layout,logw", ODD_CASES)
def test_odd_tiles_uneven_count(sg, monkeypatch, layout, logw):
    """ODD_N particles, 11 slots through the partials' table 8 at a time, both layouts and both weight forms, a gather pending: the
    model within its bounds, and the bits of the same slots inside the whole map taken in one chunk"""
    def check(s, tag):
        pk = s.peek()
        count = _uneven(s.nf())
        monkeypatch.setenv("SLAMGPU_MAP_CHUNK", "8")
        ms = s.map_summary(0, count)
        monkeypatch.delenv("SLAMGPU_MAP_CHUNK")
        _compare(ms, {q: v[:count] for q, v in _model(pk, logw).items()}, ODD_N, tag)
        whole = s.map_summary()
        assert _bits({q: v[:count] for q, v in whole.items()}) == _bits(ms), "a slot's bits depend on the chunking"
    _odd_pending(sg, layout, logw, check)


def test_far_from_the_origin(sg):
    """the N = 100 000 state of the known-association case with every landmark moved by (1e5, -1e5) m: D stays the cloud's, |mu| is
    1e5.  Raw second moments would cancel ~ sqrt(N) u x^2 = 3e-4 m^2 of noise into a scatter whose bound is ~ 1e-5 m^2"""
    N = 100000
    c = _course("FASTSLAM2", 100)
    if "far" not in _STATE:
        s = _known(sg, c, N, 2, 1)
        _run(s, c, 0, 62)
        _STATE["far"] = s.download()
        s.close()
    d = dict(_STATE["far"])
    d["xf"] = (d["xf"].astype(f64) + np.array([1e5, -1e5])).astype(f32)
    s = _known(sg, c, N, 2, 1, device_observe=False)
    s.upload(d)
    ms, m = _check(s, False, "far from the origin")
    s.close()
    b = _bounds(m, N)
    trace = m["scatter"][:, 0] + m["scatter"][:, 2]
    print("far from the origin: model scatter trace %.3g .. %.3g m^2, bound %.3g .. %.3g m^2, D %.3g .. %.3g m" %
          (trace.min(), trace.max(), b["scatter"].min(), b["scatter"].max(), m["D"].min(), m["D"].max()))
    assert np.all(m["mu"] > 9e4)
    assert np.all(trace > 100.0 * b["scatter"]), "the case would pass vacuously"


def test_windows_and_refusals(sg):
    """first_slot / count windows are the rows of the full call, bit for bit; count 0 does nothing; every refusal returns its code and
    leaves the state alone"""
    c = _course("FASTSLAM2", 150)
    s = _ctx(sg, c, 512, 2, 1)
    s.run_particle(c["ctl"][:40], c["Q"], c["dt"], c["xt"][:40], c["max_range"], c["R"], noise=2, **_opt(EXCL_ON, 1, 0.02))
    nf = s.nf()
    assert nf >= 3
    pk0 = s.peek()
    full = s.map_summary()
    windows = {(first, count) for first in (0, 1, nf // 3, nf - 1) for count in (1, (nf - first + 1) // 2, nf - first)}
    for first, count in sorted(windows):
        win = s.map_summary(first, count)
        for q in ("share", "mean", "scatter", "pf", "holders"):
            assert np.ascontiguousarray(win[q]).tobytes() == np.ascontiguousarray(full[q][first:first + count]).tobytes(), (first, count, q)
    empty = s.map_summary(nf, 0)
    assert all(len(empty[q]) == 0 for q in empty)
    assert len(s.map_summary(0, 0)["share"]) == 0
    for first, count in ((-1, 2), (0, -1), (0, nf + 1), (nf, 1), (2, nf - 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        with pytest.raises(sg.SlamGpuError) as e:
            s.map_summary(first, count)
        assert e.value.code == ERR_INVALID, (first, count)
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    with pytest.raises(sg.SlamGpuError) as e:
        shard.map_summary(0, 0)
    assert e.value.code == ERR_INVALID and "single contexts only" in str(e.value)
    shard.close()
    pk1 = s.peek()
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(pk0[k], pk1[k], equal_nan=True), k
    assert _bits(s.map_summary()) == _bits(full)
    # ... and the run goes on as its twin that was never asked anything
    s.run_particle(c["ctl"][40:60], c["Q"], c["dt"], c["xt"][40:60], c["max_range"], c["R"], noise=2, **_opt(EXCL_ON, 1, 0.02))
    t = _ctx(sg, c, 512, 2, 1)
    for a, b in ((0, 40), (40, 60)):
        t.run_particle(c["ctl"][a:b], c["Q"], c["dt"], c["xt"][a:b], c["max_range"], c["R"], noise=2, **_opt(EXCL_ON, 1, 0.02))
    _same_state(_finish(s), _finish(t), "windows and refusals")


def test_degenerate_weights_give_nan(sg):
    """weights that sum to zero, or to nothing finite: every entry NaN and no error (SLAMGPU_STATUS_DEGENERATE's convention); the
    holders are still counted"""
    c = _course("FASTSLAM2", 100)
    N = 1000
    s = _known(sg, c, N, 2, 1)
    _run(s, c, 0, 20)
    d = s.download()
    for w in (np.zeros(N, f32), np.where(np.arange(N) == 7, np.inf, d["w"]).astype(f32), np.where(np.arange(N) == 3, np.nan, d["w"]).astype(f32)):
        s.upload(dict(d, w=w))
        ms = s.map_summary()
        assert len(ms["share"]) == d["nf"] > 0
        assert all(np.isnan(ms[q]).all() for q in ("share", "mean", "scatter", "pf")) and np.all(ms["holders"] == N)
    s.upload(d)
    _check(s, False, "after the degenerate uploads")
    s.close()


def test_slam_backend_map_posterior(tmp_path):
    """slam-backend -assoc particle -observe device -map posterior: the posterior line; its three slot counts add up to the slots in
    use of the best-particle line; everything else is the output of -map best, which is the output without -map"""
    def run(extra):
        r = subprocess.run([EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
                            "-SWITCH_SEED_RANDOM", "7", "-assoc", "particle", "-observe", "device", "-rng", "philox", "-maxsteps", "3000", *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        # (the lines that quote wall-clock times differ from run to run by their nature)
        return [re.sub(r"-?\d+\.\d+ us", "T us", re.sub(r"= \d+ % of", "= T % of", ln)) for ln in r.stdout.splitlines()]
    plain, best, post = run(()), run(("-map", "best")), run(("-map", "posterior"))
    assert plain == best
    lines = [ln for ln in post if ln.startswith("posterior map:")]
    assert len(lines) == 1 and [ln for ln in post if not ln.startswith("posterior map:")] == best
    assert not any(ln.startswith("posterior map:") for ln in best)
    m = re.match(r"posterior map: (\d+) slots held by at least half of the weight \((\d+) of the 35 true landmarks within 1 m of the mean of one of them, "
                 r"(\d+) of them within 1 m of no true landmark\); (\d+) slots held by less than half, (\d+) by none$", lines[0])
    assert m, lines[0]
    confident, covered, stray, minority, dead = (int(v) for v in m.groups())
    mapline = [ln for ln in post if ln.startswith("landmarks in map:")][0]
    slots = int(re.search(r"(\d+) slots in use by all particles together", mapline).group(1))
    print("slam-backend -map posterior:", lines[0], "|", mapline)
    assert confident + minority + dead == slots and covered <= 35 and stray <= confident
    assert post.index(lines[0]) > post.index(mapline)
