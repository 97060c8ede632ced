"""Joint shares of pairs of landmark slots on the device (slamgpu_map_pairs: map_pairs_kernel + map_finish_kernel): over the particles
that hold BOTH slots of a pair, the share of the weight, the mean of d = xf_a - xf_b, its scatter and the mean of Pf_a + Pf_b.

The yardstick is a float64 numpy model on peek(first=0, stride=1, count=N) of the same context taken immediately before the call.
The bounds are those of test_gpu_map_summary.py, re-derived for d.  d_i is formed in double from two float32 numbers and is exact, so
the argument there carries over with d in the place of xf: with u = 2^-53, N the particle count and per pair D = the larger
coordinate range of d over the joint holders J, |delta| = the larger coordinate of the model's mean separation, P = the largest
|Pf_a entry| + |Pf_b entry| over J (the size of one term of the [6..8] sums): any order of summing n <= N terms in double errs by at
most (n - 1) u sum |t_i|; terms about a pivot inside the cloud of d are bounded by D and D^2 (the one extra rounding of d - pivot is
u D, one more step of the N); every merge of two partial means rounds once at the size of the mean (u |delta|) and carries that into
M2 through the difference of the means, at most D; no path from a record to an output has more than N such steps.  With the factor 8
for the division by the weight sum and the final pivot shift:
    share 8 N u | mean 8 N u (D + |delta|) | scatter 8 N u D (D + |delta|) | [6..8] 8 N u P | both exact | NaN pattern equal.
Every check prints its worst error / bound ratio before it asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_gpu_map_summary import ODD_CASES, ODD_N, _STATE, _known, _odd_pending, _psum, _run
from test_gpu_particle_assoc import DISCARD, NEW, _predicts, _tape
from test_gpu_particle_device import EXCL_ON, EXE, ERR_INVALID, _course, _ctx, _finish, _opt, _same_state
from test_gpu_particle_lists import _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
QS = ("share", "mean", "scatter", "pf")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _all_pairs(slots, ordered=False):
    """every a <= b of the slots (ordered: every (a, b))"""
    slots = list(slots)
    return np.array([(a, b) for i, a in enumerate(slots) for j, b in enumerate(slots) if ordered or i <= j], np.int32).reshape(-1, 2)


def _model(pk, logw, pairs):
    w = pk["w"].astype(f64)
    if logw:
        w = np.exp(w - w.max())
    a, b = pairs[:, 0], pairs[:, 1]
    with np.errstate(all="ignore"):
        wh = w / w.sum()
        xf, Pf = pk["xf"].astype(f64), pk["Pf"].astype(f64)
        held = ~np.isnan(xf[:, :, 0])
        J = held[:, a] & held[:, b]
        W = np.where(J, wh[:, None], 0.0)
        share = _psum(W)
        dx, dy = np.where(J, xf[:, a, 0] - xf[:, b, 0], 0.0), np.where(J, xf[:, a, 1] - xf[:, b, 1], 0.0)
        mean = np.stack([_psum(W * dx) / share, _psum(W * dy) / share], axis=1)
        ex, ey = np.where(J, dx - mean[None, :, 0], 0.0), np.where(J, dy - mean[None, :, 1], 0.0)
        scatter = np.stack([_psum(W * ex * ex) / share, _psum(W * ex * ey) / share, _psum(W * ey * ey) / share], axis=1)
        pf, Pmax = [], np.zeros(len(pairs))
        for i, j in ((0, 0), (1, 0), (1, 1), (0, 1)):
            pa, pb = np.where(J, Pf[:, a, i, j], 0.0), np.where(J, Pf[:, b, i, j], 0.0)
            Pmax = np.maximum(Pmax, (np.abs(pa) + np.abs(pb)).max(0))
            if (i, j) != (0, 1):
                pf.append(_psum(W * (pa + pb)) / share)
        pf = np.stack(pf, axis=1)
        both = J.sum(axis=0).astype(np.int32)
        big = np.where(J, 0.0, -np.inf)
        D = np.maximum((dx + big).max(0) - (dx - big).min(0), (dy + big).max(0) - (dy - big).min(0))
    return dict(share=share, mean=mean, scatter=scatter, pf=pf, both=both, D=D, delta=np.abs(mean).max(axis=1), P=Pmax)


def _bounds(m, N):
    k = 8.0 * N * U
    with np.errstate(all="ignore"):
        return dict(share=np.full_like(m["share"], k), mean=k * (m["D"] + m["delta"]), scatter=k * m["D"] * (m["D"] + m["delta"]), pf=k * m["P"])


def _compare(mp, m, N, tag):
    """the call's answer against the model within the rounding bounds; prints the worst error / bound of each quantity first"""
    b = _bounds(m, N)
    nobody = m["both"] == 0
    report, bad = [], []
    for q in QS:
        got, exp = mp[q], m[q]
        with np.errstate(all="ignore"):
            err = np.abs(got - exp)
        bound = b[q] if got.ndim == 1 else b[q][:, None]
        some = ~np.isnan(exp)
        ratio = np.where(some & (err > 0), err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
        report.append("%s %.3g (err %.3g)" % (q, ratio.max() if ratio.size else 0.0, np.nanmax(err) if some.any() else 0.0))
        if not np.array_equal(np.isnan(got), np.isnan(exp)):
            bad.append(q + ": NaN pattern")
        elif not np.all(err[some] <= np.broadcast_to(bound, err.shape)[some]):
            bad.append(q + ": outside its bound")
    print("map_pairs %s: N %d, %d pairs, %d held together by nobody; worst error / bound: %s" % (tag, N, len(m["share"]), int(nobody.sum()), ", ".join(report)))
    assert np.array_equal(mp["both"], m["both"]), tag
    assert not bad, (tag, bad)
    assert np.all(mp["share"][nobody] == 0.0) and np.isnan(mp["mean"][nobody]).all() and np.isnan(mp["scatter"][nobody]).all() and \
        np.isnan(mp["pf"][nobody]).all(), tag


def _check(s, logw, tag, pairs=None):
    pk = s.peek()
    if pairs is None:
        pairs = _all_pairs(range(s.nf()))
    mp = s.map_pairs(pairs)
    m = _model(pk, logw, pairs)
    _compare(mp, m, s.N, tag)
    return mp, m


def _bits(mp):
    return tuple(np.ascontiguousarray(mp[q]).view(np.uint8).tobytes() for q in QS + ("both",))


def _row_bits(mp, k):
    return tuple(np.ascontiguousarray(mp[q][k]).tobytes() for q in QS + ("both",))


def _both_states(s, c, logw, tag, first, last, pairs_of):
    """steps first .. one at a time, a checked call after each, until one was made with a lazy gather pending and one with none (the
    history's resampled flag of the step just made); returns the last answer and model"""
    seen = set()
    out = None
    for k in range(first, last):
        _run(s, c, k, k + 1)
        out = _check(s, logw, "%s step %d" % (tag, k), pairs_of(s))
        seen.add(bool(s.history_fetch()[2][-1]))
        if len(seen) == 2:
            break
    assert seen == {False, True}, "no call was made %s a pending gather" % ("without" if True in seen else "with")
    return out


@pytest.mark.parametrize("method,math", [(2, 0), (1, 0), (2, 1), (1, 1)])
def test_known_association(sg, method, math):
    """example_webmap after 60 observation steps, N = 1 000, all pairs of the slots in use: the model, every joint share 1, every
    particle holds both; one call with a gather pending, one without"""
    N = 1000
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 100)
    s = _known(sg, c, N, method, math)
    _run(s, c, 0, 60)
    s.history_fetch()
    mp, m = _both_states(s, c, False, "known m%d math%d" % (method, math), 60, 100, lambda s: _all_pairs(range(s.nf())))
    nf = s.nf()
    assert nf >= 3 and len(mp["share"]) == nf * (nf + 1) // 2
    assert np.all(np.abs(mp["share"] - 1.0) <= 8.0 * N * U) and np.all(mp["both"] == N)
    s.close()


def test_tiles_and_tails(sg, tmp_path_factory):
    """N = 9 301: ten tiles of 1 024 particles, the last one partial, more tiles than the finishing pass has stretches; a
    1 000-landmark map (plain genealogy rows: the two slots of a pair lie in different rows), log-weights"""
    N = 9301
    if "c1000" not in _STATE:
        _STATE["c1000"] = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 40)
    c = _STATE["c1000"]
    s = _known(sg, c, N, 2, 1, logw=True)
    assert s.genealogy_rows()[1] > 40, "not the plain layout"
    _run(s, c, 0, 25)
    s.history_fetch()

    def pairs_of(s):
        nf = s.nf()
        pick = sorted(set(np.linspace(0, nf - 1, 9).astype(int).tolist() + [0, 1, nf - 2, nf - 1]))
        return _all_pairs(pick, ordered=True)
    mp, m = _both_states(s, c, True, "plain logw N%d" % N, 25, 40, pairs_of)
    assert s.nf() >= 30 and len(mp["share"]) >= 81 and np.all(mp["both"] == N) and np.all(np.abs(mp["share"] - 1.0) <= 8.0 * N * U)
    s.close()


def _grown(sg, tape, N, n_effective):
    s = sg.SlamGpu(N, 64, method=2, n_effective=n_effective, rng_mode=sg.RNG_PHILOX, seed=3, math_mode=1, particle_maps=True)
    for st in tape["steps"][:20]:
        _predicts(s, st, tape)
        zf, zn = np.array(st["zf"], f32).reshape(-1, 2), np.array(st["zn"], f32).reshape(-1, 2)
        if len(zf) + len(zn):
            s.update(zf, np.array(st["idf"], np.int32), zn, tape["R"])
    return s


def test_constructed_sets(sg):
    """per-particle maps, uneven weights, one update_labels step with two observations: 300 particles open the first slot only, 400
    the second only, 100 both, the rest neither: the joint share of the two new slots is the 100's share of the weight; with nobody in
    both sets it is exactly 0; and a new slot paired with a slot everybody holds has the new slot's own share"""
    N = 1024
    tape = _tape("FASTSLAM2", N, 40)
    z = np.array([[25.0, 0.3], [18.0, -0.6]], f32)
    A, B, Cs = np.arange(0, 300), np.arange(300, 700), np.arange(700, 800)
    for with_c in (True, False):
        s = _grown(sg, tape, N, 0)   # (NEFFECTIVE 0: never resamples -- the weights stay uneven and nobody's hypothesis dies)
        nf = s.nf()
        lab = np.full((N, 2), DISCARD, np.int32)
        lab[A, 0] = NEW
        lab[B, 1] = NEW
        if with_c:
            lab[Cs, 0] = NEW
            lab[Cs, 1] = NEW
        rep = s.update_labels(z, tape["R"], lab, new_share=0.0, p_new=1.0, census_every=1)
        assert rep["opened"] == 2 and rep["slots"] == nf + 2, rep
        pk = s.peek()
        assert np.ptp(pk["w"]) > 0, "the weights are even: the shares would be head counts"
        wh = pk["w"].astype(f64) / pk["w"].astype(f64).sum()
        pairs = np.concatenate([[(nf, nf + 1), (nf + 1, nf)], _all_pairs(range(nf + 2))]).astype(np.int32)
        mp, m = _check(s, False, "constructed sets, %s" % ("100 in both" if with_c else "nobody in both"), pairs)
        ms = s.map_summary()
        assert np.all(ms["holders"][:nf] == N)
        # the pair of the two new slots stands first in the list and again among all pairs: the same bits in both places
        again = 2 + int(np.flatnonzero((pairs[2:, 0] == nf) & (pairs[2:, 1] == nf + 1))[0])
        assert _row_bits(mp, 0) == _row_bits(mp, again)
        if with_c:
            assert mp["both"][0] == 100 and mp["both"][1] == 100
            assert abs(mp["share"][0] - wh[Cs].sum()) <= 8.0 * N * U and 0.0 < mp["share"][0] < ms["share"][nf]
            d = pk["xf"][Cs, nf].astype(f64) - pk["xf"][Cs, nf + 1].astype(f64)
            assert np.all(mp["mean"][0] >= d.min(0)) and np.all(mp["mean"][0] <= d.max(0))
            assert np.all(-mp["mean"][1] >= d.min(0)) and np.all(-mp["mean"][1] <= d.max(0))
            assert ms["holders"][nf] == 400 and ms["holders"][nf + 1] == 500
        else:
            for k in (0, 1):
                assert mp["share"][k] == 0.0 and mp["both"][k] == 0
                assert np.isnan(mp["mean"][k]).all() and np.isnan(mp["scatter"][k]).all() and np.isnan(mp["pf"][k]).all()
            assert ms["holders"][nf] == 300 and ms["holders"][nf + 1] == 400
        # a new slot with an old one: whoever holds the new one holds the old one too
        for new in (nf, nf + 1):
            k = int(np.flatnonzero((pairs[:, 0] == 0) & (pairs[:, 1] == new))[0])
            assert mp["both"][k] == ms["holders"][new] and abs(mp["share"][k] - ms["share"][new]) <= 8.0 * N * U
        s.close()


def _pp_state(sg, N=1000, steps=40):
    c = _course("FASTSLAM2", 150)
    s = _ctx(sg, c, N, 2, 1)
    s.run_particle(c["ctl"][:steps], c["Q"], c["dt"], c["xt"][:steps], c["max_range"], c["R"], noise=2, **_opt(EXCL_ON, 1, 0.02))
    return s


def test_a_slot_with_itself(sg):
    """a == b: the summary's slot with d = 0"""
    s = _pp_state(sg)
    N, nf = s.N, s.nf()
    assert nf >= 3
    pairs = np.stack([np.arange(nf), np.arange(nf)], axis=1).astype(np.int32)
    pk = s.peek()
    ms = s.map_summary()
    mp = s.map_pairs(pairs)
    m = _model(pk, False, pairs)
    _compare(mp, m, N, "a == b")
    held = ms["holders"] > 0
    assert held.sum() >= 3 and np.array_equal(mp["both"], ms["holders"])
    assert np.all(np.abs(mp["share"] - ms["share"]) <= 8.0 * N * U)
    assert np.all(mp["mean"][held] == 0.0) and np.all(mp["scatter"][held] == 0.0)
    err = np.abs(mp["pf"][held] - 2.0 * ms["pf"][held])
    bound = (8.0 * N * U * m["P"][held])[:, None]
    print("map_pairs a == b: %d slots, %d held; [6..8] against twice the summary's mean Pf, worst error / bound %.3g" %
          (nf, int(held.sum()), float((err / bound).max())))
    assert np.all(err <= bound)
    s.close()


def test_per_particle_run(sg):
    """slamgpu_run_particle, 60 steps in calls of 30, all pairs after each call: the model, and the run with the calls in between is
    the run without them, bit for bit"""
    N, steps, K = 2048, 60, 30
    c = _course("FASTSLAM2", steps)
    opt = _opt(EXCL_ON, 1, 0.02)

    def run(observe):
        d = _ctx(sg, c, N, 2, 1)
        seen = []
        for a in range(0, steps, K):
            d.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], c["xt"][a:a + K], c["max_range"], c["R"], noise=2, **opt)
            if observe:
                seen.append(_check(d, False, "run_particle after %d" % (a + K))[0])
        rep = d.particle_report_fetch()
        return _finish(d), rep, seen
    with_, rep_w, seen = run(True)
    without, rep_o, _ = run(False)
    _same_state(with_, without, "joint shares between the calls")
    assert np.array_equal(rep_w, rep_o)
    print("map_pairs run_particle: pairs per call", [len(mp["share"]) for mp in seen], "; pairs with 0 < joint share < 1 per call:",
          [int(((mp["share"] > 0) & (mp["share"] < 1 - 1e-9)).sum()) for mp in seen])
    assert len(seen) == steps // K and all(len(mp["share"]) >= 6 for mp in seen)


def test_deterministic_and_independent_of_position(sg, monkeypatch):
    """one state, at least 20 pairs: two calls, the list shuffled, the list cut into chunks of 8 (SLAMGPU_MAP_CHUNK, in a fresh
    context of the same run), and after download() has flattened the genealogy: the same bits pair by pair"""
    s = _pp_state(sg)
    nf = s.nf()
    pairs = _all_pairs(range(nf), ordered=True)
    assert len(pairs) >= 20 and nf >= 3
    x, y = s.map_pairs(pairs), s.map_pairs(pairs)
    assert _bits(x) == _bits(y), "two calls on one state differ"
    perm = np.random.default_rng(4).permutation(len(pairs))
    z = s.map_pairs(pairs[perm])
    for k, src in enumerate(perm):
        assert _row_bits(z, k) == _row_bits(x, src), ("shuffled", k, src)
    # a pair alone, and twice in one list
    for k in (0, len(pairs) // 2, len(pairs) - 1):
        one = s.map_pairs(pairs[[k, k]])
        assert _row_bits(one, 0) == _row_bits(x, k) and _row_bits(one, 1) == _row_bits(x, k), ("alone", k)
    t = _pp_state(sg)
    monkeypatch.setenv("SLAMGPU_MAP_CHUNK", "8")
    y = t.map_pairs(pairs)
    monkeypatch.delenv("SLAMGPU_MAP_CHUNK")
    t.close()
    assert _bits(x) == _bits(y), "the pairs in chunks of 8: different bits"
    d = s.download()
    y = s.map_pairs(pairs)
    assert _bits(x) == _bits(y), "through the genealogy and flattened: different bits"
    _compare(y, _model(d, False, pairs), s.N, "flattened")
    s.close()


@pytest.mark.parametrize("layout,logw", ODD_CASES)
def test_odd_tiles_uneven_count(sg, monkeypatch, layout, logw):
    """test_gpu_map_summary's shapes: ODD_N particles (a last tile of six), 11 pairs through the partials' table 8 at a time, both
    layouts and both weight forms, a gather pending: the model within its bounds, and the bits of the same list in one chunk"""
    def check(s, tag):
        pairs = _all_pairs(range(s.nf()))[4:15]
        assert len(pairs) == 11 and s.N == ODD_N
        monkeypatch.setenv("SLAMGPU_MAP_CHUNK", "8")
        mp, m = _check(s, logw, tag, pairs)
        monkeypatch.delenv("SLAMGPU_MAP_CHUNK")
        assert _bits(s.map_pairs(pairs)) == _bits(mp), "a pair's bits depend on the chunking"
    _odd_pending(sg, layout, logw, check)


def test_degenerate_weights_give_nan(sg):
    """weights that sum to zero, or to nothing finite: every double NaN and no error; `both` is still counted"""
    c = _course("FASTSLAM2", 100)
    N = 1000
    s = _known(sg, c, N, 2, 1)
    _run(s, c, 0, 20)
    d = s.download()
    pairs = _all_pairs(range(d["nf"]))
    assert len(pairs) >= 3
    for w in (np.zeros(N, f32), np.where(np.arange(N) == 7, np.inf, d["w"]).astype(f32), np.where(np.arange(N) == 3, np.nan, d["w"]).astype(f32)):
        s.upload(dict(d, w=w))
        mp = s.map_pairs(pairs)
        assert all(np.isnan(mp[q]).all() for q in QS) and np.all(mp["both"] == N)
    s.upload(d)
    _check(s, False, "after the degenerate uploads")
    s.close()


def test_refusals_leave_the_outputs_alone(sg):
    import ctypes as C
    s = _pp_state(sg, 512)
    nf = s.nf()
    assert nf >= 2
    L = s.L

    def raw(ctx, pairs, count, null_pairs=False, null_out=False):
        pairs = np.ascontiguousarray(pairs, np.int32)
        out, both = np.full((4, 9), -7.25), np.full(4, -77, np.int32)
        rc = L.slamgpu_map_pairs(ctx.h, None if null_pairs else pairs.ctypes.data_as(C.c_void_p), count,
                                 None if null_out else out.ctypes.data_as(C.c_void_p), both.ctypes.data_as(C.c_void_p))
        assert np.all(out == -7.25) and np.all(both == -77), "a refused call wrote to its outputs"
        return rc
    pk0 = s.peek()
    full = s.map_pairs(_all_pairs(range(nf)))
    assert raw(s, [[0, -1], [0, 1]], 2) == ERR_INVALID
    assert raw(s, [[0, 1], [nf, 0]], 2) == ERR_INVALID
    assert raw(s, [[0, 1]], -1) == ERR_INVALID
    assert raw(s, [[0, 1]], 1, null_pairs=True) == ERR_INVALID
    assert raw(s, [[0, 1]], 1, null_out=True) == ERR_INVALID
    assert raw(s, [[0, 1]], 0) == 0 and raw(s, [[0, 1]], 0, null_pairs=True, null_out=True) == 0
    with pytest.raises(sg.SlamGpuError) as e:
        s.map_pairs([[0, nf]])
    assert e.value.code == ERR_INVALID
    empty = s.map_pairs(np.zeros((0, 2), np.int32))
    assert all(len(empty[q]) == 0 for q in empty)
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    assert raw(shard, [[0, 0]], 1) == ERR_INVALID
    with pytest.raises(sg.SlamGpuError) as e:
        shard.map_pairs([[0, 0]])
    assert e.value.code == ERR_INVALID and "single contexts only" in str(e.value)
    shard.close()
    pk1 = s.peek()
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(pk0[k], pk1[k], equal_nan=True), k
    assert _bits(s.map_pairs(_all_pairs(range(nf)))) == _bits(full)
    s.close()


_RUNS = {}
POSTERIOR = (r"posterior map: (\d+) slots held by at least half of the weight \((\d+) of the 35 true landmarks within 1 m of the mean of one of them, "
             r"(\d+) of them within 1 m of no true landmark\); (\d+) slots held by less than half, (\d+) by none$")
MERGED = (r"merged map: (\d+) landmarks held by at least half of the weight \((\d+) of the 35 true landmarks within 1 m of one of them, (\d+) of them within 1 m "
          r"of no true landmark\); (\d+) clusters of more than one slot; largest joint share of the (\d+) candidate pairs (\d+\.\d+) "
          r"\(radius 1 m, cohold 0\.1\)$")


def _backend(*extra):
    if extra not in _RUNS:
        _RUNS[extra] = subprocess.run([EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
                                       "-SWITCH_SEED_RANDOM", "7", "-rng", "philox", "-maxsteps", "3000", *extra], capture_output=True, text=True, timeout=600)
    return _RUNS[extra]


def _lines(r, start):
    return [ln for ln in r.stdout.splitlines() if ln.startswith(start)]


def test_slam_backend_map_merged_known_association():
    """-map merged with the known association: the posterior line of a -map posterior run, then the merged line: as many landmarks as
    confident slots, no cluster of more than one slot"""
    post, mer = _backend("-map", "posterior"), _backend("-map", "merged")
    assert post.returncode == 0 and mer.returncode == 0, mer.stdout[-800:] + mer.stderr[-800:]
    pl, ml = _lines(mer, "posterior map:"), _lines(mer, "merged map:")
    assert len(pl) == 1 and len(ml) == 1 and pl == _lines(post, "posterior map:") and not _lines(post, "merged map:")
    out = mer.stdout.splitlines()
    assert out.index(ml[0]) == out.index(pl[0]) + 1
    p, m = re.match(POSTERIOR, pl[0]), re.match(MERGED, ml[0])
    assert p and m, (pl[0], ml[0])
    print("slam-backend -map merged, known association:", pl[0], "|", ml[0])
    assert int(m.group(1)) == int(p.group(1)) and int(m.group(4)) == 0
    assert int(m.group(2)) == int(p.group(2)) and int(m.group(3)) == int(p.group(3))


def test_slam_backend_map_merged_per_particle():
    """-assoc particle -observe device -map merged: the line parses, and merging never makes landmarks"""
    r = _backend("-assoc", "particle", "-observe", "device", "-map", "merged")
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    pl, ml = _lines(r, "posterior map:"), _lines(r, "merged map:")
    assert len(pl) == 1 and len(ml) == 1
    p, m = re.match(POSTERIOR, pl[0]), re.match(MERGED, ml[0])
    assert p and m, (pl[0], ml[0])
    print("slam-backend -map merged, per-particle association:", pl[0], "|", ml[0])
    confident, covered, stray, minority, dead = (int(v) for v in p.groups())
    assert int(m.group(1)) <= confident + minority
    assert int(m.group(2)) <= 35 and int(m.group(3)) <= int(m.group(1)) and 0.0 <= float(m.group(6)) <= 1.0 + 1e-6


def test_slam_backend_log_weights():
    """-LOG_WEIGHTS 1: the run keeps log-weights, maps the same landmarks, and the posterior line is there"""
    lin, log = _backend("-map", "merged"), _backend("-map", "merged", "-LOG_WEIGHTS", "1")
    assert lin.returncode == 0 and log.returncode == 0, log.stdout[-800:] + log.stderr[-800:]
    a, b = _lines(lin, "landmarks in map:"), _lines(log, "landmarks in map:")
    assert len(a) == 1 and a == b
    pl = _lines(log, "posterior map:")
    assert len(pl) == 1 and re.match(POSTERIOR, pl[0]) and "not available" not in pl[0]
    assert len(_lines(log, "merged map:")) == 1


def test_slam_backend_refuses_merged_and_log_weights_with_gpus():
    for extra, word in ((("-map", "merged", "-gpus", "2"), "-map merged"), (("-LOG_WEIGHTS", "1", "-gpus", "2"), "-LOG_WEIGHTS")):
        r = _backend(*extra)
        assert r.returncode != 0 and word in r.stderr and "single GPU only" in r.stderr, (extra, r.stderr[-400:])
        assert "particles over" not in r.stdout, "the distributed run had begun"
