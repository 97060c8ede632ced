"""The joint posterior on the device (slamgpu_joint_summary: joint_hold / joint_pivot / joint_gram / joint_reduce / joint_finish): over
the particles J that hold EVERY listed slot, the share of the weight, the mean and the between-particle scatter of
v = (x, y, u, xf_s0, xf_s1, ...) and the mean Pv / Pf.

The yardstick is the float64 numpy model of tests/joint_model.py on peek(first=0, stride=1, count=N) of the same context taken
immediately before the call.  The bounds are derived as in test_gpu_map_pairs.py, for the implementation as built.  With u = 2^-53,
N the particle count, per column a: D_a the coordinate's range over J and |mu_a| the model's mean; P the largest |Pv| / |Pf| entry
over J.  Every d = v - p is formed in double from float32 numbers about ONE pivot p inside the cloud of J (exact for x, y, xf; one
rounding u D_a for the heading's deviation), so |d_a| <= D_a.  The matrix instruction's A operand w d_a rounds once (u w D_a); its
products and sums over n <= N particles, in whatever order the instruction, the sub-tiles and the tiles take them, err by at most
(n + 1) u sum_i w_i |d_a d_b| <= (N + 1) u D_a D_b sum w: the merges of partials are plain additions of such sums, no Chan updates.
The finishing pass divides by s (one rounding each) and subtracts delta_a delta_b, |delta_a| <= D_a: three more roundings of size
u D_a D_b.  The column of ones carries sum w d and sum w through the same products (w d_a 1, w 1 1: exact), so delta_a errs by
(N + 1) u D_a and mu_a = p_a + delta_a rounds once more at the size of the mean.  The weights sum to at most 1 after the division
by the sum of all weights, itself within N u.  The model's own pairwise sums err by less than the same terms.  With the project's
factor 8 for the divisions, the model and the final shifts:
    share 8 N u | mean 8 N u (D_a + |mu_a|) | scatter (a, b) 8 N u D_a D_b | mean Pv / Pf 8 N u P | both exact | NaN pattern equal.
A bound of 0 (N = 1, or a coordinate that is the same in every particle) asks for the exact value.  On exact data -- dyadic
numbers, equal weights, a power of two of them -- every sum is exact in double and the answer must EQUAL the model's bits: the
check that a wrong lane map of the matrix instruction cannot pass.  Every check prints its worst error / bound ratio before it
asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

import joint_model as jm
import pose_model
from conftest import DATA
from test_gpu_map_pairs import _grown, _pp_state
from test_gpu_map_pairs import _bounds as _pair_bounds, _model as _pair_model
from test_gpu_map_summary import ODD_CASES, ODD_N, _STATE, _known, _odd_pending, _run, _uneven
from test_gpu_map_summary import _bounds as _map_bounds, _model as _map_model
from test_gpu_particle_assoc import DISCARD, NEW, _tape
from test_gpu_particle_device import EXCL_ON, EXE, ERR_INVALID, _course, _ctx, _finish, _opt, _same_state
from test_gpu_particle_lists import _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = jm.U
WORST = {}   # the worst error / bound ratio of each quantity over the module's checks, printed by the last test


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _note(ratios):
    for q, r in ratios.items():
        WORST[q] = max(WORST.get(q, 0.0), r)


def _check(s, logw, slots, tag):
    pk = s.peek()
    got = s.joint_summary(slots)
    m = jm.model(pk, logw, slots)
    _note(jm.compare(got, m, s.N, tag))
    if m["both"] == 0:
        assert got["share"] == 0.0 and np.isnan(got["raw"][1:]).all(), tag
    return got, m, pk


def _bits(got):
    return got["raw"].tobytes() + np.int32(got["both"]).tobytes()


def _uploaded(sg, N, nf, math=1, logw=False, seed=3, exact=False, particle_maps=False):
    """a set built by hand and uploaded.  exact: small integers, headings multiples of 1/4 inside (-1, 1), dyadic Pv / Pf, equal
    weights; else a 2 m cloud of poses, 1 m clouds of landmarks, uneven weights with zeros"""
    rng = np.random.default_rng(seed + 7 * N + nf)
    s = sg.SlamGpu(N, max(nf, 4), method=2, rng_mode=sg.RNG_PHILOX, seed=2, math_mode=math, log_weights=logw, particle_maps=particle_maps)
    d = s.download()
    if exact:
        xv = np.stack([rng.integers(-8, 9, N), rng.integers(-8, 9, N), rng.integers(-3, 4, N) / 4.0], axis=1)
        xf = rng.integers(-50, 51, (N, nf, 2)).astype(f64)
        A, Bm = rng.integers(-2, 3, (N, 3, 3)) / 4.0, rng.integers(-2, 3, (N, nf, 2, 2)) / 2.0
        w = np.full(N, 1.0 / N)
    else:
        xv = np.stack([12.0 + rng.normal(0, 2, N), -7.0 + rng.normal(0, 2, N), rng.normal(3.0, 0.3, N)], axis=1)   # (headings about 3: some wrap)
        centre = rng.uniform(-100, 100, (1, nf, 2))
        xf = centre + rng.normal(0, 1, (N, nf, 2)) + 0.3 * xv[:, None, :2]   # (correlated with the pose)
        A, Bm = rng.normal(0, 0.2, (N, 3, 3)), rng.normal(0, 0.3, (N, nf, 2, 2))
        if logw:
            w = rng.normal(-700.0, 1.5, N) + np.where(np.arange(N) < 1024, 0.0, -3.0)   # (the tiles' maxima differ)
        else:
            w = rng.uniform(0.0, 1.0, N)
            if N > 2:
                w[1::5] = 0.0
    d.update(nf=nf, xv=xv.astype(f32), Pv=(A @ A.transpose(0, 2, 1)).astype(f32), w=w.astype(f32), xf=xf.astype(f32),
             Pf=(Bm @ Bm.transpose(0, 1, 3, 2)).astype(f32))
    s.upload(d)
    return s, d


# ---- exact data: the bits of the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_exact_data_equals_the_model(sg, N, mm):
    s, d = _uploaded(sg, N, 7, math=mm, exact=True)
    slots = np.arange(7)
    pk = s.peek()
    assert np.array_equal(pk["xf"], d["xf"]) and np.array_equal(pk["w"], d["w"]) and float(pk["w"][0]) * N == 1.0
    got, m = s.joint_summary(slots), jm.model(pk, False, slots)
    D = 17
    assert got["both"] == N and got["share"] == 1.0 == m["share"]
    wrong = [q for q in ("mean", "scatter", "pv", "pf") if not np.array_equal(got[q], m[q])]
    print("joint_summary exact data N %d: fields that differ from the model's bits: %s; largest |scatter| %.6g" % (N, wrong or "none", np.abs(m["scatter"]).max()))
    assert not wrong, wrong
    assert np.array_equal(got["raw"][1 + D:1 + D + D * (D + 1) // 2], m["scatter"][np.tril_indices(D)])
    assert np.abs(m["scatter"][:3, 3:]).max() > 0 and np.abs(np.diag(m["scatter"])).min() > 0   # (nothing trivially zero)
    # a permutation of the slots permutes the answer (exactly, on exact data)
    perm = np.array([4, 0, 6, 2, 1, 5, 3])
    gp = s.joint_summary(slots[perm])
    idx = np.concatenate([[0, 1, 2], np.stack([3 + 2 * perm, 4 + 2 * perm], axis=1).reshape(-1)])
    assert np.array_equal(gp["mean"], got["mean"][idx]) and np.array_equal(gp["scatter"], got["scatter"][np.ix_(idx, idx)])
    assert np.array_equal(gp["pf"], got["pf"][perm])
    s.close()


def test_plain_fma_form_of_the_gram_pass(sg, monkeypatch):
    """SLAMGPU_JOINT_PLAIN_FMA=1 (the diagnostic form tools/joint_probe.py times beside the matrix instruction): the model's bits on
    exact data, the bounds elsewhere"""
    monkeypatch.setenv("SLAMGPU_JOINT_PLAIN_FMA", "1")
    s, d = _uploaded(sg, 1024, 7, exact=True)
    got, m = s.joint_summary(np.arange(7)), jm.model(s.peek(), False, np.arange(7))
    assert all(np.array_equal(got[q], m[q]) for q in ("mean", "scatter", "pv", "pf")) and got["share"] == 1.0
    s.close()
    s, d = _uploaded(sg, 3000, 18)
    _check(s, False, np.arange(18), "plain FMA form, uploaded k 18")
    s.close()


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N", [(0, 1), (0, 1025), (1, 3), (6, 255), (7, 1025), (8, 3000), (14, 255), (15, 1025), (126, 3), (126, 3000), (40, 1)])
def test_shapes_uploaded(sg, k, N):
    """D = 3, 5, 15, 17, 19, 31, 33, 255 (one column short of, at and past a block of 16; the widest), N = one particle, less than a
    sub-tile, a workgroup less one, a tile plus one, three tiles with a tail; uneven weights with zeros"""
    nf = max(k, 1) + 2
    s, d = _uploaded(sg, N, nf)
    slots = (np.arange(k) * 7) % nf if k else np.zeros(0, np.int32)
    got, m, pk = _check(s, False, slots, "uploaded k %d" % k)
    assert got["both"] == N and got["mean"].shape == (3 + 2 * k,)
    if N == 1:
        assert np.all(got["scatter"] == 0.0) and got["share"] == 1.0 and np.array_equal(got["mean"][:2], d["xv"][0, :2].astype(f64))
    s.close()


@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_shapes_log_weights(sg, mm):
    """log-weights near -700 whose tile maxima differ, three tiles"""
    s, d = _uploaded(sg, 3000, 10, math=mm, logw=True)
    _check(s, True, np.arange(10), "uploaded logw math%d" % mm)
    _check(s, True, [], "uploaded logw math%d k 0" % mm)
    s.close()


def _both_states(s, c, logw, tag, first, last, slots_of):
    """steps first .. one at a time, a checked call after each, until one was made with a lazy gather pending and one with none (the
    history's resampled flag of the step just made); each time the bits must equal those after download() has settled the state"""
    seen = set()
    out = None
    for k in range(first, last):
        _run(s, c, k, k + 1)
        slots = slots_of(s)
        out = _check(s, logw, slots, "%s step %d" % (tag, k))
        pending = bool(s.history_fetch()[2][-1])
        if pending not in seen:
            s.download()
            again = s.joint_summary(slots)
            assert _bits(again) == _bits(out[0]), "%s: %s a pending gather and after download(): different bits" % (tag, "under" if pending else "without")
        seen.add(pending)
        if len(seen) == 2:
            break
    assert seen == {False, True}, "no call was made %s a pending gather" % ("without" if True in seen else "with")
    return out


@pytest.mark.parametrize("method,math,logw", [(2, 0, False), (1, 0, False), (2, 1, True), (1, 1, False)])
def test_known_association_both_states(sg, method, math, logw):
    """example_webmap after 60 observation steps, N = 1 000, all slots in use: the model; every particle holds everything; one call
    with a gather pending, one without, each equal in bits to the call after download()"""
    N = 1000
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", 100)
    s = _known(sg, c, N, method, math, logw=logw)
    _run(s, c, 0, 60)
    s.history_fetch()
    got, m, pk = _both_states(s, c, logw, "known m%d math%d logw%d" % (method, math, logw), 60, 100, lambda s: np.arange(s.nf()))
    assert s.nf() >= 3 and got["both"] == N and abs(got["share"] - 1.0) <= 8.0 * N * U
    s.close()


def test_wide_list_on_a_synthetic_map(sg, tmp_path_factory):
    """a 1 000-landmark map (plain genealogy rows), log-weights, N = 3 000, more than 35 slots listed (as many as are in use, 126 at
    the most): several groups of block pairs per tile"""
    N = 3000
    if "c1000" not in _STATE:
        _STATE["c1000"] = _course_of(_synthetic(tmp_path_factory, 1000), "FASTSLAM2", 40)
    c = _STATE["c1000"]
    s = _known(sg, c, N, 2, 1, logw=True)
    assert s.genealogy_rows()[1] > 40, "not the plain layout"
    _run(s, c, 0, 30)
    s.history_fetch()
    got, m, pk = _both_states(s, c, True, "plain logw N%d" % N, 30, 40, lambda s: np.arange(min(s.nf(), 126)))
    assert len(got["pf"]) > 35 and got["both"] == N
    s.close()


# ---- agreement with the marginals ------------------------------------------------------------------------------------------------------
def test_agrees_with_the_marginal_summaries(sg):
    """k = 0 against pose_summary; the diagonal blocks, means and mean Pf against map_summary; block (a, a) + (b, b) - (a, b) - (a, b)^T
    against map_pairs' scatter: each within the sum of both calls' bounds"""
    N = 1000
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, N, 2, 1)
    _run(s, c, 0, 70)
    pk = s.peek()
    nf = s.nf()
    assert nf >= 4
    # the pose
    j0, m0 = s.joint_summary([]), jm.model(pk, False, [])
    ps = s.pose_summary()
    pb = pose_model.bounds(pk["xv"], pk["Pv"], pose_model.summary(pk["xv"], pk["Pv"], pk["w"], False))
    jb = jm.bounds(m0, N)
    tri = j0["scatter"][np.tril_indices(3)]   # xx, xy, yy, xu, yu, uu
    pairs = [("mean", j0["mean"], ps[1:4], jb["mean"] + pb[1:4]), ("scatter", tri, ps[6:12], jb["scatter"][np.tril_indices(3)] + pb[6:12]),
             ("pv", j0["pv"], ps[12:18], jb["pv"] + pb[12:18])]
    for name, a, b, bound in pairs:
        err = np.abs(a - b)
        print("joint_summary k = 0 against pose_summary, %s: worst error / bound %.3g" % (name, float((err / np.where(bound > 0, bound, 1)).max())))
        assert np.all(err <= bound), name
    # the slots
    slots = np.arange(nf)
    j, m = s.joint_summary(slots), jm.model(pk, False, slots)
    jb = jm.bounds(m, N)
    ms, mm = s.map_summary(), _map_model(pk, False)
    mb = _map_bounds(mm, N)
    assert np.all(ms["holders"] == N) and j["both"] == N
    for a in range(nf):
        r = 3 + 2 * a
        blk, bb = j["scatter"][r:r + 2, r:r + 2], jb["scatter"][r:r + 2, r:r + 2]
        assert np.all(np.abs(j["mean"][r:r + 2] - ms["mean"][a]) <= jb["mean"][r:r + 2] + mb["mean"][a]), a
        assert np.all(np.abs(np.array([blk[0, 0], blk[1, 0], blk[1, 1]]) - ms["scatter"][a]) <= np.array([bb[0, 0], bb[1, 0], bb[1, 1]]) + mb["scatter"][a]), a
        assert np.all(np.abs(j["pf"][a] - ms["pf"][a]) <= jb["pf"][a] + mb["pf"][a]), a
    # the pairs
    pr = np.array([(a, b) for a in range(nf) for b in range(a + 1, nf)], np.int32)
    mp, pm = s.map_pairs(pr), _pair_model(pk, False, pr)
    pbnd = _pair_bounds(pm, N)["scatter"]
    worst = 0.0
    for q, (a, b) in enumerate(pr):
        ra, rb = 3 + 2 * a, 3 + 2 * b
        Sc, Bd = j["scatter"], jb["scatter"]
        comb = Sc[ra:ra + 2, ra:ra + 2] + Sc[rb:rb + 2, rb:rb + 2] - Sc[ra:ra + 2, rb:rb + 2] - Sc[ra:ra + 2, rb:rb + 2].T
        cbnd = Bd[ra:ra + 2, ra:ra + 2] + Bd[rb:rb + 2, rb:rb + 2] + Bd[ra:ra + 2, rb:rb + 2] + Bd[ra:ra + 2, rb:rb + 2].T
        err = np.abs(np.array([comb[0, 0], comb[1, 0], comb[1, 1]]) - mp["scatter"][q])
        bound = np.array([cbnd[0, 0], cbnd[1, 0], cbnd[1, 1]]) + pbnd[q]
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (a, b)
    print("joint_summary against map_pairs' scatter, %d pairs: worst error / bound %.3g" % (len(pr), worst))
    s.close()


# ---- partial holding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_c", [True, False], ids=["100 hold both", "nobody holds both"])
def test_partial_holding(sg, with_c):
    """per-particle maps, uneven weights, one update_labels step with two observations: 300 particles open the first new slot only,
    400 the second only, 100 both (or none): J of (old, new, new) is those 100 -- a strict subset, share < 1 -- or empty; a repeated
    slot repeats its rows and columns; retired slots are reported like any other"""
    N = 1024
    tape = _tape("FASTSLAM2", N, 40)
    z = np.array([[25.0, 0.3], [18.0, -0.6]], f32)
    A, B, Cs = np.arange(0, 300), np.arange(300, 700), np.arange(700, 800)
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
    got, m, pk = _check(s, False, [0, nf, nf + 1], "partial holding")
    wh = pk["w"].astype(f64) / pk["w"].astype(f64).sum()
    assert np.ptp(pk["w"]) > 0, "the weights are even: the shares would be head counts"
    if with_c:
        assert got["both"] == 100 and 0.0 < got["share"] < 1.0 and abs(got["share"] - wh[Cs].sum()) <= 8.0 * N * U
        lo, hi = pk["xf"][Cs, nf].astype(f64).min(0), pk["xf"][Cs, nf].astype(f64).max(0)
        assert np.all(got["mean"][5:7] >= lo) and np.all(got["mean"][5:7] <= hi)
    else:
        assert got["both"] == 0 and got["share"] == 0.0 and np.isnan(got["raw"][1:]).all()
    one, _, _ = _check(s, False, [nf], "partial holding, one new slot")
    assert one["both"] == (400 if with_c else 300) and 0.0 < one["share"] < 1.0
    # a repeated slot
    r, mr, _ = _check(s, False, [1, nf, 1, nf], "partial holding, repeated slots")
    assert r["both"] == one["both"]
    assert np.array_equal(r["mean"][3:7], r["mean"][7:11]) and np.array_equal(r["pf"][:2], r["pf"][2:])
    assert np.array_equal(np.diag(r["scatter"])[3:7], np.diag(r["scatter"])[7:11])
    # retired slots are reported like any other
    before = s.joint_summary([0, 1, nf])
    s.retire_landmarks([1])
    after, _, _ = _check(s, False, [0, 1, nf], "partial holding, slot 1 retired")
    assert _bits(before) == _bits(after)
    s.close()


# ---- determinism, chunking, read-only ---------------------------------------------------------------------------------------------------
def test_deterministic_and_independent_of_the_chunking(sg, monkeypatch):
    """one state: two calls, and the block pairs cut into chunks of 1, 3 and 16 (SLAMGPU_JOINT_CHUNK): the same bits"""
    s = _pp_state(sg)
    nf = s.nf()
    assert nf >= 3
    held = np.flatnonzero(s.map_summary()["share"] > 0.5)
    assert len(held) >= 1
    for slots in (held, np.arange(nf), []):
        x, y = s.joint_summary(slots), s.joint_summary(slots)
        assert _bits(x) == _bits(y), "two calls on one state differ"
        for chunk in ("1", "3", "16"):
            monkeypatch.setenv("SLAMGPU_JOINT_CHUNK", chunk)
            y = s.joint_summary(slots)
            monkeypatch.delenv("SLAMGPU_JOINT_CHUNK")
            assert _bits(x) == _bits(y), "block pairs in chunks of %s: different bits" % chunk
    _check(s, False, held, "per-particle run, slots held by most")
    d = s.download()
    assert _bits(s.joint_summary(held)) == _bits(s.joint_summary(held))
    _note(jm.compare(s.joint_summary(np.arange(nf)), jm.model(d, False, np.arange(nf)), s.N, "flattened, every slot"))
    s.close()


@pytest.mark.parametrize("layout,logw", ODD_CASES)
def test_odd_tiles_uneven_count(sg, monkeypatch, layout, logw):
    """test_gpu_map_summary's shapes: ODD_N particles (a last tile of six), a list of 11 slots (three block pairs, taken two at a
    time), both layouts and both weight forms, a gather pending: the model within its bounds, and the bits of the call in one chunk"""
    def check(s, tag):
        slots = np.arange(_uneven(s.nf()))
        assert s.N == ODD_N
        monkeypatch.setenv("SLAMGPU_JOINT_CHUNK", "2")
        got, m, pk = _check(s, logw, slots, tag)
        monkeypatch.delenv("SLAMGPU_JOINT_CHUNK")
        assert _bits(s.joint_summary(slots)) == _bits(got), "the block pairs in chunks of 2: different bits"
    _odd_pending(sg, layout, logw, check)


def test_per_particle_run_is_not_disturbed(sg):
    """slamgpu_run_particle, 60 steps in calls of 30, a checked call after each: the run with the calls in between is the run without
    them, bit for bit"""
    N, steps, K = 2048, 60, 30
    c = _course("FASTSLAM2", steps)
    opt = _opt(EXCL_ON, 1, 0.02)

    def run(observe):
        d = _ctx(sg, c, N, 2, 1)
        seen = []
        for a in range(0, steps, K):
            d.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], c["xt"][a:a + K], c["max_range"], c["R"], noise=2, **opt)
            if observe:
                held = np.flatnonzero(d.map_summary()["share"] > 0.5)
                seen.append(_check(d, False, held, "run_particle after %d" % (a + K))[0])
                _check(d, False, np.arange(d.nf()), "run_particle after %d, every slot" % (a + K))
        rep = d.particle_report_fetch()
        return _finish(d), rep, seen
    with_, rep_w, seen = run(True)
    without, rep_o, _ = run(False)
    _same_state(with_, without, "joint summaries between the calls")
    assert np.array_equal(rep_w, rep_o)
    assert len(seen) == steps // K and all(len(g["pf"]) >= 1 and 0 < g["both"] <= N for g in seen)


# ---- degenerate weights, refusals ---------------------------------------------------------------------------------------------------------
def test_degenerate_weights_give_nan(sg):
    """weights that sum to zero, or to nothing finite: every double NaN and no error; `both` is still counted"""
    N = 1000
    s, d = _uploaded(sg, N, 5)
    for w in (np.zeros(N, f32), np.where(np.arange(N) == 7, np.inf, d["w"]).astype(f32), np.where(np.arange(N) == 3, np.nan, d["w"]).astype(f32)):
        s.upload(dict(d, w=w))
        for slots in ([0, 1, 2], []):
            got = s.joint_summary(slots)
            assert np.isnan(got["raw"]).all() and got["both"] == N
            m = jm.model(s.peek(), False, slots)
            assert np.isnan(m["share"]) and m["both"] == N
    s.upload(d)
    _check(s, False, [0, 1, 2], "after the degenerate uploads")
    s.close()


def test_refusals_leave_the_outputs_alone(sg):
    import ctypes as C
    s, d = _uploaded(sg, 512, 5)
    L = s.L

    def raw(ctx, slots, k, null_slots=False, null_out=False):
        slots = np.ascontiguousarray(slots, np.int32)
        out, both = np.full(jm.joint_size(max(k, 0)) if k <= 126 else 8, -7.25), np.full(1, -77, np.int32)
        rc = L.slamgpu_joint_summary(ctx.h, None if null_slots else slots.ctypes.data_as(C.c_void_p), k,
                                     None if null_out else out.ctypes.data_as(C.c_void_p), both.ctypes.data_as(C.c_void_p))
        if rc != 0:
            assert np.all(out == -7.25) and np.all(both == -77), "a refused call wrote to its outputs"
        return rc
    pk0 = s.peek()
    full = s.joint_summary(np.arange(5))
    assert raw(s, [0, -1], 2) == ERR_INVALID
    assert raw(s, [0, 5], 2) == ERR_INVALID
    assert raw(s, [0], -1) == ERR_INVALID
    assert raw(s, np.zeros(127), 127) == ERR_INVALID
    assert raw(s, [0], 1, null_slots=True) == ERR_INVALID
    assert raw(s, [0], 1, null_out=True) == ERR_INVALID
    assert raw(s, [0], 0, null_out=True) == ERR_INVALID
    assert raw(s, [0], 0, null_slots=True) == 0
    assert L.slamgpu_joint_summary(s.h, None, 0, np.zeros(jm.joint_size(0)).ctypes.data_as(C.c_void_p), None) == 0   # (both may be NULL)
    with pytest.raises(sg.SlamGpuError) as e:
        s.joint_summary([0, 5])
    assert e.value.code == ERR_INVALID
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    assert raw(shard, [0], 0) == ERR_INVALID
    with pytest.raises(sg.SlamGpuError) as e:
        shard.joint_summary([])
    assert e.value.code == ERR_INVALID and "single contexts only" in str(e.value)
    shard.close()
    pk1 = s.peek()
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(pk0[k], pk1[k], equal_nan=True), k
    assert _bits(s.joint_summary(np.arange(5))) == _bits(full)
    s.close()


# ---- far from the origin -----------------------------------------------------------------------------------------------------------------
def test_map_moved_far_from_the_origin(sg):
    """the set of a run moved to (10^5, -10^5) m: the scatter keeps its bound (8 N u D_a D_b, no |mu| in it): the pivot earns its keep"""
    N = 1000
    c = _course("FASTSLAM2", 100)
    s = _known(sg, c, N, 2, 1)
    _run(s, c, 0, 50)
    d = s.download()
    shift = np.array([1.0e5, -1.0e5], f32)
    d["xv"] = d["xv"].copy()
    d["xv"][:, :2] += shift
    d["xf"] = d["xf"] + shift
    s.upload(d)
    slots = np.arange(d["nf"])
    got, m, pk = _check(s, False, slots, "moved to (1e5, -1e5)")
    assert np.abs(m["mean"][:2]).min() > 9.0e4 and m["range"][:2].max() < 100.0
    # what the bound would have to be without a pivot: the cancellation of sum w v v^T - mu mu^T is at the size of mu^2
    print("joint_summary moved: worst scatter error %.3g, bound %.3g, u mu^2 %.3g" %
          (np.abs(got["scatter"] - m["scatter"]).max(), jm.bounds(m, N)["scatter"].max(), U * 1.0e10))
    s.close()


# ---- slam-backend -map joint -----------------------------------------------------------------------------------------------------------------
JOINT = (r"joint posterior: k (\d+), D (\d+), joint share (\d+\.\d+), (\d+) particles hold them all; pose position sigma (\d+\.\d+) m; P is (positive definite|"
         r"NOT positive definite); largest \|correlation\| pose-landmark (\d+\.\d+), landmark-landmark (\d+\.\d+)$")


CLI_RUN = ["-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384", "-SWITCH_SEED_RANDOM", "7"]


def _backend_twin(sg, maxsteps):
    """the context of `slam-backend CLI_RUN -rng philox -maxsteps n -assoc particle -observe device` at the end of its run, driven from
    Python as slam_backend.cpp drives it: the configuration from the same arguments, the host simulator's controls and true poses
    with NO host observation drawn (the device makes them; the sensor noise would advance libc rand() and change the controls), the
    simulator created after the context (HIP's start-up draws from rand()), slamgpu_run_particle in calls of 256 iterations"""
    import math
    from slam_amd import host
    probe = host.HostSim(CLI_RUN)
    cf, lm = probe.conf, probe.map()[0]
    Qe, Re, dt = probe.noise()
    probe.close()
    N = int(cf.NPARTICLES)
    s = sg.SlamGpu(N, 4 * int(cf.n_landmarks), method=2, n_effective=int(cf.NEFFECTIVE), resample=cf.SWITCH_RESAMPLE == 1,
                   use_heading=cf.SWITCH_HEADING_KNOWN == 1, add_predict_noise=cf.SWITCH_PREDICT_NOISE == 1, wheel_base=float(cf.WHEELBASE),
                   sigma_phi=float(cf.sigmaT), rng_mode=sg.RNG_PHILOX, seed=int(cf.SWITCH_SEED_RANDOM), math_mode=sg.MATH_FAST,
                   device_observe=True, particle_maps=True)
    s.set_particle_excl_spacing(0.0)
    s.set_map(lm)
    sim = host.HostSim(CLI_RUN)   # (seeds rand() now, as the binary does after slamgpu_create)
    ctl, steps, xts = [], [], []
    for it in range(maxsteps):
        r, V, G, phi = sim.control()
        if r < 0:
            break
        ctl.append((V, G, phi))
        if r == 1:
            steps.append(np.array(ctl, f32).reshape(-1, 3))
            xts.append(sim.true_pose())
            ctl = []
    sim.close()
    R4 = np.asarray(Re, f64).reshape(-1)
    p_new = math.exp(-0.5 * float(cf.GATE_REJECT)) / (2.0 * math.pi * math.sqrt(max(1e-30, R4[0] * R4[3] - R4[1] * R4[2])))
    for a in range(0, len(steps), 256):
        s.run_particle(steps[a:a + 256], Qe, float(dt), xts[a:a + 256], float(cf.MAX_RANGE), Re, noise=2 if cf.SWITCH_SENSOR_NOISE else 0,
                       gate_reject=float(cf.GATE_REJECT), gate_augment=float(cf.GATE_AUGMENT), mode=0, new_share=0.02, p_new=p_new, census_every=1,
                       excl=(2.0, 0.05, 2.0))
    s.particle_report_fetch()
    s.history_fetch()
    return s, len(steps)


def test_slam_backend_map_joint(sg, tmp_path):
    """-assoc particle -observe device -map joint -JOINT_OUT file on example_webmap, 512 particles, seed 7: the posterior line, then
    the joint line; the file holds D, x and the D rows of a symmetric P, and the line's figures are those of that P.  The same run
    driven from Python (_backend_twin) is the independent source: the slots listed are those its map_summary gives at least half of the
    weight, the file equals joint_dense of its joint_summary, and -- where the sets coincide: a slot whose holders are exactly J, the
    pose when J is everybody -- x and the diagonal blocks of P equal map_summary's / pose_summary's mean and scatter + mean Pf / Pv
    within the sum of both calls' bounds"""
    import slam_amd.host as host
    path = str(tmp_path / "joint.txt")
    r = subprocess.run([EXE, *CLI_RUN, "-rng", "philox", "-maxsteps", "3000", "-assoc", "particle", "-observe", "device", "-map", "joint",
                        "-JOINT_OUT", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
    out = r.stdout.splitlines()
    pl, jl = [ln for ln in out if ln.startswith("posterior map:")], [ln for ln in out if ln.startswith("joint posterior:")]
    assert len(pl) == 1 and len(jl) == 1 and out.index(jl[0]) == out.index(pl[0]) + 1
    g = re.match(JOINT, jl[0])
    assert g, jl[0]
    print("slam-backend -map joint:", jl[0])
    k, D, share, both = int(g.group(1)), int(g.group(2)), float(g.group(3)), int(g.group(4))
    assert D == 3 + 2 * k and 1 <= k <= 126 and 0.0 < share <= 1.0 + 1e-6 and 0 < both <= 512
    assert 0.0 <= float(g.group(7)) <= 1.0 + 1e-9 and 0.0 <= float(g.group(8)) <= 1.0 + 1e-9
    assert k == int(re.match(r"posterior map: (\d+) slots held by at least half", pl[0]).group(1)) or k == 126
    lines = open(path).read().splitlines()
    assert len(lines) == D + 2 and int(lines[0]) == D
    x = np.array(lines[1].split(), f64)
    P = np.array([ln.split() for ln in lines[2:]], f64)
    assert x.shape == (D,) and P.shape == (D, D) and np.array_equal(P, P.T) and -np.pi < x[2] <= np.pi
    ev = np.linalg.eigvalsh(P)
    assert (g.group(6) == "positive definite") == bool(ev.min() > 0) or abs(ev.min()) < 1e-12 * ev.max()
    # the line's figures are the file's
    assert abs(float(g.group(5)) - np.sqrt(P[0, 0] + P[1, 1])) <= 1e-6
    sd = np.sqrt(np.diag(P))
    R = np.abs(P / np.outer(sd, sd))
    lm = (np.arange(3, D) - 3) // 2
    other = lm[:, None] != lm[None, :]
    assert abs(float(g.group(7)) - R[3:, :3].max()) <= 1e-6 and abs(float(g.group(8)) - (R[3:, 3:] * other).max()) <= 1e-6
    # the same run through Python
    nobs = int(re.search(r"observation steps (\d+)", r.stdout).group(1))
    s, steps = _backend_twin(sg, 3000)
    N = s.N
    assert steps == nobs, "the twin made %d observation steps, the binary %d" % (steps, nobs)
    pk = s.peek()
    ms, ps = s.map_summary(), s.pose_summary()
    slots = np.flatnonzero(ms["share"] >= 0.5)[:126]
    assert len(slots) == k, "the twin gives %d slots at least half of the weight, the binary listed %d" % (len(slots), k)
    j = s.joint_summary(slots)
    xt, Pt, status = host.joint_dense(j)
    assert j["both"] == both and abs(j["share"] - share) <= 1e-6 and (status == 0) == (g.group(6) == "positive definite")
    assert np.array_equal(xt, x) and np.array_equal(Pt, P), "the file is not joint_dense of the same run's joint_summary"
    m = jm.model(pk, False, slots)
    _note(jm.compare(j, m, N, "slam-backend's run through Python"))
    jb = jm.bounds(m, N)
    mb = _map_bounds(_map_model(pk, False), N)
    same = [a for a, l in enumerate(slots) if ms["holders"][l] == both]   # J is a subset of every listed slot's holders
    assert same, "no listed slot is held by exactly the particles that hold them all"
    worst = 0.0
    for a in same:
        l, r0 = slots[a], 3 + 2 * a
        sc, pf = ms["scatter"][l], ms["pf"][l]
        exp = np.array([[sc[0] + pf[0], sc[1] + pf[1]], [sc[1] + pf[1], sc[2] + pf[2]]])
        bound = jb["scatter"][r0:r0 + 2, r0:r0 + 2] + jb["pf"][a, 0] + mb["scatter"][l] + mb["pf"][l]
        err = np.abs(P[r0:r0 + 2, r0:r0 + 2] - exp)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (a, l)
        assert np.all(np.abs(x[r0:r0 + 2] - ms["mean"][l]) <= jb["mean"][r0:r0 + 2] + mb["mean"][l]), (a, l)
    print("slam-backend -map joint: %d of %d listed slots held by exactly J (|J| %d of %d): diagonal blocks against map_summary's scatter + mean Pf, "
          "worst error / summed bound %.3g" % (len(same), k, both, N, worst))
    if both == N:
        pb = pose_model.bounds(pk["xv"], pk["Pv"], pose_model.summary(pk["xv"], pk["Pv"], pk["w"], False))
        exp = np.zeros((3, 3))
        exp[np.tril_indices(3)] = ps[6:12] + ps[12:18]
        exp = exp + np.tril(exp, -1).T
        bnd = np.zeros((3, 3))
        bnd[np.tril_indices(3)] = pb[6:12] + pb[12:18] + jb["scatter"][np.tril_indices(3)] + jb["pv"]
        bnd = bnd + np.tril(bnd, -1).T
        err = np.abs(P[:3, :3] - exp)
        print("slam-backend -map joint: pose block against pose_summary's scatter + mean Pv, worst error / summed bound %.3g" % float((err / bnd).max()))
        assert np.all(err <= bnd)
        assert np.all(np.abs(x[:2] - ps[1:3]) <= jb["mean"][:2] + pb[1:3])
        assert abs(np.remainder(x[2] - ps[3] + np.pi, 2 * np.pi) - np.pi) <= jb["mean"][2] + pb[3] + 4 * U * np.pi
    s.close()


def test_worst_ratios():
    """(last) prints the worst error / bound ratio of every quantity over the checks this process has made before it: a report for
    DESIGN.md section 7g, not a check -- every compare() asserts its own bounds, and run alone this has nothing to print"""
    print("joint_summary worst error / bound over the module: " + ", ".join("%s %.3g" % (q, r) for q, r in sorted(WORST.items())))
