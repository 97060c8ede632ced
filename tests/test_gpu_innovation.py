"""Innovation posterior on the device (slamgpu_innovation_summary, slamgpu_innovation_*): per re-observed landmark of a packet the holders'
share, the mean and scatter of the innovation, the mean innovation covariance and the mean per-particle NIS, reduced over ALL particles
by innovation_summary_kernel / innovation_finish_kernel.

The yardstick is tests/innovation_model.py (float64, math.fsum / sqrt / atan2 / remainder, written from the header) evaluated on
peek(first=0, stride=1, count=N) of the same context taken immediately before the call.  The tolerances are rounding bounds
(innovation_model.bounds), derived as tests/test_gpu_pose.py derives its own.  With u = 2^-53, N the particle count, and for one
observation D0 / D1 the ranges of v0 / v1 over the holders that carry weight, |mu| the model's mean innovation:
  * any order of summing n terms in double errs by at most (n - 1) u sum |t_i|; the weights are non-negative and sum to 1; terms about
    a pivot inside the holders' cloud are bounded by D and D^2; every merge of two partial means rounds once at the size of the mean and
    carries that into M2 through delta^2, |delta| <= D; no path from a particle to an output has more than N such steps; a factor 8
    covers the division by the weight sum, the final pivot shift and (log-weights) the few ulps between two correct exp: 8 N u at the
    scale of the terms, as for the map and pose summaries;
  * per term, device and model evaluate the SAME formula on the same float32 inputs promoted to double; dx, dy, d2 round identically;
    two correct sqrt differ by at most 2 ulps of d, and v0 = z_r - d rounds once more: e0 = 4 u d + 2 u |v0|; two correct atan2 differ
    by at most 4 ulps, and the two subtractions before the (exact) remainder round at the size of their operands:
    e1 = 8 u (|atan2| + |theta| + |z_b|).  A per-term error passes into a weighted mean unchanged and into a second moment as 2 D e + e^2;
  * S_i takes 4 divisions (carrying sqrt's ulps), 12 products and 9 sums: 16 u at the size of the terms it is summed from,
    |H| |Pf| |H|^T + |R| entrywise, from the model's own H and Pf;
  * nis_i = num / det: the errors of v and S enter num directly and det = s00 s11 - s10^2 at 1 / det -- the amplification by the
    conditioning of S_i, taken from the model's own S_i.
    [0] share          8 N u
    [1] mean v0        8 N u (D0 + |mu0|) + e0                     [2] likewise with D1, mu1, e1
    [3] rr             8 N u D0 (D0 + |mu0|) + 2 D0 e0 + e0^2      [5] likewise
    [4] rb             8 N u (D0 (D1 + |mu1|) + D1 (D0 + |mu0|)) + D0 e1 + D1 e0 + e0 e1
    [6..8] mean S      8 N u max |S_i entry| + 16 u max (|H| |Pf| |H|^T + |R|) entry
    [9] mean nis       8 N u max |nis_i| + max_i (dnum_i + |nis_i| ddet_i) / |det_i|
and NaN exactly where the model says NaN; holders exactly.  A bound of 0 (N = 1: D = 0, e enters the mean only) asks for the exact
value.  Every check prints its worst error / bound ratio before it asserts.

A summary taken after queued predicts never meets a pending gather (flushing the predicts settles it first), so the pending path is
reached by a second summary of the same packet immediately after the update that resampled: the contract does not care when it is asked."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import innovation_model as im
from conftest import DATA
from test_gpu_particle_assoc import _predicts, _tape
from test_gpu_particle_device import EXE, ERR_INVALID, _same_state
from test_gpu_particle_lists import _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53
KBLOCK, TILE = 256, 1024   # kernels.h: kBlock, kMapTile
ERR_CAPACITY = -3
GROUPS = (("share", slice(0, 1)), ("mean v", slice(1, 3)), ("scatter", slice(3, 6)), ("mean S", slice(6, 9)), ("mean nis", slice(9, 10)))
_TAPES = {}
WORST = {}


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _compare(got, holders, exp, eh, bound, tag):
    """summaries against the model within the rounding bounds; prints the worst error / bound of each group first"""
    report, bad = [], []
    with np.errstate(all="ignore"):
        err = np.abs(got - exp)
        ratio = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
    for name, sl in GROUPS:
        some = ~np.isnan(exp[:, sl])
        worst = float(ratio[:, sl][some].max()) if some.any() else 0.0
        WORST[name] = max(WORST.get(name, 0.0), worst)
        report.append("%s %.3g (err %.3g)" % (name, worst, float(err[:, sl][some].max()) if some.any() else 0.0))
        if not np.array_equal(np.isnan(got[:, sl]), np.isnan(exp[:, sl])):
            bad.append(name + ": NaN pattern")
        elif not np.all(err[:, sl][some] <= bound[:, sl][some]):
            bad.append(name + ": outside its bound")
    print("innovation_summary %s: %d observations; worst error / bound: %s" % (tag, len(exp), ", ".join(report)))
    assert np.array_equal(holders, eh), (tag, holders, eh)
    assert not bad, (tag, bad)


def _check(s, zf, idf, R, logw, tag):
    pk = s.peek()
    got, holders = s.innovation_summary(zf, idf, R)
    exp, eh, terms = im.summary(pk["xv"], pk["w"], pk["xf"], pk["Pf"], zf, idf, R, logw)
    _compare(got, holders, exp, eh, im.bounds(terms, s.N, exp), "%s N %d" % (tag, s.N))
    return got, holders, exp


def _packet(st):
    return np.array(st["zf"], f32).reshape(-1, 2), np.array(st["idf"], np.int32), np.array(st["zn"], f32).reshape(-1, 2)


def _update(s, st, tape):
    zf, idf, zn = _packet(st)
    if len(zf) + len(zn):
        s.update(zf, idf, zn, tape["R"])
    s.estimate_async()


def _webmap(N, steps=100):
    if ("webmap", N, steps) not in _TAPES:
        _TAPES[("webmap", N, steps)] = _tape("FASTSLAM2", N, steps)
    return _TAPES[("webmap", N, steps)]


def _big(tmp_path_factory, steps=30):
    """host-made packets on a synthetic 1 000-landmark map: plain genealogy rows, packets of dozens of observations"""
    if "big" not in _TAPES:
        from slam_amd import host
        mp = _synthetic(tmp_path_factory, 1000)
        _TAPES["big"] = host.make_tape(["-m", mp, "-method", "FASTSLAM2", "-NPARTICLES", 100, "-NEFFECTIVE", 75, "-SWITCH_SEED_RANDOM", 7], max_obs=steps)
    return _TAPES["big"]


def _uploaded(sg, xv, w, xf, Pf, mm=1, logw=False):
    """a PARTICLE_MAPS context holding exactly this set (absent records: NaN)"""
    xv = np.asarray(xv, f32)
    N, nf = len(xv), np.asarray(xf).shape[1]
    s = sg.SlamGpu(N, max(nf, 4), method=2, rng_mode=sg.RNG_PHILOX, seed=2, math_mode=mm, particle_maps=True, log_weights=logw)
    d = s.download()
    d.update(nf=nf, xv=xv, w=np.asarray(w, f32), xf=np.asarray(xf, f32), Pf=np.asarray(Pf, f32))
    s.upload(d)
    return s


R0 = np.array([0.01, 0.0, 0.0, 0.0004], f32)


def _cloud(N, x0=0.0, seed=1, nf=3):
    """a 1 m cloud about (x0, -3) heading about 0.7, three landmarks 15 to 25 m away, every record with its own spread and covariance"""
    rng = np.random.default_rng(seed + N)
    xv = np.stack([x0 + rng.normal(0.0, 1.0, N), -3.0 + rng.normal(0.0, 0.5, N), rng.normal(0.7, 0.1, N)], axis=1).astype(f32)
    lm = np.array([[x0 + 20.0, 4.0], [x0 - 12.0, -14.0], [x0 + 3.0, 17.0]])[:nf]
    xf = (lm[None] + rng.normal(0.0, 0.3, (N, nf, 2))).astype(f32)
    A = rng.normal(0.0, 0.2, (N, nf, 2, 2))
    Pf = (A @ A.transpose(0, 1, 3, 2) + 0.01 * np.eye(2)).astype(f32)
    w = rng.uniform(0.0, 1.0, N)
    if N > 2:
        w[1::5] = 0.0
    true = np.array([x0, -3.0, 0.7])
    d = lm - true[:2]
    zf = np.stack([np.hypot(d[:, 0], d[:, 1]) + 0.1, np.arctan2(d[:, 1], d[:, 0]) - true[2] + 0.01], axis=1).astype(f32)
    return xv, w.astype(f32), xf, Pf, zf


# ---- 1. the model on a real run, compact layout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_model_on_example_webmap(sg, mm):
    """FastSLAM 2, N = 1 000, host-made packets: predicts, the checked summary, the update -- one step at a time from step 20 until one
    summary was taken under a pending gather (right after an update that resampled) and one without; every share 1, holders = N"""
    N = 1000
    tape = _webmap(N)
    s = sg.SlamGpu(N, tape["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=mm)
    assert s.genealogy_rows()[1] <= 40, "not the compact layout"
    for st in tape["steps"][:20]:
        _predicts(s, st, tape)
        _update(s, st, tape)
    seen = set()
    for k in range(20, 100):
        st = tape["steps"][k]
        zf, idf, zn = _packet(st)
        _predicts(s, st, tape)
        if len(idf):
            got, holders, exp = _check(s, zf, idf, tape["R"], False, "webmap math%d step %d before the update" % (mm, k))
            seen.add(False)
            assert np.all(np.abs(got[:, 0] - 1.0) <= 8.0 * N * U) and np.all(holders == N)
            assert np.all(got[:, 3] >= 0) and np.all(got[:, 5] >= 0) and np.all(got[:, 6] > 0) and np.all(got[:, 8] > 0) and np.all(got[:, 9] >= 0)
        _update(s, st, tape)
        if len(idf) and s.stats()[1]:   # this update resampled: its gather is pending, and no predict is queued that would settle it
            got, holders, exp = _check(s, zf, idf, tape["R"], False, "webmap math%d step %d under the pending gather" % (mm, k))
            seen.add(True)
            assert np.all(np.abs(got[:, 0] - 1.0) <= 8.0 * N * U) and np.all(holders == N)
        if len(seen) == 2:
            break
    assert seen == {False, True}, "no summary was taken %s a pending gather" % ("without" if True in seen else "with")
    s.close()


# ---- 2. plain layout, log-weights, a packet across the group of 8, chunks ---------------------------------------------------------------
def test_plain_layout_log_weights(sg, tmp_path_factory, monkeypatch):
    """a 1 000-landmark map (plain genealogy rows), log-weights, N = 3 000 (not a multiple of the tile): the first 12 observations of a
    packet against the model; the same 12 inside the whole packet, and through the partials' table 8 at a time: the same bits"""
    N = 3000
    tape = _big(tmp_path_factory)
    s = sg.SlamGpu(N, tape["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1, log_weights=True)
    assert s.genealogy_rows()[1] > 40, "not the plain layout"
    k = next(k for k in range(12, len(tape["steps"])) if len(tape["steps"][k]["idf"]) >= 12)
    for st in tape["steps"][:k]:
        _predicts(s, st, tape)
        _update(s, st, tape)
    st = tape["steps"][k]
    zf, idf, zn = _packet(st)
    _predicts(s, st, tape)
    assert tape["nlm"] > 256 and s.nf() >= 30 and len(idf) >= 9
    got, holders, exp = _check(s, zf[:12], idf[:12], tape["R"], True, "plain logw step %d" % k)
    assert np.all(holders == N) and np.all(np.abs(got[:, 0] - 1.0) <= 8.0 * N * U)
    whole, wh = s.innovation_summary(zf, idf, tape["R"])
    assert whole[:12].tobytes() == got.tobytes() and np.array_equal(wh[:12], holders), "an observation's bits depend on what else the packet holds"
    monkeypatch.setenv("SLAMGPU_INNOV_CHUNK", "8")
    cut, ch = s.innovation_summary(zf, idf, tape["R"])
    monkeypatch.delenv("SLAMGPU_INNOV_CHUNK")
    assert cut.tobytes() == whole.tobytes() and np.array_equal(ch, wh), "the packet in chunks of 8: different bits"
    back, bh = s.innovation_summary(zf[::-1], idf[::-1], tape["R"])
    assert back[::-1].tobytes() == whole.tobytes(), "an observation's bits depend on its place in the packet"
    s.close()


# ---- 3. per-particle maps: absent records in disjoint sets ----------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_disjoint_holder_sets(sg, mm):
    """slot 0: everybody; slot 1: particles [0, 300); slot 2: particles [300, 1100) (across the tile); slot 3: nobody.  Shares against the
    hand-computed sums of the holders' weights, holders exact; nobody: share 0, NaN; the same slot twice: two identical entries"""
    N = TILE + KBLOCK + 7
    xv, w, xf, Pf, zf = _cloud(N, nf=3)
    xf = np.concatenate([xf, xf[:, :1] + 1.0], axis=1)
    Pf = np.concatenate([Pf, Pf[:, :1]], axis=1)
    A, B = np.arange(0, 300), np.arange(300, 1100)
    for slot, who in ((1, A), (2, B), (3, np.arange(0))):
        out_ = np.setdiff1d(np.arange(N), who)
        xf[out_, slot] = np.nan
        Pf[out_, slot] = np.nan
    s = _uploaded(sg, xv, w, xf, Pf, mm)
    idf = np.array([0, 1, 2, 3, 1], np.int32)
    z = np.concatenate([zf, zf[:1], zf[1:2]]).astype(f32)
    got, holders, exp = _check(s, z, idf, R0, False, "disjoint sets math%d" % mm)
    wd = w.astype(f64)
    assert list(holders) == [N, 300, 800, 0, 300]
    for q, who in ((1, A), (2, B)):
        assert abs(got[q, 0] - wd[who].sum() / wd.sum()) <= 8.0 * N * U and 0.0 < got[q, 0] < 1.0
    assert abs(got[0, 0] - 1.0) <= 8.0 * N * U
    assert got[3, 0] == 0.0 and np.isnan(got[3, 1:]).all()
    assert got[4].tobytes() == got[1].tobytes(), "the same slot twice: different entries"
    s.close()


# ---- 4. constructed sets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_known_answers_on_the_device(sg, mm):
    """the sets of innovation_model.self_check() uploaded: the hand answers hold of the device's summaries (to 1e-12 of their size), and
    the model within its bounds; N = 1: a scatter of exactly 0; N = 4 with non-uniform weights and zeros"""
    for name, (xv, w, xf, Pf, zf, idf, R, logw) in im.known_sets().items():
        s = _uploaded(sg, xv, w, xf, Pf, mm, logw)
        got, holders, exp = _check(s, zf, idf, R, logw, "known set %s math%d" % (name, mm))
        im.check_known(name, got, holders, tol=1e-12)
        s.close()
    xv, w, xf, Pf, zf = _cloud(4)
    w = np.array([0.5, 0.0, 0.3, 0.2], f32)
    s = _uploaded(sg, xv, w, xf, Pf, mm)
    got, holders, exp = _check(s, zf, [0, 1, 2], R0, False, "four particles math%d" % mm)
    assert np.all(holders == 4) and np.all(got[:, 3] > 0)
    s.close()
    xv, w, xf, Pf, zf = _cloud(1)
    s = _uploaded(sg, xv, w, xf, Pf, mm)
    got, holders, exp = _check(s, zf, [0, 1, 2], R0, False, "one particle math%d" % mm)
    assert np.all(got[:, 3:6] == 0.0) and np.all(got[:, 0] == 1.0) and np.all(holders == 1)
    s.close()


@pytest.mark.parametrize("N", [KBLOCK - 1, KBLOCK + 1, TILE + 1])
def test_constructed_clouds(sg, N):
    """uploaded clouds, uneven weights with zeros: a workgroup less one / plus one, one particle more than a tile"""
    xv, w, xf, Pf, zf = _cloud(N)
    s = _uploaded(sg, xv, w, xf, Pf, 1)
    _check(s, zf, [0, 1, 2], R0, False, "cloud")
    s.close()
    rng = np.random.default_rng(N)
    lw = (rng.normal(-700.0, 1.5, N) + np.where(np.arange(N) < TILE, 0.0, -3.0)).astype(f32)   # (the tiles' maxima differ)
    s = _uploaded(sg, xv, lw, xf, Pf, 1, logw=True)
    _check(s, zf, [2, 1, 0], R0, True, "cloud, log-weights")
    s.close()


# ---- 5. far from the origin, bearings at +-pi -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
def test_far_from_the_origin_and_behind_the_vehicle(sg, mm):
    """a 1 m cloud at x = 1e5 m: the innovations stay those of the cloud; and a landmark straight behind the vehicle, whose predicted
    bearing is +pi for half of the particles and -pi for the other half: v1 stays small and so does its scatter"""
    N = TILE + 1
    xv, w, xf, Pf, zf = _cloud(N, x0=1.0e5)
    s = _uploaded(sg, xv, w, xf, Pf, mm)
    got, holders, exp = _check(s, zf, [0, 1, 2], R0, False, "far from the origin math%d" % mm)
    assert np.all(np.abs(got[:, 1]) < 2.0) and np.all(got[:, 3] > 0.1) and np.all(got[:, 3] < 5.0), got[:, :4]
    s.close()
    rng = np.random.default_rng(3)
    xv = np.stack([rng.normal(0.0, 0.05, N), rng.normal(0.0, 0.05, N), rng.normal(0.0, 0.002, N)], axis=1).astype(f32)
    xf = np.stack([np.full(N, -15.0) + rng.normal(0.0, 0.05, N), rng.normal(0.0, 0.05, N)], axis=1).astype(f32)[:, None, :]
    Pf = np.tile((0.01 * np.eye(2)).astype(f32), (N, 1, 1, 1))
    s = _uploaded(sg, xv, np.ones(N, f32), xf, Pf, mm)
    zf = np.array([[15.0, float(f32(np.pi)) - 0.002]], f32)
    got, holders, exp = _check(s, zf, [0], R0, False, "behind the vehicle math%d" % mm)
    ang = np.arctan2(xf[:, 0, 1].astype(f64) - xv[:, 1], xf[:, 0, 0].astype(f64) - xv[:, 0])
    assert (ang > 3.0).sum() > N // 4 and (ang < -3.0).sum() > N // 4, "the bearings do not straddle +-pi"
    assert abs(got[0, 2]) < 0.01 and got[0, 5] < 1e-4, got[0]
    s.close()


# ---- 6. read-only, deterministic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["compact", "plain"])
def test_read_only_and_deterministic(sg, tmp_path_factory, layout):
    """two calls: the same bits; under a pending gather and after download() has settled it: the same bits; the state and the following
    10 steps are bit for bit those of a twin context that never called it"""
    if layout == "compact":
        tape, N, first, logw = _webmap(1000), 1000, 20, False
    else:
        tape, N, first, logw = _big(tmp_path_factory), 1280, 8, True
    last = first + 12

    def run(observe):
        s = sg.SlamGpu(N, tape["nlm"], method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1, log_weights=logw)
        assert (s.genealogy_rows()[1] <= 40) == (layout == "compact")
        pending = 0
        for k in range(last + 10):
            st = tape["steps"][k]
            zf, idf, zn = _packet(st)
            _predicts(s, st, tape)
            look = observe and first <= k < last and len(idf) > 0
            if look:
                a, b = s.innovation_summary(zf, idf, tape["R"]), s.innovation_summary(zf, idf, tape["R"])
                assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), "two summaries of one state differ"
            _update(s, st, tape)
            if look and s.stats()[1]:
                pending += 1
                a = s.innovation_summary(zf, idf, tape["R"])
                s.download()
                b = s.innovation_summary(zf, idf, tape["R"])
                assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), "pending and settled: different bits"
        if observe:
            assert pending > 0, "no summary was taken with a gather pending"
        hist = s.history_fetch()
        d = s.download()
        s.close()
        return hist, d
    _same_state(run(True), run(False), "summaries between the steps (%s)" % layout)


# ---- the shapes at which the code the summaries share can go wrong -----------------------------------------------------------------------
ODD_N = 9222   # ten tiles of 1 024 particles with six in the last (tests/test_gpu_map_summary.py: ODD_N)


@pytest.mark.parametrize("layout,logw", [(layout, logw) for layout in ("compact", "plain") for logw in (False, True)])
def test_odd_tiles_uneven_count(sg, monkeypatch, layout, logw):
    """ODD_N particles on example_webmap (at most 16 slots in use), compact rows or plain ones (a capacity past the compact layouts'),
    linear or log weights: straight after an update that resampled (its gather pending), a packet of 11 observations (the step's own,
    repeated) through the partials' table 8 at a time: the model within its bounds, and the bits of the same packet in one chunk"""
    tape = _webmap(1000)
    s = sg.SlamGpu(ODD_N, tape["nlm"] if layout == "compact" else 300, method=2, n_effective=int(0.75 * ODD_N), rng_mode=sg.RNG_PHILOX, seed=5,
                   math_mode=1, log_weights=logw)
    assert (s.genealogy_rows()[1] <= 40) == (layout == "compact")
    for k, st in enumerate(tape["steps"]):
        zf, idf, zn = _packet(st)
        _predicts(s, st, tape)
        _update(s, st, tape)
        if k >= 40 and len(idf) and s.stats()[1]:   # this update resampled: its gather is pending, and no predict is queued that would settle it
            assert s.nf() <= 16
            zf, idf = np.resize(zf, (11, 2)), np.resize(idf, 11)
            monkeypatch.setenv("SLAMGPU_INNOV_CHUNK", "8")
            got, holders, exp = _check(s, zf, idf, tape["R"], logw, "odd tiles %s %s step %d" % (layout, "log" if logw else "linear", k))
            monkeypatch.delenv("SLAMGPU_INNOV_CHUNK")
            whole, wh = s.innovation_summary(zf, idf, tape["R"])
            assert whole.tobytes() == got.tobytes() and np.array_equal(wh, holders), "the packet in chunks of 8: different bits"
            s.close()
            return
    raise AssertionError("no update from step 40 on resampled: no summary was taken with a gather pending")


# ---- 7. degenerate weights, refusals --------------------------------------------------------------------------------------------------
def test_degenerate_weights_give_nan(sg):
    """all-zero weights, one infinite weight: every double NaN, return 0, holders still exact"""
    N = KBLOCK + 1
    xv, w, xf, Pf, zf = _cloud(N)
    xf[:100, 1] = np.nan
    Pf[:100, 1] = np.nan
    for ww in (np.zeros(N, f32), np.where(np.arange(N) == 7, np.inf, w).astype(f32)):
        s = _uploaded(sg, xv, ww, xf, Pf)
        got, holders = s.innovation_summary(zf, [0, 1, 2], R0)
        assert np.isnan(got).all() and list(holders) == [N, N - 100, N]
        s.close()
    s = _uploaded(sg, xv, np.full(N, -np.inf, f32), xf, Pf, logw=True)
    got, holders = s.innovation_summary(zf, [0, 1, 2], R0)
    assert np.isnan(got).all() and list(holders) == [N, N - 100, N]
    s.close()


def test_refusals_leave_outputs_untouched(sg):
    vp = C.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    out, hold = np.full((3, 10), -1.0), np.full(3, -1, np.int32)
    xv, w, xf, Pf, zf = _cloud(300)
    idf = np.array([0, 1, 2], np.int32)
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    assert shard.L.slamgpu_innovation_summary(shard.h, p(zf), p(idf), 3, p(R0), p(out), p(hold)) == ERR_INVALID
    assert b"single contexts only" in shard.L.slamgpu_last_error()
    assert shard.L.slamgpu_innovation_history_enable(shard.h, 8) == ERR_INVALID and shard.innovation_history_info() == (0, 0, 0, 0)
    assert shard.L.slamgpu_innovation_record(shard.h, p(zf), p(idf), 3, p(R0)) == ERR_INVALID
    shard.close()
    s = _uploaded(sg, xv, w, xf, Pf)
    pk0 = s.peek()
    L = s.L
    for bad in (np.array([0, 3, 1], np.int32), np.array([-1, 0, 1], np.int32)):
        assert L.slamgpu_innovation_summary(s.h, p(zf), p(bad), 3, p(R0), p(out), p(hold)) == ERR_INVALID, bad
    assert L.slamgpu_innovation_summary(s.h, p(zf), p(idf), -1, p(R0), p(out), p(hold)) == ERR_INVALID
    for a in ((None, idf, R0, out), (zf, None, R0, out), (zf, idf, None, out), (zf, idf, R0, None)):
        assert L.slamgpu_innovation_summary(s.h, p(a[0]), p(a[1]), 3, p(a[2]), p(a[3]), p(hold)) == ERR_INVALID
    assert L.slamgpu_innovation_summary(s.h, None, None, 0, None, None, None) == 0   # m == 0 does nothing
    assert np.all(out == -1.0) and np.all(hold == -1)
    assert L.slamgpu_innovation_record(s.h, p(zf), p(idf), 3, p(R0)) == ERR_INVALID and b"ring is off" in L.slamgpu_last_error()
    assert L.slamgpu_innovation_history_enable(s.h, -1) == ERR_INVALID and s.innovation_history_info() == (0, 0, 0, 0)
    assert L.slamgpu_innovation_summary(s.h, p(zf), p(idf), 3, p(R0), p(out), None) == 0 and not np.any(out == -1.0)   # holders may be NULL
    pk1 = s.peek()
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(pk0[k], pk1[k], equal_nan=True), k
    s.close()


# ---- 8. the ring ----------------------------------------------------------------------------------------------------------------------
def _twins(sg, tape, N):
    kw = dict(method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1)
    return sg.SlamGpu(N, tape["nlm"], **kw), sg.SlamGpu(N, tape["nlm"], **kw)


@pytest.mark.parametrize("entry", ["record", "step"])
def test_ring_entries_are_the_synchronous_summaries(sg, entry):
    """the ring's entries equal the synchronous summaries a twin (ring off) takes at the same moments, bit for bit, with the right record
    and slot tags; slamgpu_step records by itself; the twin's poses, weights, history and ancestors are the ring context's"""
    N, steps = 512, 40
    tape = _webmap(N)
    r, t = _twins(sg, tape, N)
    r.innovation_history_enable(4096)
    assert r.innovation_history_info() == (0, 0, 4096, 0)
    sync, tags, anc = [], [], []
    for k in range(steps):
        st = tape["steps"][k]
        zf, idf, zn = _packet(st)
        ctl = np.array(st["controls"], f32).reshape(-1, 3)
        if entry == "step":
            r.step(ctl, tape["Q"], float(tape["dt"]), zf, idf, zn, tape["R"])
        else:
            _predicts(r, st, tape)
            r.innovation_record(zf, idf, tape["R"])
            r.update(zf, idf, zn, tape["R"])
            r.estimate_async()
        _predicts(t, st, tape)
        if len(idf):
            sync.append(t.innovation_summary(zf, idf, tape["R"])[0])
        tags += [(k, int(l)) for l in idf]
        t.update(zf, idf, zn, tape["R"])
        t.estimate_async()
        if k % 8 == 7:
            anc.append((r.ancestors(), t.ancestors()))
    sync = np.concatenate(sync)
    a, b, cap, rec = r.innovation_history_info()
    assert (a, b, cap, rec) == (0, len(sync), 4096, steps), (a, b, cap, rec, len(sync))
    ring, record, slot = r.innovation_history_fetch()
    assert ring.shape == sync.shape and ring.tobytes() == sync.tobytes(), "ring entries differ from the synchronous summaries"
    assert [(int(x), int(y)) for x, y in zip(record, slot)] == tags
    again = r.innovation_history_fetch()
    assert again[0].tobytes() == ring.tobytes(), "the fetch consumed something"
    part = r.innovation_history_fetch(5, 7)
    assert part[0].tobytes() == ring[5:12].tobytes() and np.array_equal(part[2], slot[5:12])
    for x, y in anc:
        assert np.array_equal(x, y), "ancestors differ"
    hr, ht = r.history_fetch(), t.history_fetch()
    assert np.any(hr[2]) and not np.all(hr[2]), "the window holds no resampling step, or nothing else"
    _same_state((hr, r.download()), (ht, t.download()), "ring on / off (%s)" % entry)
    r.close()
    t.close()


def test_ring_capacity_upload_and_launch_counts(sg):
    """with the ring off and the summary never called: zero launches of both kernels; capacity 16 fed 5 packets of 6: entries [14, 30)
    retained; m > capacity refused with nothing appended; m == 0 counts a record and appends nothing; upload keeps the entries"""
    N = 512
    tape = _webmap(N)
    s, t = _twins(sg, tape, N)
    t.close()
    s.profile(True)
    for st in tape["steps"][:14]:
        _predicts(s, st, tape)
        _update(s, st, tape)
    s.peek()
    s.download()
    for name in ("innovation_summary", "innovation_finish"):
        assert s.kernel_time(name)[1] == 0, name
    assert s.innovation_history_info() == (0, 0, 0, 0)
    assert s.innovation_history_fetch(0, 0)[0].shape == (0, 10)
    nf = s.nf()
    assert nf >= 3
    rng = np.random.default_rng(1)
    s.innovation_history_enable(16)
    sync, slots = [], []
    for k in range(5):
        idf = rng.integers(0, nf, 6).astype(np.int32)
        zf = np.stack([rng.uniform(5.0, 25.0, 6), rng.uniform(-1.0, 1.0, 6)], axis=1).astype(f32)
        s.innovation_record(zf, idf, tape["R"])
        sync.append(s.innovation_summary(zf, idf, tape["R"])[0])
        slots += [int(l) for l in idf]
    sync = np.concatenate(sync)
    assert s.innovation_history_info() == (14, 30, 16, 5)
    for name in ("innovation_summary", "innovation_finish"):
        assert s.kernel_time(name)[1] == 10, name   # five records, five synchronous summaries, one chunk each
    got, record, slot = s.innovation_history_fetch()
    assert got.tobytes() == sync[14:].tobytes() and list(slot) == slots[14:] and list(record) == [q // 6 for q in range(14, 30)]
    # m > capacity: refused, nothing appended, no record counted; m == 0: a record, nothing appended
    idf = np.zeros(17, np.int32)
    zf = np.ones((17, 2), f32)
    with pytest.raises(sg.SlamGpuError) as e:
        s.innovation_record(zf, idf, tape["R"])
    assert e.value.code == ERR_CAPACITY and s.innovation_history_info() == (14, 30, 16, 5)
    pk0 = s.peek(landmarks=False)   # (slamgpu_step with such a packet: refused before its predicts are queued)
    with pytest.raises(sg.SlamGpuError) as e:
        s.step(np.array([[1.0, 0.0, 0.0]], f32), tape["Q"], float(tape["dt"]), zf, idf, np.zeros((0, 2), f32), tape["R"])
    pk1 = s.peek(landmarks=False)
    assert e.value.code == ERR_CAPACITY and s.innovation_history_info() == (14, 30, 16, 5) and np.array_equal(pk0["xv"], pk1["xv"])
    s.innovation_record(np.zeros((0, 2), f32), np.zeros(0, np.int32), tape["R"])
    assert s.innovation_history_info() == (14, 30, 16, 6)
    with pytest.raises(sg.SlamGpuError) as e:
        s.innovation_record(zf[:2], np.array([0, nf], np.int32), tape["R"])
    assert e.value.code == ERR_INVALID and s.innovation_history_info() == (14, 30, 16, 6)
    # range errors of the fetch, outputs untouched
    out = np.full((16, 10), -1.0)
    vp = C.c_void_p
    for first, count in ((13, 1), (13, 5), (29, 2), (30, 1), (14, -1), (-1, 1)):
        assert s.L.slamgpu_innovation_history_fetch(s.h, first, count, out.ctypes.data_as(vp), None, None) == ERR_INVALID, (first, count)
    assert s.L.slamgpu_innovation_history_fetch(s.h, 30, 0, None, None, None) == 0
    assert np.all(out == -1.0)
    # slamgpu_upload keeps the entries; the next record carries on
    s.upload(s.download())
    assert s.innovation_history_info() == (14, 30, 16, 6) and s.innovation_history_fetch()[0].tobytes() == got.tobytes()
    s.innovation_record(zf[:1], idf[:1], tape["R"])
    last = s.innovation_history_fetch(30, 1)
    assert s.innovation_history_info() == (15, 31, 16, 7) and last[0].tobytes() == s.innovation_summary(zf[:1], idf[:1], tape["R"])[0].tobytes()
    assert int(last[1][0]) == 6 and int(last[2][0]) == 0
    # a restart drops the entries and numbers from 0; 0 stops
    s.innovation_history_enable(8)
    assert s.innovation_history_info() == (0, 0, 8, 0)
    s.innovation_history_enable(0)
    assert s.innovation_history_info() == (0, 0, 0, 0)
    s.close()


# ---- 9. slam-backend ------------------------------------------------------------------------------------------------------------------
LINE = (r"innovation posterior: (\d+) entries summarised, (\d+) retained; mean mixture NIS (\S+), NIS <= 5.9915 in (\S+) of the entries; "
        r"mean per-particle NIS (\S+); mean share (\S+); (\d+) bad entries$")


@pytest.mark.parametrize("assoc", ["known", "gated"])
def test_slam_backend_innovation_posterior(assoc, tmp_path):
    """slam-backend -NPARTICLES 512 -innovation posterior: the line parses, its figures are finite, bad = 0; the trajectory written
    with the option is that of the run without it (both in the loop that makes its own updates: -loop step)"""
    def run(extra, log):
        cmd = [EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
               "-SWITCH_SEED_RANDOM", "7", "-rng", "philox", "-maxsteps", "1500", "-loop", "step", "-log", str(log)]
        if assoc == "gated":
            cmd += ["-assoc", "gated"]
        r = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        traj = [ln.rsplit(",", 1)[0] for ln in open(log).read().splitlines()]   # (the last column is the loop time)
        return r.stdout.splitlines(), traj
    plain, tp = run((), tmp_path / "plain.csv")
    post, tq = run(("-innovation", "posterior"), tmp_path / "post.csv")
    lines = [ln for ln in post if ln.startswith("innovation posterior:")]
    assert len(lines) == 1 and not [ln for ln in plain if ln.startswith("innovation posterior:")]
    assert len(tp) > 1000 and tp == tq, "the trajectory changed with -innovation posterior"
    m = re.match(LINE, lines[0])
    assert m, lines[0]
    print("slam-backend -innovation posterior (%s association):" % assoc, lines[0])
    n, kept, bad = int(m.group(1)), int(m.group(2)), int(m.group(7))
    nis, share95, own, share = (float(m.group(q)) for q in (3, 4, 5, 6))
    assert n > 0 and kept == min(n, 65536) and bad == 0
    assert np.isfinite([nis, share95, own, share]).all() and nis >= 0.0 and own >= 0.0 and 0.0 <= share95 <= 1.0 and 0.0 < share <= 1.0 + 1e-9
    small = run(("-innovation", "posterior", "-INNOVATION_RECORDS", "64"), tmp_path / "small.csv")[0]
    m2 = re.match(LINE, [ln for ln in small if ln.startswith("innovation posterior:")][0])
    assert m2 and int(m2.group(1)) == n and int(m2.group(2)) <= 64
