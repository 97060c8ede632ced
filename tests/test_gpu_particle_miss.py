"""Negative information for the per-particle steps (slamgpu_set_particle_miss): a particle pays p_miss for every landmark it holds,
expects to see from its own pose and has no fresh claim on (pp_missed_kernel, between the resolve and the update launch).

The yardstick for the counts is a float64 numpy model of the header's definition, evaluated on peek() of the same context taken
immediately before the step, and the labels of the step.  A (particle, slot) pair CLEARS when the two comparisons of the definition are
decided by more than 1e-4 of their scale (|d^2 - R^2| > 1e-4 R^2 and |fwd - F| > 1e-4 R; float32 rounding of these expressions stays
two orders of magnitude below that); particles with a pair that does not clear are left out of the comparison, and at most 2 % of the
particles may be left out (a condition on the inputs).  Every check prints its figures before it asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_gpu_particle_assoc import DISCARD, NEW, _predicts, _tape
from test_gpu_particle_device import EXCL_ON, EXE, ERR_INVALID, REPORT, _course, _ctx, _finish, _host_step, _opt, _same_state
from test_gpu_particle_lists import EXHAUSTIVE, LISTS, _course_of, _synthetic

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U53 = 2.0 ** -53
VIEW = (55.0, 1.0)       # view_range, view_front of the constructed cases (example_webmap: MAX_RANGE 60): three slots of the shared map in view
Z_SUB = (25.0, 0.3)      # where the subset's landmark is opened: 25 m out, 0.3 rad off the heading -- well inside that view
_TAPES = {}


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _tape_of(name, N, steps):
    if (name, N, steps) not in _TAPES:
        _TAPES[(name, N, steps)] = _tape(name, N, steps)
    return _TAPES[(name, N, steps)]


# ---- the constructed state: a grown map everybody holds, one slot only a subset holds -----------------------------------------------
def _constructed(sg, method, math, logw, N=1024):
    """test_gpu_map_summary's construction: 20 known-association steps of example_webmap (NEFFECTIVE 0: no resampling, the weights
    stay uneven), then one slot opened by the subset A alone, then the controls of the next step.  Returns the context and (R, nf of the shared map, A)"""
    tape = _tape_of("FASTSLAM2" if method == 2 else "FASTSLAM1", N, 40)
    s = sg.SlamGpu(N, 64, method=method, n_effective=0, rng_mode=sg.RNG_PHILOX, seed=3, math_mode=math, particle_maps=True, log_weights=logw)
    for st in tape["steps"][:20]:
        _predicts(s, st, tape)
        zf, zn = np.array(st["zf"], f32).reshape(-1, 2), np.array(st["zn"], f32).reshape(-1, 2)
        if len(zf) + len(zn):
            s.update(zf, np.array(st["idf"], np.int32), zn, tape["R"])
    nf = s.nf()
    A = np.arange(0, 300)
    lab = np.full((N, 1), DISCARD, np.int32)
    lab[A, 0] = NEW
    rep = s.update_labels(np.array([Z_SUB], f32), tape["R"], lab, new_share=0.0, p_new=1.0, census_every=1)
    assert rep["opened"] == 1 and rep["slots"] == nf + 1, rep
    # (the next step's controls: FastSLAM 2 leaves Pv at nothing after an update, and a second update without a predict in between
    # would invert it)
    _predicts(s, tape["steps"][20], tape)
    return s, (tape["R"], nf, A)


def _geometry(pk):
    xv, xf = pk["xv"].astype(f64), pk["xf"].astype(f64)
    dx, dy = xf[:, :, 0] - xv[:, None, 0], xf[:, :, 1] - xv[:, None, 1]
    held = ~np.isnan(xf[:, :, 0])
    with np.errstate(invalid="ignore"):
        d2 = dx * dx + dy * dy
        fwd = dx * np.cos(xv[:, None, 2]) + dy * np.sin(xv[:, None, 2])
    return held, d2, fwd


def _model(pk, lab, view_range, view_front, retired=()):
    """missed_i by the header's definition in float64, and which particles have every pair cleared"""
    R, F = float(f32(view_range)), float(f32(view_front))
    held, d2, fwd = _geometry(pk)
    nf = held.shape[1]
    with np.errstate(invalid="ignore"):
        inview = held & (d2 < R * R) & (fwd > F)
        clear = ~held | ((np.abs(d2 - R * R) > 1e-4 * R * R) & (np.abs(fwd - F) > 1e-4 * R))
    claimed = np.zeros(held.shape, bool)
    for q in range(lab.shape[1]):   # (the resolve's first-claim rule: the first observation naming a slot claims it, so any does)
        named = lab[:, q] >= 0
        claimed[np.nonzero(named)[0], lab[named, q]] = True
    live = np.ones(nf, bool)
    live[list(retired)] = False
    cnt = (inview & ~claimed & live[None, :]).sum(axis=1).astype(np.int32)
    return cnt, clear[:, live].all(axis=1), inview


def _step_labels(pk, nf, A, view_range, view_front, retire_first=False):
    """one step on the constructed state: three observations (towards two slots of the shared map and the subset's slot), labels by
    kind of particle -- claims both / discards all / claims one twice / claims the other -- half of the subset claims its slot;
    plus a third slot of the shared map to retire.  The slots are those most particles have in view (retire_first: the one most have in
    view is the one to retire, so that a slot only some have in view is one of the two the labels name)"""
    N = pk["xv"].shape[0]
    held, d2, fwd = _geometry(pk)
    with np.errstate(invalid="ignore"):
        seen = (held & (d2 < view_range ** 2) & (fwd > view_front)).sum(axis=0)[:nf]
    order = np.argsort(-seen, kind="stable")
    assert seen[order[2]] > N // 2, "fewer than three slots of the shared map in view: nothing to construct from (%s)" % seen
    a, b, r = (int(v) for v in (order[[1, 2, 0]] if retire_first else order[:3]))
    xv, xf = pk["xv"].astype(f64).mean(axis=0), np.nanmean(pk["xf"].astype(f64), axis=0)
    z = []
    for j in (a, b, nf):
        dx, dy = xf[j] - xv[:2]
        z.append([np.hypot(dx, dy), (np.arctan2(dy, dx) - xv[2] + np.pi) % (2 * np.pi) - np.pi])
    lab = np.full((N, 3), DISCARD, np.int32)
    kind = np.arange(N) % 4
    lab[kind == 0, 0], lab[kind == 0, 1] = a, b
    lab[kind == 2, 0], lab[kind == 2, 1] = a, a
    lab[kind == 3, 1] = b
    lab[A[::2], 2] = nf
    return np.array(z, f32), lab, r


def _split_view(pk, nf):
    """a view whose range boundary runs THROUGH the particle cloud: view_range at the 55th .. 98th percentile of the particles' distance
    to the farthest slot of the shared map that VIEW shows to everybody -- the candidate that leaves the fewest pairs undecided (chosen
    by the float64 model alone)"""
    held, d2, fwd = _geometry(pk)
    every = [j for j in range(nf) if np.all(held[:, j] & (d2[:, j] < VIEW[0] ** 2) & (fwd[:, j] > VIEW[1]))]
    j = max(every, key=lambda q: d2[:, q].mean())
    best = None
    for q in range(55, 99):
        R = float(f32(np.sqrt(np.percentile(d2[:, j], q))))
        undecided = int((np.abs(d2 - R * R) <= 1e-4 * R * R).any(axis=1).sum())
        if best is None or undecided < best[0]:
            best = (undecided, R)
    return (best[1], VIEW[1])


def _constructed_step(sg, method, math, logw, p_miss, retire=True, split=False):
    """the constructed state, the step's labels, (optionally) one slot retired, the feature set to p_miss and the view (None: the setter
    is never called), the step.  Returns the context and what the checks need"""
    s, (R, nf, A) = _constructed(sg, method, math, logw)
    pk = s.peek()
    view = _split_view(pk, nf) if split else VIEW
    z, lab, r = _step_labels(pk, nf, A, *view, retire_first=split)
    retired = (r,) if retire else ()
    if retire:
        s.retire_landmarks([r])
    if p_miss is not None:
        s.set_particle_miss(p_miss, *view)
    rep = s.update_labels(z, R, lab, new_share=0.0, p_new=0.05, census_every=1)
    assert rep["rewritten"] == 3 and rep["opened"] == 0, rep
    return s, dict(pk=pk, lab=lab, nf=nf, A=A, retired=retired, rep=rep, view=view)


# ---- 1. off and count-only are today's results -----------------------------------------------------------------------------------
@pytest.mark.parametrize("logw", [False, True], ids=["linear", "logw"])
@pytest.mark.parametrize("math", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("method", [2, 1], ids=["fs2", "fs1"])
def test_off_and_count_only_are_todays_results(sg, method, math, logw):
    """60 steps of example_webmap through update_particle (exhaustive) and run_particle (exhaustive, lists): never calling the setter,
    view_range = 0 and p_miss = 1 with the view on give bit-identical downloads, histories and reports; off: no particle_missed launch
    and nothing counted; on: one launch per step that had observations, and one run's counts on all three paths (a clean run
    this short misses next to nothing: the dense map below is where the paths' counts are compared in earnest)"""
    N, steps, K = 512, 60, 20
    c = _course("FASTSLAM2" if method == 2 else "FASTSLAM1", steps)
    settings = {"never": None, "range 0": (0.5, 0.0, 0.0), "count only": (1.0, c["max_range"] - 3.0, 3.0)}

    def run(path, setting):
        s = _ctx(sg, c, N, method, math, logw=logw)
        s.profile(True)
        if setting is not None:
            s.set_particle_miss(*setting)
        if path == "host":
            rep = np.array([_host_step(s, c, k, _opt(EXCL_ON, 1, 0.02, EXHAUSTIVE)) for k in range(steps)])
        else:
            for a in range(0, steps, K):
                s.run_particle(c["ctl"][a:a + K], c["Q"], c["dt"], c["xt"][a:a + K], c["max_range"], c["R"], noise=2,
                               **_opt(EXCL_ON, 1, 0.02, LISTS if path == "lists" else EXHAUSTIVE))
            rep = s.particle_report_fetch()
        missed, stats, launches = s.particle_missed(), s.particle_miss_stats(), s.kernel_time("particle_missed")[1]
        return _finish(s), rep, missed, stats, launches
    counted = {}
    for path in ("host", "exhaustive", "lists"):
        base, rep0, missed0, stats0, launches0 = run(path, None)
        with_obs = int((rep0[:, REPORT.index("need")] > 0).sum())
        assert with_obs == steps, "an iteration without observations: the launch count below would not be the steps'"
        assert launches0 == 0 and len(missed0) == 0 and not any(stats0.values()), (path, launches0, stats0)
        for tag in ("range 0", "count only"):
            got, rep, missed, stats, launches = run(path, settings[tag])
            assert np.array_equal(rep, rep0), (path, tag)
            _same_state(base, got, "%s, %s" % (path, tag))
            if tag == "range 0":
                assert launches == 0 and len(missed) == 0 and not any(stats.values()), (path, launches, stats)
            else:
                assert launches == with_obs and stats["steps"] == with_obs and len(missed) == N, (path, launches, stats)
                counted[path] = (missed, stats)
    print("particle_miss off / count only m%d math%d logw%d: %s" % (method, math, logw, {p: v[1] for p, v in counted.items()}))
    for path in ("exhaustive", "lists"):
        assert np.array_equal(counted[path][0], counted["host"][0]), path
        assert {k: v for k, v in counted[path][1].items() if k != "visited"} == {k: v for k, v in counted["host"][1].items() if k != "visited"}, path


# ---- 2. counts against the float64 model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,math,logw,split", [(2, 1, False, False), (1, 1, False, False), (2, 0, False, False), (1, 0, True, False),
                                                    (2, 1, False, True), (1, 0, False, True)], ids=lambda v: str(v))
def test_counts_match_the_float64_model(sg, method, math, logw, split):
    """the constructed step with the feature on: particle_missed equals the model for every particle whose pairs all clear; particles
    outside the subset never count the subset's slot; a retired slot counts for nobody; the statistics are the sums.  split: the view's
    range boundary runs through the particle cloud, so that one slot is in view of some particles and not of others"""
    s, k = _constructed_step(sg, method, math, logw, 0.5, split=split)
    VIEW = k["view"]
    got, stats = s.particle_missed(), s.particle_miss_stats()
    s.close()
    N, nf, A = len(got), k["nf"], k["A"]
    cnt, ok, inview = _model(k["pk"], k["lab"], *VIEW, retired=k["retired"])
    left_out = int((~ok).sum())
    rest = np.setdiff1d(np.arange(N), A)
    print("particle_miss counts m%d math%d logw%d view %s: left out %d of %d (cap %d); model counts %d..%d; device == model on %d of %d cleared; "
          "subset slot in view of %d of the subset; retired slot %d in view of %d; stats %s" %
          (method, math, logw, VIEW, left_out, N, N // 50, cnt.min(), cnt.max(), int((got[ok] == cnt[ok]).sum()), int(ok.sum()),
           int(inview[A, nf].sum()), k["retired"][0], int(inview[:, k["retired"][0]].sum()), stats))
    assert left_out <= 0.02 * N, "the inputs leave too many particles undecided: move VIEW"
    assert np.array_equal(got[ok], cnt[ok])
    # the cases the construction is there for, each non-trivially present
    assert inview[A, nf].sum() > len(A) // 2 and np.isnan(k["pk"]["xf"][rest, nf, 0]).all()      # the subset's slot: held by the subset only ...
    without_sub, _, _ = _model(k["pk"], np.where(k["lab"] == nf, DISCARD, k["lab"]), *VIEW, retired=tuple(k["retired"]) + (nf,))
    sel = ok & np.isin(np.arange(N), rest)
    assert np.array_equal(got[sel], without_sub[sel]), "a particle outside the subset counted the subset's slot"
    sel = ok & np.isin(np.arange(N), A[1::2]) & inview[:, nf]
    assert sel.any() and np.array_equal(got[sel], without_sub[sel] + 1), "an unclaimed subset slot in view is one miss"
    sel = ok & np.isin(np.arange(N), A[::2])
    assert np.array_equal(got[sel], without_sub[sel]), "a claimed slot is no miss"
    assert inview[:, k["retired"][0]].sum() > N // 2, "the retired slot is in nobody's view anyway"
    with_retired, _, _ = _model(k["pk"], k["lab"], *VIEW)
    assert (with_retired[ok] > cnt[ok]).any() and np.array_equal(got[ok], cnt[ok])                 # ... the retired slot counts for nobody
    kinds = np.arange(N) % 4
    assert len({int(np.median(cnt[ok & (kinds == q)])) for q in range(4)}) >= 2, "the labels made no difference to the counts"
    if split:
        part = inview[:, :nf].any(axis=0) & ~inview[:, :nf].all(axis=0)
        part[list(k["retired"])] = False
        assert part.any(), "no slot of the shared map that counts is in view of some particles only"
    assert stats["steps"] == 1
    if left_out == 0:
        assert stats["missed"] == int(cnt.sum()) and stats["particles"] == int((cnt > 0).sum())
    assert stats["missed"] == int(got.sum()) and stats["particles"] == int((got > 0).sum())


# ---- 3. weights -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logw", [False, True], ids=["linear", "logw"])
@pytest.mark.parametrize("math", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("method", [2, 1], ids=["fs2", "fs1"])
def test_weights_carry_the_factor_and_nothing_else_moves(sg, method, math, logw):
    """the same step from the same state, off and with p_miss = 0.5: poses, Pv and every record bit-identical; the weights differ by
    0.5^missed_i up to one constant (the normalisation) within (max missed + 8) 2^-23 -- one rounding per multiplication on each side
    plus the normalisation; 0.5^k is exact (log-weights: the same count of float32 roundings at the magnitude of l)"""
    off, _ = _constructed_step(sg, method, math, logw, None)
    on, _ = _constructed_step(sg, method, math, logw, 0.5)
    missed = on.particle_missed().astype(f64)
    a, b = off.download(), on.download()
    off.close()
    on.close()
    assert a["nf"] == b["nf"]
    for q in ("xv", "Pv", "xf", "Pf"):
        assert np.array_equal(a[q], b[q], equal_nan=True), q
    wa, wb = a["w"].astype(f64), b["w"].astype(f64)
    assert missed.max() >= 2 and missed.min() < missed.max(), "every particle missed the same number: the factor would be the constant"
    bound = (missed.max() + 8) * 2.0 ** -23
    if logw:
        cst = wb - wa - missed * np.log(0.5)
        spread, scale = cst.max() - cst.min(), max(np.abs(wa).max(), np.abs(wb).max())
        small = np.zeros(len(wa), bool)
    else:
        # (after 20 steps without a resample FastSLAM 1's most unlikely particles carry weights that are zero or subnormal in float32: a
        # relative rounding bound speaks of normal numbers only, so those are held to the format's absolute quantum 2^-149 per rounding)
        tiny = float(np.finfo(f32).tiny)
        small = (wa < tiny) | (wb < tiny)
        cst = (wb[~small] / wa[~small]) / 0.5 ** missed[~small]
        spread, scale = cst.max() - cst.min(), cst.min()
        expect = np.median(cst) * wa * 0.5 ** missed
        assert np.all(np.abs(wb[small] - expect[small]) <= bound * expect[small] + (missed[small] + 8) * 2.0 ** -149)
    print("particle_miss weights m%d math%d logw%d: missed %d..%d, constant %.9g, spread / scale %.3g, bound %.3g; %d of %d weights below float32's normal range" %
          (method, math, logw, missed.min(), missed.max(), cst.mean(), spread / scale, bound, int(small.sum()), len(wa)))
    assert small.sum() < len(wa) // 2
    assert spread <= bound * scale


# ---- 4. the same counts on every path ----------------------------------------------------------------------------------------------
def test_same_counts_on_every_path_and_the_boxes_prune(sg, tmp_path_factory):
    """config 5's map at MAX_RANGE 20, N = 4 096, 20 steps in count-only mode (one run on all three paths): per step, particle_missed of
    update_particle(EXHAUSTIVE), update_particle(LISTS) and run_particle(LISTS) is identical; with the lists' boxes a workgroup looks at
    far fewer records per particle than there are slots in use"""
    N, cap, steps = 4096, 960, 20
    c = _course_of(_synthetic(tmp_path_factory, 10000), "FASTSLAM2", steps, max_range=20)
    ex, li, dv = (_ctx(sg, c, N, 2, 1, cap) for _ in range(3))
    for s in (ex, li, dv):
        s.set_particle_miss(1.0, 17.0, 3.0)
    slots_looked_at_all = 0
    total = 0
    for k in range(steps):
        nf_before = li.nf()
        rex = _host_step(ex, c, k, _opt(EXCL_ON, 1, 0.02, EXHAUSTIVE))
        rli = _host_step(li, c, k, _opt(EXCL_ON, 1, 0.02, LISTS))
        dv.run_particle(c["ctl"][k:k + 1], c["Q"], c["dt"], c["xt"][k:k + 1], c["max_range"], c["R"], noise=2, **_opt(EXCL_ON, 1, 0.02, LISTS))
        assert rex[REPORT.index("need")] > 0, "a step without observations"
        a, b, d = ex.particle_missed(), li.particle_missed(), dv.particle_missed()
        assert len(a) == N and np.array_equal(a, b) and np.array_equal(a, d), (k, int((a != b).sum()), int((a != d).sum()))
        assert np.array_equal(rex, rli)
        slots_looked_at_all += nf_before
        total += int(a.sum())
    sx, sl, sd = ex.particle_miss_stats(), li.particle_miss_stats(), dv.particle_miss_stats()
    rdv = dv.particle_report_fetch()
    _same_state(_finish(ex), _finish(li), "exhaustive vs lists, count only")
    dv.close()
    print("particle_miss paths: %d steps, slots in use before the steps (summed) %d, missed in all %d; records looked at per particle: every slot %.1f, "
          "host lists %.1f, device lists %.1f" % (steps, slots_looked_at_all, total, sx["visited"] / N, sl["visited"] / N, sd["visited"] / N))
    assert len(rdv) == steps and total > 0
    for st in (sx, sl, sd):
        assert st["steps"] == steps and st["missed"] == total
    assert sx["visited"] <= N * slots_looked_at_all
    for st in (sl, sd):
        assert st["visited"] < sx["visited"] and st["visited"] < N * slots_looked_at_all


# ---- 5. it acts as intended --------------------------------------------------------------------------------------------------------
def test_share_of_the_subset_slot_falls_by_the_factor(sg):
    """(a) no resampling: with p_miss = 0.25 the subset's slot has share sum_subset w_off p^missed / sum_all w_off p^missed (float64, from
    the feature-off weights and the model's counts) within test 3's bound plus the summary's 8 N u, strictly below its share with the
    feature off"""
    p = 0.25
    off, k = _constructed_step(sg, 2, 1, False, None, retire=False)
    on, _ = _constructed_step(sg, 2, 1, False, p, retire=False)
    N, nf, A = 1024, k["nf"], k["A"]
    cnt, ok, _ = _model(k["pk"], k["lab"], *VIEW)
    got = on.particle_missed()
    assert (~ok).sum() <= 0.02 * N and np.array_equal(got[ok], cnt[ok])
    cnt = np.where(ok, cnt, got)  # (a particle the model cannot decide: the device's count)
    w = off.download()["w"].astype(f64) * p ** cnt.astype(f64)
    share_off = off.map_summary()["share"][nf]
    share_on, holders = on.map_summary()["share"][nf], on.map_summary()["holders"][nf]
    off.close()
    on.close()
    expect = w[A].sum() / w.sum()
    bound = (cnt.max() + 8) * 2.0 ** -23 + 8 * N * U53
    print("particle_miss share: off %.9g, on %.9g, expected %.9g, |on - expected| / expected %.3g (bound %.3g), holders %d" %
          (share_off, share_on, expect, abs(share_on - expect) / expect, bound, holders))
    assert holders == len(A)
    assert abs(share_on - expect) <= bound * expect
    assert share_on < share_off


def test_resampling_removes_the_holders_and_the_census_reclaims_the_slot(sg):
    """(b) a context that resamples every step (NEFFECTIVE N, Philox, one fixed seed), p_miss = 1e-6, census every step: a subset opens a
    slot, then steps whose only observation everybody discards keep it in the subset's view and unclaimed.  Within three steps the
    report shows the slot dead and the summary no holders; the same steps with the feature off leave it held.  (The context starts from
    an empty map, so the subset's slot is the only one anybody can miss: with a shared map of k slots in view and nothing claimed every
    weight would carry 1e-6^k, which float32 does not hold)"""
    N = 1024
    tape = _tape_of("FASTSLAM2", N, 40)
    A = np.arange(0, 300)

    def run(miss):
        s = sg.SlamGpu(N, 16, method=2, n_effective=N, rng_mode=sg.RNG_PHILOX, seed=3, math_mode=1, particle_maps=True)
        _predicts(s, tape["steps"][0], tape)
        lab = np.full((N, 1), DISCARD, np.int32)
        lab[A, 0] = NEW
        rep = s.update_labels(np.array([Z_SUB], f32), tape["R"], lab, new_share=0.0, p_new=1.0, census_every=1)
        assert rep["opened"] == 1 and rep["slots"] == 1, rep
        if miss:
            s.set_particle_miss(1e-6, *VIEW)
        out = []
        for _ in range(3):
            pk = s.peek()
            rep = s.update_labels(np.array([[30.0, -0.8]], f32), tape["R"], np.full((N, 1), DISCARD, np.int32), new_share=0.0, p_new=1.0, census_every=1)
            cnt, ok, inview = _model(pk, np.full((N, 1), DISCARD, np.int32), *VIEW)
            out.append((rep["dead"], int(s.map_summary(0, 1)["holders"][0]), int((~np.isnan(pk["xf"][:, 0, 0])).sum()), int(inview[:, 0].sum()),
                        s.particle_missed() if miss else None, cnt, ok))
        assert s.status() == 0
        s.close()
        return out
    on, off = run(True), run(False)
    print("particle_miss census: (dead, holders after, holders before, of them in view) per step: on %s, off %s" %
          ([o[:4] for o in on], [o[:4] for o in off]))
    dead, holders_after, holders_before, seen, got, cnt, ok = on[0]
    assert holders_before > 200 and seen == holders_before, "the slot is not in its holders' view"
    assert ok.all() and np.array_equal(got, cnt) and got.sum() == holders_before
    assert on[-1][0] >= 1 and on[-1][1] == 0, "the slot was not reclaimed within three steps"
    assert all(o[0] == 0 and o[1] > 0 for o in off), "the slot died without the feature"


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(sg):
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, rng_mode=sg.RNG_PHILOX, particle_maps=True)
    assert len(s.particle_missed()) == 0 and not any(s.particle_miss_stats().values())
    for bad in ((0.0, 20.0, 1.0), (-0.5, 20.0, 1.0), (1.5, 20.0, 1.0), (0.5, -1.0, 1.0), (0.5, 20.0, -1.0), (np.nan, 20.0, 1.0), (0.5, np.nan, 1.0),
                (0.5, 20.0, np.nan), (np.inf, 20.0, 1.0), (0.5, np.inf, 1.0), (0.5, 20.0, np.inf), (np.nan, 0.0, 0.0), (0.5, 0.0, np.inf)):
        with pytest.raises(sg.SlamGpuError) as e:
            s.set_particle_miss(*bad)
        assert e.value.code == ERR_INVALID, bad
    for good in ((0.5, 20.0, 0.0), (1.0, 20.0, 3.0), (1e-6, 0.5, 0.25), (0.5, 0.0, 0.0)):
        s.set_particle_miss(*good)
    assert len(s.particle_missed()) == 0
    s.close()
    s = sg.SlamGpu(256, 16, method=sg.FASTSLAM1, rng_mode=sg.RNG_PHILOX)
    with pytest.raises(sg.SlamGpuError) as e:
        s.set_particle_miss(0.5, 20.0, 1.0)
    assert e.value.code == ERR_INVALID and "SLAMGPU_FLAG_PARTICLE_MAPS" in str(e.value)
    s.close()


# ---- 7. slam-backend ---------------------------------------------------------------------------------------------------------------
def test_slam_backend_count_only_prints_todays_run_and_the_statistics():
    def run(extra):
        r = subprocess.run([EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-NPARTICLES", "512", "-NEFFECTIVE", "384",
                            "-SWITCH_SEED_RANDOM", "7", "-assoc", "particle", "-observe", "device", "-rng", "philox", "-maxsteps", "2000", *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        # (the lines that quote wall-clock times differ from run to run by their nature)
        return [re.sub(r"-?\d+\.\d+ us", "T us", re.sub(r"= \d+ % of", "= T % of", ln)) for ln in r.stdout.splitlines()]
    plain = run(())
    miss = run(("-PARTICLE_MISS", "1", "-PARTICLE_MISS_MARGIN", "3"))
    line = [ln for ln in miss if ln.startswith("negative information:")]
    assert len(line) == 1 and not any(ln.startswith("negative information:") for ln in plain)
    # (the settings echoed at the top name the two keys; everything else is the run without them)
    assert [ln for ln in miss if "PARTICLE_MISS" not in ln and not ln.startswith("negative information:")] == [ln for ln in plain if "PARTICLE_MISS" not in ln]
    m = re.match(r"negative information: (\d+) steps, (\d+) held landmarks in view and unmatched \(summed over particles and steps\), (\d+) particles with one or more$", line[0])
    print("slam-backend -PARTICLE_MISS 1 -PARTICLE_MISS_MARGIN 3:", line[0])
    assert m and int(m.group(1)) > 0 and int(m.group(2)) >= int(m.group(3))
