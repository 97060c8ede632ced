"""Local periods of the device EKF (include/slamgpu.h: slamgpu_ekf_local_*; slam_amd/csrc/ekf_local.cpp) on the GPU.
The reference is the float64 full EkfModel (tests/ekf_model.py) with the device's chunks of 64 observations, the yardstick the full device filter -- the same handle type without
a period -- from the same uploaded state and the same stage calls, and the rule the one of tests/test_gpu_ekf.py: the local filter's
error is at most max(4 x the full device filter's error, 8 * 2^-24), x relative to max |x| and P relative to max |P|.  The factor was
fixed before anything was measured; the measured ratios are in profiles/ekf_local.txt (worst 1.00; with psi kept in float32 the
shapes with a passive part and more than one active feature missed the rule at 9 .. 36, which is why the library sums psi in float64).
  1. a period without a stage changes no bit;  2. equivalence over shapes on both sides of the lane, panel and tile edges;  3. a period
  of predicts;  4. two periods in a row;  5. the gates and sim inside a period;  6. the contract;  7. slam-backend -EKF_LOCAL."""
import os
import subprocess

import numpy as np
import pytest

import ekf_local_model as LM
from conftest import DATA, bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
FLOOR = 8.0 * 2.0 ** -24
FACTOR = 4.0
SENTINEL = f32(777.25)
ROOT = os.path.dirname(DATA)


def make_dev(max_landmarks, **kw):
    import slam_amd
    return slam_amd.EkfGpu(max_landmarks, **dict(LM.CONF, **kw))


def errors(x, P, xm, Pm):
    return float(np.abs(x - xm).max() / np.abs(xm).max()), float(np.abs(P - Pm).max() / np.abs(Pm).max())


def within(dev, ref):
    return dev <= max(FACTOR * ref, FLOOR)


def symmetric(P):
    return bits_equal(P, P.T.copy())


def features_of(nf, k, rng):
    """k features, ascending, the first and the last of the map among them"""
    if k >= nf:
        return np.arange(nf)
    ends = [nf - 1] if k == 1 else [0, nf - 1][:k]
    rest = rng.permutation(np.arange(1, nf - 1))[:k - len(ends)]
    return np.sort(np.concatenate([ends, rest]).astype(np.int64))


def run_both(tag, x0, P0, periods, heading, seed, cap, out=None):
    """the script on a local and on a full device filter; the 4 x rule, symmetry and the dimension after the last commit.  A dict
    `out` is given the script, the model and the full device filter's state before the rule is asserted"""
    script, ref = LM.build_script(x0, P0, periods, heading, seed)
    loc, full = (make_dev(cap, use_heading=heading, association_known=True) for _ in range(2))
    for d in (loc, full):
        d.upload(x0, P0)
    LM.drive(loc, script)
    LM.drive(full, script, periods=False)
    info = loc.local_info()
    assert loc.dim == full.dim == ref.dim and info["open"] == 0 and info["commits"] == len(periods)
    (xl, Pl), (xf, Pf) = loc.state(), full.state()
    assert loc.status() == 0 and full.status() == 0
    loc.close()
    full.close()
    assert symmetric(Pl) and symmetric(Pf)
    lx, lP = errors(xl, Pl, ref.x, ref.P)
    fx, fP = errors(xf, Pf, ref.x, ref.P)
    if out is not None:
        out.update(script=script, ref=ref, local=(xl, Pl), full=(xf, Pf))
    print("EKF local %s: dim %d, local x %.3e P %.3e, full device x %.3e P %.3e, ratio x %.3f P %.3f" %
          (tag, ref.dim, lx, lP, fx, fP, lx / max(fx, FLOOR / FACTOR), lP / max(fP, FLOOR / FACTOR)))
    assert within(lx, fx) and within(lP, fP), (lx, fx, lP, fP)
    return xl, Pl


# ---- 1. a period without a stage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,k", [(63, 0), (64, 15), (130, 70), (63, 63)])
def test_noop_period_changes_no_bit(nf, k):
    x0, P0 = LM.synthetic_state(nf, 31 * nf + k)
    D, cap = 3 + 2 * nf, 3 + 2 * (nf + 2)
    d = make_dev(nf + 2)
    d.upload(np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))  # what lies beyond dim must stay as it was uploaded
    d.upload(x0, P0)
    feats = features_of(nf, k, np.random.default_rng(k))
    with d.local(feats, 2):
        info = d.local_info()
        assert info == dict(open=1, k=k, new=0, max_new=2, calls=0, commits=0) and d.dim == D
    x, P = d.state()
    assert bits_equal(x, x0) and bits_equal(P, P0)
    full = d.block(np.arange(cap, dtype=np.int32))
    assert bits_equal(full[:D, :D], P0) and (full[D:, :] == SENTINEL).all() and (full[:, D:] == SENTINEL).all()
    assert d.local_info()["commits"] == 1
    d.close()


# ---- 2. equivalence over shapes -----------------------------------------------------------------------------------------------------------
# nf, k (na0 = 3 + 2 k: 3, 5, 31, 33, 127, 129, 143), use_heading, steps, observations per step, features created per step
SHAPES = [(63, 0, True, 4, 0, [1]), (64, 1, False, 3, 1, []), (128, 14, True, 4, 10, [0, 3]), (130, 15, False, 5, 15, [1]),
          (128, 62, True, 3, 40, []), (130, 63, False, 4, 63, [0, 1]), (130, 70, True, 3, 65, [3]), (63, 63, True, 4, 30, [1]),
          (64, 64, False, 3, 64, [])]


@pytest.mark.parametrize("nf,k,heading,steps,m,new", SHAPES)
def test_local_period_matches_the_full_filter(nf, k, heading, steps, m, new):
    rng = np.random.default_rng(100 * nf + k)
    x0, P0 = LM.synthetic_state(nf, 7 * nf + k)
    feats = features_of(nf, k, rng)
    assert feats.shape[0] == k and (k < 2 or (feats[0] == 0 and feats[-1] == nf - 1))
    periods = [dict(features=feats, max_new=sum(new), steps=steps, m=m, new=new)]
    run_both("shape nf %d k %d heading %d m %d new %s" % (nf, k, heading, m, new), x0, P0, periods, heading, 9 * nf + k, nf + sum(new))


# ---- 3. a period of predicts ----------------------------------------------------------------------------------------------------------------
def test_predict_only_period_moves_the_passive_cross_covariance():
    nf = 130
    x0, P0 = LM.synthetic_state(nf, 5)
    feats = features_of(nf, 15, np.random.default_rng(5))
    _, P = run_both("predicts only", x0, P0, [dict(features=feats, steps=5, m=0)], False, 3, nf)
    passive = np.setdiff1d(np.arange(nf), feats)
    cols = 3 + 2 * passive
    assert (P[:2, cols] != P0[:2, cols]).mean() > 0.9 and bits_equal(P[2, cols], P0[2, cols])       # Gv moves the x and y rows, not the heading's
    assert bits_equal(P[np.ix_(cols, cols)], P0[np.ix_(cols, cols)])                          # psi = 0: P[B, B] stays


# ---- 4. two periods in a row ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heading", [False, True])
def test_two_periods_in_a_row(heading):
    nf = 128
    x0, P0 = LM.synthetic_state(nf, 77)
    rng = np.random.default_rng(8)
    first = features_of(nf, 14, rng)
    second = np.sort(np.concatenate([rng.permutation(np.arange(1, nf - 1))[:20], [nf, nf + 1, nf + 2]]))  # three of them made by the first
    periods = [dict(features=first, max_new=3, steps=4, m=8, new=[1, 2]), dict(features=second, max_new=2, steps=4, m=12, new=[0, 1])]
    run_both("two periods heading %d" % heading, x0, P0, periods, heading, 21, nf + 4)


# ---- 5. the gates, and sim inside a period --------------------------------------------------------------------------------------------------
def gate_scene():
    """40 landmarks on a ring of 40 .. 50 m, 4 m and more apart; features 5 .. 24 active, the passive ones 20 m and more from every
    observation; two observations of new landmarks 10 m from the pose"""
    nf = 40
    x0, P0 = LM.synthetic_state(nf, 12, spread=2.0)
    P0 = (P0 * f32(0.05)).astype(f32)  # tight: a neighbour 4 m away is far outside the augment gate
    P0 = np.tril(P0) + np.tril(P0, -1).T
    return nf, x0, P0, np.arange(5, 25), np.array([8, 11, 12, 15, 19, 21])


@pytest.mark.parametrize("heading", [False, True])
def test_gates_inside_a_period(heading):
    import ekf_model
    nf, x0, P0, active, seen = gate_scene()
    rng = np.random.default_rng(3)
    kw = dict(use_heading=heading, association_known=False)
    mdl = ekf_model.EkfModel(**dict(LM.CONF, **kw))
    mdl.upload(x0, P0)
    loc, full, sim = (make_dev(nf + 2, **kw) for _ in range(3))
    for d in (loc, full, sim):
        d.upload(x0, P0)
    loc.local_begin(active, 2)
    sim.local_begin(active, 2)
    z = np.concatenate([LM.observations(x0, seen, rng, noise=0.3), np.array([[10.0, 2.0], [11.0, -2.4]], f32)])  # ... and two new landmarks
    for step in range(2):
        ctl = (3.0, float(f32(0.04)), LM.Q, LM.DT)
        phi = float(f32(mdl.x[2] + 0.002))
        for f in (mdl, loc, full):
            f.predict(*ctl)
            if heading:
                f.observe_heading(phi)
        want, margin = mdl.associate(z, LM.R, want_margin=True)
        assert margin.min() >= 1e-2, margin
        got_l, got_f = loc.associate(z, LM.R), full.associate(z, LM.R)
        assert np.array_equal(got_l, want) and np.array_equal(got_f, want), (step, got_l, got_f, want)
        if step == 0:
            assert np.array_equal(want, np.concatenate([seen, [-1, -1]]))
        else:
            assert np.array_equal(want, np.concatenate([seen, [nf, nf + 1]]))  # the features the period created, by their global indices
        for f in (mdl, loc, full):
            f.update(z[want >= 0], want[want >= 0], LM.R)
            f.augment(z[want == -1], LM.R)
        sim.sim(*ctl, phi, z, None, LM.R, LM.R, 1)
        pa, pb = loc.pose(), sim.pose()
        assert bits_equal(pa[0], pb[0]) and bits_equal(pa[1], pb[1])
        # the next step sees the same landmarks again, the two new ones included, from the pose the model has now
        z = LM.observations(mdl.x, np.concatenate([seen, [nf, nf + 1]]), rng, noise=0.3)
    assert loc.local_info() == dict(open=1, k=20, new=2, max_new=2, calls=8 + 2 * heading, commits=0)
    assert sim.local_info()["calls"] == 2
    loc.local_end()
    sim.local_end()
    (xl, Pl), (xs, Ps), (xf, Pf) = loc.state(), sim.state(), full.state()
    assert bits_equal(xl, xs) and bits_equal(Pl, Ps)  # sim == the stages one by one, inside a period too
    assert symmetric(Pl) and loc.dim == full.dim == mdl.dim
    lx, lP = errors(xl, Pl, mdl.x, mdl.P)
    fx, fP = errors(xf, Pf, mdl.x, mdl.P)
    print("EKF local gates heading %d: local x %.3e P %.3e, full device x %.3e P %.3e, ratio x %.3f P %.3f" %
          (heading, lx, lP, fx, fP, lx / max(fx, FLOOR / FACTOR), lP / max(fP, FLOOR / FACTOR)))
    assert within(lx, fx) and within(lP, fP), (lx, fx, lP, fP)
    for d in (loc, full, sim):
        d.close()


# ---- 6. the contract ------------------------------------------------------------------------------------------------------------------------
def test_contract():
    import slam_amd
    nf = 12
    x0, P0 = LM.synthetic_state(nf, 2)
    rng = np.random.default_rng(1)
    a, twin = (make_dev(nf + 3, use_heading=True, association_known=True) for _ in range(2))
    for d in (a, twin):
        d.upload(x0, P0)
    ctl = (3.0, float(f32(0.05)), LM.Q, LM.DT)
    feats = np.array([1, 4, 5, 9], np.int32)
    z = LM.observations(x0, [4, 9], rng)

    def refused(call, code=-1):
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            call()
        assert ei.value.code == code, ei.value

    refused(a.local_end)                                               # no period open
    for bad in ([4, 1], [1, 1], [nf], [-1]):
        refused(lambda: a.local_begin(bad, 0))
    refused(lambda: a.local_begin(feats, -1))
    assert a.local_info() == dict(open=0, k=0, new=0, max_new=0, calls=0, commits=0)
    assert np.array_equal(a.lookup([0, nf - 1, nf, 500, -3]), [0, nf - 1, -1, -1, -1])
    for d in (a, twin):
        d.local_begin(feats, 1)
        d.predict(*ctl)
        d.update(z, [4, 9], LM.R)
    # each of these is refused and changes nothing
    refused(lambda: a.local_begin(feats, 1))
    refused(lambda: a.update(z[:1], [0], LM.R))                        # a passive feature
    refused(lambda: a.update(z, [4, nf], LM.R))                        # a feature that does not exist
    refused(lambda: a.sim(*ctl, 0.1, z, [4, 3], LM.R, LM.R, 1))        # the known association: id 3 is feature 3, passive; before the predict
    refused(a.state)
    refused(lambda: a.block([0, 1]))
    refused(lambda: a.upload(x0, P0))
    assert a.dim == 3 + 2 * nf and a.local_info()["calls"] == 2
    for d in (a, twin):
        d.augment([[15.0, 0.3]], LM.R)
    assert a.dim == 3 + 2 * (nf + 1) and a.local_info()["new"] == 1
    refused(lambda: a.augment([[16.0, 1.3]], LM.R), -3)                 # max_new: SLAMGPU_ERR_CAPACITY, the period stays usable
    refused(lambda: a.sim(*ctl, 0.1, z, [4, 700], LM.R, LM.R, 1), -3)   # ... in sim with a new id, before the predict
    assert a.local_info() == dict(open=1, k=4, new=1, max_new=1, calls=3, commits=0)
    assert np.array_equal(a.lookup([4, 700]), [4, -1])
    for d in (a, twin):
        d.sim(*ctl, 0.1, z, [4, 9], LM.R, LM.R, 1)
        d.local_end()
    (xa, Pa), (xt, Pt) = a.state(), twin.state()
    assert bits_equal(xa, xt) and bits_equal(Pa, Pt) and symmetric(Pa) and xa.shape[0] == 3 + 2 * (nf + 1)
    assert a.local_info() == dict(open=0, k=0, new=0, max_new=0, calls=0, commits=1)
    # destroy with an open period discards it
    twin.local_begin([0], 0)
    twin.predict(*ctl)
    twin.close()
    a.close()


# ---- 7. slam-backend ------------------------------------------------------------------------------------------------------------------------
def test_backend_local_periods_print_the_same_run(tmp_path):
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")

    def run(*extra):
        r = subprocess.run([exe, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "EKF1", "-ekf", "device", "-SWITCH_SEED_RANDOM", "7",
                            "-SWITCH_ASSOCIATION_KNOWN", "1", "-maxsteps", "4000", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        lines = r.stdout.splitlines()
        final = [ln for ln in lines if "final estimate" in ln][0]
        return final[final.index("final estimate"):], [ln for ln in lines if ln.startswith("landmarks in map:")][0]
    fa, ma = run()
    fb, mb = run("-EKF_LOCAL", "20")
    print("slam-backend: %s | %s || -EKF_LOCAL 20: %s | %s" % (fa, ma, fb, mb))
    assert "commits" in mb and "commits" not in ma and int(mb.split()[-2]) >= 2
    assert mb.split()[3] == ma.split()[3] and int(ma.split()[3]) >= 10
    assert fa == fb
