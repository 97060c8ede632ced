"""Local periods of the device EKF (slam_amd/csrc/ekf_local.cpp) past ONE workgroup of its launches, over several chunks per update, on
buffers an earlier period left behind, with room a period does not use, and through a chunk that does not factorise.  The conventions
are tests/test_gpu_ekf_local.py's: the reference is the float64 full EkfModel with the device's chunks of 64 (tests/ekf_model.py), the
yardstick the full device filter -- no period -- given the same uploaded state and the same stage calls, the rule
local <= max(4 x yardstick, 8 * 2^-24).  Here the rule is held over the whole state (x relative to max |x|, P to max |P|) AND per block:
P[A,A], P[A,B], P[B,B], x_A, x_B (A: the pose, the period's features and those it created; B: the rest), each relative to the
model's largest magnitude in that block, so that a wrong tile of a block with small entries cannot hide below max |P|.  The measured
ratios are in profiles/ekf_local.txt, section 5.
  1. shapes past 256 (grid x extent of a launch: its lanes / 256, workgroups of 256 lanes):
       nf 255 k 126: na0 255, dimA 255 -> 257 through a created feature: ekf_local_scatter_kernel's second workgroup carries ONE lane,
                     ekf_local_ab_kernel has 3 row tiles; nB 258: ekf_local_t_kernel and ekf_local_xb_kernel have a second workgroup of
                     TWO lanes, ekf_local_bb_kernel a fifth tile 2 wide; updates of 70, 71, 71 observations: two chunks
       nf 255 k 127: na0 257: ekf_local_augment_kernel and ekf_local_psi_heading_kernel have a second workgroup of ONE lane,
                     ekf_local_psi_chunk_kernel 9 x 9 tiles, the last of one row; nB 256: NO tail in t, xb, bb; updates of 127, 127,
                     129 observations: the last chunk holds one, n = 2
       nf 300 k 0:   na0 3, nB 600: K = 3 is below the k step of both products of the commit; bb has 10 x 10 tiles, t and xb three
                     workgroups; the only updates are of the two features the period created
       nf 260 k 260: nB 0: the commit is the scatter alone (three workgroups a row); na0 523, M 1 048 wide: three workgroups of
                     augment and psi_heading, 17 x 17 tiles of psi_chunk; updates of 150 and 151 observations: three chunks
       nf 400 k 200: na0 403, nB 400: second workgroups of every launch above at once, three chunks each update; the period ends with
                     room for two features unused (max_new 5, three created)
  2. the gates inside a period of 300 and of 343 features (ekf_gate_kernel's `j += 256`, then ekf_local_labels' local -> global) on the
     packet of tests/test_gpu_ekf_scale.py, the float64 local model's labels and margins deciding; the caps of the packet are checked on
     the CPU as well (tests/test_ekf_cpu.py); the odd-feature period then applies its labels and is held to the rule;
  3. bit for bit: a small period after a large one on the same handle (every grow-only buffer reused smaller, under stale contents)
     against a fresh handle; one script under three layouts of M (max_new 2, 9 and 1 000 000 clamped by the handle's capacity);
  4. a chunk without a Cholesky factor inside a period: alone (nothing changes, the commit included), and behind a good chunk of the
     same update (psi must not take the good chunk's W1 a second time)."""
import numpy as np
import pytest

import ekf_local_model as LM
import ekf_model
from conftest import bits_equal
from test_gpu_ekf_local import FACTOR, FLOOR, errors, features_of, make_dev, run_both, symmetric, within
from test_gpu_ekf_scale import CLEAR, GATES, NEW, RE, study

pytestmark = pytest.mark.gpu
f32 = np.float32


def ratio(dev, ref):
    return dev / max(ref, FLOOR / FACTOR)


def held_per_block(tag, loc, full, ref, A, B, only=LM.BLOCKS):
    """the rule on each block in `only` (all five: the figures of every block are printed first).  loc, full: (x, P); ref: the model"""
    el, ef = (LM.block_errors(x, P, ref.x, ref.P, A, B) for x, P in (loc, full))
    print("EKF local blocks %s: |A| %d |B| %d, " % (tag, A.shape[0], B.shape[0]) +
          ", ".join("%s local %.3e full device %.3e ratio %.3f" % (b, el[b], ef[b], ratio(el[b], ef[b])) for b in LM.BLOCKS if b in el))
    missed = {b: (el[b], ef[b]) for b in only if b in el and not within(el[b], ef[b])}
    assert not missed, (tag, missed)


# ---- 1. shapes past 256 -----------------------------------------------------------------------------------------------------------------
# nf, k, use_heading, steps, observations per step, features created per step, max_new
SCALE_SHAPES = [(255, 126, False, 3, 70, [1], 1), (255, 127, True, 3, 130, [0, 2], 2), (300, 0, True, 4, 0, [2], 2),
                (260, 260, True, 2, 150, [1], 1), (400, 200, True, 3, 130, [1, 0, 2], 5)]


@pytest.mark.parametrize("nf,k,heading,steps,m,new,max_new", SCALE_SHAPES)
def test_local_period_past_256(nf, k, heading, steps, m, new, max_new):
    rng = np.random.default_rng(100 * nf + k)
    x0, P0 = LM.synthetic_state(nf, 7 * nf + k)
    feats = features_of(nf, k, rng)
    assert feats.shape[0] == k and (k < 2 or (feats[0] == 0 and feats[-1] == nf - 1))
    periods = [dict(features=feats, max_new=max_new, steps=steps, m=m, new=new)]
    tag = "shape nf %d k %d heading %d m %d new %s max_new %d" % (nf, k, heading, m, new, max_new)
    out = {}
    try:
        run_both(tag, x0, P0, periods, heading, 9 * nf + k, nf + max_new, out=out)  # status, symmetry, dim, open, commits; the rule on x and P
    finally:
        if out:
            ref = out["ref"]
            A, B = LM.blocks_of(out["script"], x0.shape[0], ref.dim)
            assert A.shape[0] == 3 + 2 * (k + sum(new)) and B.shape[0] == 2 * (nf - k)
            held_per_block(tag, out["local"], out["full"], ref, A, B)


# ---- 2. the gates past one pass of lanes, inside a period -------------------------------------------------------------------------------
PERIODS = {"odd": np.arange(1, 600, 2), "tail": np.arange(257, 600)}
MAX_NEW = 8
_period = {}


def period_study(which):
    """study(600)'s state and packet, gated by the float64 LOCAL model inside a period of PERIODS[which]: labels (global), margins, the
    local index of every match, and the full map's labels for the same readings.  Computed once (no GPU: tests/test_ekf_cpu.py runs it)"""
    if which not in _period:
        s = study(600)
        feats = PERIODS[which]
        mdl = LM.EkfLocalModel(**GATES)
        mdl.upload(s["x0"], s["P0"])
        mdl.local_begin(feats, MAX_NEW)
        lab, margin = mdl.associate(s["z"], RE, want_margin=True)
        local = np.where(lab >= 0, np.searchsorted(feats, np.maximum(lab, 0)), -1)
        assert np.array_equal(feats[local[lab >= 0]], lab[lab >= 0])  # every match is a feature of the period
        _period[which] = dict(s, which=which, feats=feats, lab=lab, margin=margin, clear=margin > CLEAR, local=local, full_lab=s["lab"])
    return _period[which]


def period_caps(p):
    """the conditions of a period's 64 decisions: at most 2 unclear; at least 40 (odd features) or 30 (257 .. 599) matches; at least 5
    winners at a local index of 256 or more; at least 20 labels that are not the full map's label for the same reading (the period
    answered, not the map); in the odd-feature period, whose labels are applied, no more new landmarks than it has room for.  Returns
    (matches, past 256, differing)"""
    lab, clear = p["lab"], p["clear"]
    matches, past, differ = int((lab >= 0).sum()), int((p["local"] >= 256).sum()), int((lab != p["full_lab"]).sum())
    assert int((~clear).sum()) <= 2, (p["which"], p["margin"])
    assert matches >= (40 if p["which"] == "odd" else 30) and past >= 5 and differ >= 20, (p["which"], matches, past, differ)
    if p["which"] == "odd":
        assert 1 <= int((lab == NEW).sum()) <= MAX_NEW
    return matches, past, differ


@pytest.mark.parametrize("which", ["odd", "tail"])
def test_gates_past_one_pass_of_lanes_inside_a_period(which):
    """k 300 and 343: every lane of ekf_gate_kernel holds one or two active features, and a winner past local index 255 has to be
    translated by ekf_local_labels.  The odd-feature period then applies the model's labels with explicit update and augment calls, ends,
    and is held to the rule with a full device filter given the same calls as the yardstick"""
    p = period_study(which)
    matches, past, differ = period_caps(p)
    x0, P0, z, lab, clear, feats = p["x0"], p["P0"], p["z"], p["lab"], p["clear"], p["feats"]
    nn = int((lab == NEW).sum())
    loc = make_dev(600 + MAX_NEW, **GATES)
    loc.upload(x0, P0)
    loc.local_begin(feats, MAX_NEW)
    got = loc.associate(z, RE)
    print("EKF local gates in a period of %s features (k %d): checked %d skipped %d, match / new / discard %d / %d / %d, winners at a local index >= 256: %d, "
          "labels that differ from the full map's: %d, smallest margin %.2e" % (which, feats.shape[0], clear.sum(), (~clear).sum(), matches, nn,
                                                                                  (lab == ekf_model.ASSOC_DISCARD).sum(), past, differ, p["margin"].min()))
    assert np.array_equal(got[clear], lab[clear]), (got, lab, p["margin"])
    assert loc.local_info() == dict(open=1, k=feats.shape[0], new=0, max_new=MAX_NEW, calls=1, commits=0)
    if which != "odd":
        loc.local_end()
        x, P = loc.state()
        assert loc.status() == 0 and symmetric(P) and loc.dim == x0.shape[0]
        loc.close()
        return
    full = make_dev(600 + MAX_NEW, **GATES)
    full.upload(x0, P0)
    ref = ekf_model.EkfModel(chunk=LM.CHUNK, **GATES)
    ref.upload(x0, P0)
    for f in (ref, loc, full):
        f.update(z[lab >= 0], lab[lab >= 0], RE)
        f.augment(z[lab == NEW], RE)
    assert loc.local_info() == dict(open=1, k=300, new=nn, max_new=MAX_NEW, calls=3, commits=0)
    loc.local_end()
    (xl, Pl), (xf, Pf) = loc.state(), full.state()
    assert loc.status() == 0 and full.status() == 0 and loc.dim == full.dim == ref.dim == x0.shape[0] + 2 * nn
    assert loc.local_info() == dict(open=0, k=0, new=0, max_new=0, calls=0, commits=1)
    loc.close()
    full.close()
    assert symmetric(Pl) and symmetric(Pf)
    lx, lP = errors(xl, Pl, ref.x, ref.P)
    fx, fP = errors(xf, Pf, ref.x, ref.P)
    print("EKF local gated period of odd features, %d matched %d new: dim %d, local x %.3e P %.3e, full device x %.3e P %.3e, ratio x %.3f P %.3f" %
          (matches, nn, ref.dim, lx, lP, fx, fP, ratio(lx, fx), ratio(lP, fP)))
    assert within(lx, fx) and within(lP, fP), (lx, fx, lP, fP)


# ---- 3. bit for bit ---------------------------------------------------------------------------------------------------------------------
def test_a_small_period_after_a_large_one_leaves_the_same_bits():
    """M, Y, T, psi, PHt, W1, cw and the index maps only grow, and W1 is zeroed only when it grows.  A handle that ran a period of
    na0 203 on 200 landmarks is uploaded a 40-landmark state and runs a period of na0 27: ld, ldY, off and all three maps are smaller
    than what the buffers hold.  A fresh handle of the same capacity, given the upload and the small period only, leaves the same bits;
    so does the first handle when it does both once more"""
    cap = 201
    xb, Pb = LM.synthetic_state(200, 1400)
    big, _ = LM.build_script(xb, Pb, [dict(features=features_of(200, 100, np.random.default_rng(20)), max_new=1, steps=2, m=70, new=[1])], True, 1800)
    xs, Ps = LM.synthetic_state(40, 280)
    small, ref = LM.build_script(xs, Ps, [dict(features=features_of(40, 12, np.random.default_rng(4)), max_new=1, steps=3, m=8, new=[1])], True, 360)
    used, fresh = (make_dev(cap, use_heading=True, association_known=True) for _ in range(2))
    used.upload(xb, Pb)
    LM.drive(used, big)
    assert used.dim == 3 + 2 * 201 and used.status() == 0

    def small_period(d):
        d.upload(xs, Ps)
        LM.drive(d, small)
        return d.state()
    (x1, P1), (x0, P0), (x2, P2) = small_period(used), small_period(fresh), small_period(used)
    assert used.status() == 0 and fresh.status() == 0 and used.dim == fresh.dim == ref.dim == 3 + 2 * 41
    assert used.local_info() == dict(open=0, k=0, new=0, max_new=0, calls=0, commits=3) and fresh.local_info()["commits"] == 1
    used.close()
    fresh.close()
    assert symmetric(P0) and not bits_equal(P0[:83, :83], Ps) and np.isfinite(P0).all()
    assert bits_equal(x1, x0) and bits_equal(P1, P0)
    assert bits_equal(x2, x0) and bits_equal(P2, P0)


def test_the_layout_of_the_gap_changes_no_bit():
    """nf 100, k 60, heading observed, new [0, 2]: na0 123, dimA 123 -> 127.  max_new 2: the carried entries start at off 127 and the gap
    closes; max_new 9: off 141, beyond the 128 tile edge, and 14 entries of the gap stay (zero, apart from the heading update's eps on
    their diagonal); max_new 1 000 000 on a handle with room for four: the clamp decides, off 131.  Every stage is elementwise in
    position and the rank update a k-ordered chain per element, so the three states are equal bit for bit"""
    nf, k = 100, 60
    x0, P0 = LM.synthetic_state(nf, 7 * nf + k)
    feats = features_of(nf, k, np.random.default_rng(100 * nf + k))
    script, ref = LM.build_script(x0, P0, [dict(features=feats, max_new=2, steps=3, m=40, new=[0, 2])], True, 9 * nf + k)
    assert script[0][0] == "begin" and script[-1][0] == "end"
    states = []
    for max_new, cap in ((2, nf + 9), (9, nf + 9), (1000000, nf + 4)):
        d = make_dev(cap, use_heading=True, association_known=True)
        d.upload(x0, P0)
        d.local_begin(feats.astype(np.int32), max_new)
        assert d.local_info() == dict(open=1, k=k, new=0, max_new=max_new, calls=0, commits=0)
        LM.drive(d, script[1:-1])
        assert d.local_info() == dict(open=1, k=k, new=2, max_new=max_new, calls=len(script) - 2, commits=0)
        d.local_end()
        states.append(d.state())
        assert d.status() == 0 and d.dim == ref.dim == 3 + 2 * (nf + 2) and d.local_info()["commits"] == 1
        d.close()
    (xa, Pa), (xb, Pb), (xc, Pc) = states
    assert symmetric(Pa) and max(errors(xa, Pa, ref.x, ref.P)) < 1e-4  # (a run of the script, not a state nobody touched)
    assert bits_equal(xb, xa) and bits_equal(Pb, Pa), "max_new 9 against max_new 2"
    assert bits_equal(xc, xa) and bits_equal(Pc, Pa), "the clamped max_new against max_new 2"


# ---- 4. a chunk that does not factorise, inside a period ----------------------------------------------------------------------------------
def indefinite_state():
    """80 landmarks; the own 2 x 2 block of features 64 .. 69 is -4 I: an observation of one of them has a range variance of about -4,
    the first pivot of its chunk.  Features 0 .. 69 are the period's, 70 .. 79 passive"""
    x0, P0 = LM.synthetic_state(80, 560)
    for f in range(64, 70):
        P0[3 + 2 * f:5 + 2 * f, 3 + 2 * f:5 + 2 * f] = -4.0 * np.eye(2, dtype=f32)
    assert symmetric(P0)
    return x0, P0


def test_a_period_whose_only_chunk_fails_changes_no_bit():
    import slam_amd
    x0, P0 = indefinite_state()
    d = make_dev(80, association_known=True)
    d.upload(x0, P0)
    assert d.status() == 0
    bad = np.arange(64, 70)
    d.local_begin(np.arange(70), 0)
    d.update(LM.observations(x0, bad, np.random.default_rng(6)), bad, LM.R)
    d.local_end()
    x, P = d.state()
    assert d.status() == slam_amd.EKF_STATUS_NOT_PD and d.local_info()["commits"] == 1 and d.dim == x0.shape[0]
    d.close()
    assert np.isfinite(x).all() and np.isfinite(P).all()
    assert bits_equal(x, x0) and bits_equal(P, P0)


def test_a_failing_chunk_behind_a_good_one():
    """begin; predict; an update of features 0 .. 63 (a chunk that is applied) and 64 .. 69 (a chunk whose first pivot is about -4);
    predict; an update of features 0 .. 9; end.  The failing chunk leaves W1 as the good one wrote it: a psi that added W1 regardless
    of flag[0] would count the first chunk twice, and the commit would take Y^T G1 G1^T Y from P[B, B] a second time.  The reference
    is the float64 model given the script WITHOUT the six observations; the rule on the whole state and on P[B, B]"""
    import slam_amd
    x0, P0 = indefinite_state()
    rng = np.random.default_rng(7)
    ref = ekf_model.EkfModel(chunk=LM.CHUNK, association_known=True, **LM.CONF)
    ref.upload(x0, P0)
    ids = np.arange(70, dtype=np.int32)
    ctl = [(3.0, float(f32(g)), LM.Q, LM.DT) for g in (0.05, -0.05)]
    ref.predict(*ctl[0])
    z1 = LM.observations(ref.x, ids, rng)
    passive = np.arange(3 + 2 * 70, x0.shape[0])
    before = ref.P[np.ix_(passive, passive)].copy()
    ref.update(z1[:64], ids[:64], LM.R)
    taken = before - ref.P[np.ix_(passive, passive)]  # Y^T G1 G1^T Y: what the good chunk takes from P[B, B], and a stale W1 would take again
    ref.predict(*ctl[1])
    z2 = LM.observations(ref.x, ids[:10], rng)
    ref.update(z2, ids[:10], LM.R)
    script = [("begin", (ids, 0)), ("predict", ctl[0]), ("update", (z1, ids, LM.R)), ("predict", ctl[1]), ("update", (z2, ids[:10], LM.R)), ("end", ())]
    loc, full = (make_dev(80, association_known=True) for _ in range(2))
    for d in (loc, full):
        d.upload(x0, P0)
    LM.drive(loc, script)
    LM.drive(full, script, periods=False)
    (xl, Pl), (xf, Pf) = loc.state(), full.state()
    assert loc.status() == slam_amd.EKF_STATUS_NOT_PD and full.status() == slam_amd.EKF_STATUS_NOT_PD
    assert loc.dim == full.dim == ref.dim and loc.local_info() == dict(open=0, k=0, new=0, max_new=0, calls=0, commits=1)
    loc.close()
    full.close()
    assert symmetric(Pl) and symmetric(Pf) and np.isfinite(Pl).all() and np.isfinite(xl).all()
    lx, lP = errors(xl, Pl, ref.x, ref.P)
    fx, fP = errors(xf, Pf, ref.x, ref.P)
    print("EKF local failing chunk behind a good one: dim %d, local x %.3e P %.3e, full device x %.3e P %.3e, ratio x %.3f P %.3f" %
          (ref.dim, lx, lP, fx, fP, ratio(lx, fx), ratio(lP, fP)))
    A, B = LM.blocks_of(script, x0.shape[0], ref.dim)
    assert np.array_equal(B, passive)
    # the construction has teeth: the term counted twice would be 100 x the bound P[B, B] is held to, or more
    gap = float(np.abs(taken).max() / np.abs(ref.P[np.ix_(B, B)]).max())
    bound = max(FACTOR * LM.block_errors(xf, Pf, ref.x, ref.P, A, B)["P[B,B]"], FLOOR)
    print("EKF local failing chunk behind a good one: the good chunk takes %.3e of max |P[B,B]|, the bound is %.3e" % (gap, bound))
    assert gap >= 100.0 * bound, (gap, bound)
    try:
        assert within(lx, fx) and within(lP, fP), (lx, fx, lP, fP)
    finally:
        held_per_block("failing chunk behind a good one", (xl, Pl), (xf, Pf), ref, A, B, only=("P[B,B]",))
