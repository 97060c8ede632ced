"""The device EKF (slam_amd/csrc/ekf.cpp) and its ensemble (ekf_ens.cpp) past ONE pass of their lanes: every loop of the form
`for (r = tid; r < dim; r += 256)` and every per-lane loop of the gates (`j += 256` in ekf_gate_kernel, `j += 64` in the ensemble's
waves) makes a second pass here, up to the ensemble's capacity (512 landmarks, dim 1027, ld 1056).
  1. the single filter's gates on 255 / 256 / 257 / 600 features against the float64 model's labels (tests/ekf_model.py), with the
     model's own margin deciding which decisions are clear (> 1e-3, the rule of test_gpu_ekf.py);
  2. exact ties between two bit-identical features: the lower one wins, in the single filter and through the ensemble;
  3. the seam of the bearing innovation: readings wrapped into (-pi, pi] of landmarks whose predicted bearing lies beyond -pi or pi;
  4. the ensemble's stages past 256 columns, up to the capacity: tests/test_gpu_ekf_ens.py's tile test at three larger shapes, a gated
     launch of three sizes, a member that runs out of room at 510 landmarks;
  5. the single filter's gated step at ten tiles of the rank update and two chunks;
  6. K steps per launch on members of 127 and 300 landmarks.
The packet of observations (`study`) and its caps are checked on the CPU as well (tests/test_ekf_cpu.py).  The error rule is
tests/test_gpu_ekf.py's, unchanged: x relative to max |x| and P relative to max |P| of the float64 model, at most max(4 x yardstick,
8 * 2^-24); the yardstick is the host filter's step up to dim 523, the float32 model with the device's chunks beyond (the host's
heading update is two naive dense D^3 products).  The measured ratios are in profiles/ekf_scale.txt.
NOT reached here: the single filter's heading kernel caps gridDim.y at 16 384, so its row loop repeats only for dim > 16 384, a 1 GB
covariance."""
import numpy as np
import pytest

from conftest import bits_equal

import ekf_model
import ekf_ens_run_model as M
from test_gpu_ekf import FACTOR, FLOOR, SENTINEL, errors, make_dev, make_model, symmetric, within
from test_gpu_ekf_ens import Q0, cfg_of, known_host, observations, ratio, synthetic_state, tile, tiles_and_chunks

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RE = np.array([[0.1 ** 2, 0], [0, (np.pi / 180) ** 2]], f32)
GATES = dict(gate_reject=4.0, gate_augment=25.0)
CLEAR = 1e-3  # a decision whose float64 margin exceeds this is held against the device
NEW, DISCARD = ekf_model.ASSOC_NEW, ekf_model.ASSOC_DISCARD
DT = 0.025


# ---- 0. the shared packet and its float64 study (no GPU: tests/test_ekf_cpu.py runs it too) ---------------------------------------------
_study = {}


def study(nf, extra=0):
    """The state synthetic_state(nf, 7 nf) and 64 readings of it: 48 of features drawn without repeats, 8 far beyond the ring (new
    landmarks), 8 of the first eight features displaced by (1.2 m, 0.03 rad); `extra` more readings of further distinct features behind
    them.  With them the float64 model's labels, its margins and which features the readings were generated from.  Computed once"""
    if (nf, extra) not in _study:
        x0, P0 = synthetic_state(nf, 7 * nf)
        rng = np.random.default_rng(nf)
        perm = rng.permutation(nf)
        idf = perm[:48]
        far = np.stack([90.0 + 3.0 * np.arange(8), np.linspace(-3, 3, 8)], axis=1).astype(f32)
        parts = [observations(x0, idf, rng), far, observations(x0, idf[:8], rng) + np.array([1.2, 0.03], f32)]
        if extra:
            parts.append(observations(x0, perm[48:48 + extra], rng))
        z = np.concatenate(parts).astype(f32)
        mdl = ekf_model.EkfModel(**GATES)
        mdl.upload(x0, P0)
        lab, margin = mdl.associate(z, RE, want_margin=True)
        _study[(nf, extra)] = dict(nf=nf, x0=x0, P0=P0, idf=idf, z=z, lab=lab, margin=margin, clear=margin > CLEAR)
    return _study[(nf, extra)]


def caps(s):
    """the conditions of the packet's first 64 decisions: at most 2 unclear, at least 40 matches, at least 6 new; at 600 features at least
    5 of the first 48 winners are a feature other than the one the reading came from (the dense ring makes nd comparisons decide)"""
    lab, clear = s["lab"][:64], s["clear"][:64]
    assert int((~clear).sum()) <= 2 and int((lab >= 0).sum()) >= 40 and int((lab == NEW).sum()) >= 6, (s["nf"], lab, s["margin"][:64])
    foreign = int(((lab[:48] >= 0) & (lab[:48] != s["idf"])).sum())
    if s["nf"] == 600:
        assert foreign >= 5, foreign
    return foreign


def forced_ids(lab):
    """the ids that make a model with a known association (feature f has id f after an upload) apply `lab`: (keep, ids)"""
    lab = np.asarray(lab)
    return lab != DISCARD, np.where(lab >= 0, lab, (1 << 20) + np.arange(lab.shape[0])).astype(np.int64)


def forced_step(dtype, x0, P0, z, lab):
    """zero motion, no heading: the update and the augment of `lab` on (x0, P0), in `dtype`, with the device's chunks"""
    mdl = ekf_model.EkfModel(dtype=dtype, chunk=64, association_known=True, **GATES)
    mdl.upload(x0, P0)
    keep, ids = forced_ids(lab)
    mdl.sim(0.0, 0.0, Q0, DT, 0.0, z[keep], ids[keep], RE, RE, 1)
    return mdl


def held(tag, xd, Pd, m64, xr, Pr):
    """the error rule, with the figures printed first"""
    rx, rP = errors(xr, Pr, m64.x, m64.P)
    dx, dP = errors(xd, Pd, m64.x, m64.P)
    print("SCALE %s: device x %.3e P %.3e, yardstick x %.3e P %.3e, ratio x %.3f P %.3f" % (tag, dx, dP, rx, rP, ratio(dx, rx), ratio(dP, rP)))
    assert within(dx, rx) and within(dP, rP), (tag, dx, rx, dP, rP)


# ---- 1. single filter: gates past one pass of lanes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [255, 256, 257, 600])
def test_gates_past_one_pass_of_lanes(nf):
    """ekf_gate_kernel's lanes stride by 256: at 257 features lane 0 holds two, at 600 every lane two or three, and a candidate has to
    survive from one feature of a lane to the next"""
    import slam_amd
    s = study(nf)
    foreign = caps(s)
    dev = slam_amd.EkfGpu(nf, **GATES)
    dev.upload(s["x0"], s["P0"])
    got = dev.associate(s["z"], RE)
    dev.close()
    clear, lab = s["clear"], s["lab"]
    second = int((lab[clear] >= 256).sum())
    print("SCALE gates nf %d: checked %d skipped %d, match / new / discard %d / %d / %d, foreign winners %d, winners past index 256: %d, smallest margin %.2e"
          % (nf, clear.sum(), (~clear).sum(), (lab >= 0).sum(), (lab == NEW).sum(), (lab == DISCARD).sum(), foreign, second, s["margin"].min()))
    assert np.array_equal(got[clear], lab[clear]), (nf, got, lab, s["margin"])
    if nf == 600:
        assert second >= 10, second


# ---- 2. exact ties -----------------------------------------------------------------------------------------------------------------------
def tie_state(x0, P0, src, dst):
    """Feature dst made a bit-identical twin of feature src, and one noise-free reading of it.  src is first moved 8 m outwards along
    its ray: on the dense ring a neighbour's nd can undercut the pair's even for a noise-free reading (the float64 model labels 199 for
    feature 200 of the 600), and then no tie decides anything.  dst takes src's coordinates, its 2 x 2 block and ALL its rows and
    columns, the pose's among them -- P = J S J^T + blockdiag(own) with row J_src twice, positive definite by construction (with dst's
    old blocks against the other features left in place it is not: the float64 Cholesky fails); the block between the two is what both
    inherit from the pose, J_src S J_src^T = P[src, 0:3] Pvv^-1 P[0:3, src], with neither own block in it.  The gate reads
    x, Pvv, P[0:3, f] and the own block only: the two pairs evaluate the same operations on the same bits.  Asserted on the float64
    model: before the twin exists src wins with a margin > 1e-3 against every other feature; with it, the lower of the two"""
    x, P = x0.copy(), P0.astype(f64)
    fs, fd = 3 + 2 * src, 3 + 2 * dst
    ray = (x[fs:fs + 2] - x[:2]).astype(f64)
    x[fs:fs + 2] = (x[fs:fs + 2] + 8.0 * ray / np.hypot(*ray)).astype(f32)
    dx, dy = f64(x[fs]) - f64(x[0]), f64(x[fs + 1]) - f64(x[1])
    z = np.array([[np.hypot(dx, dy), (np.arctan2(dy, dx) - f64(x[2]) + np.pi) % (2 * np.pi) - np.pi]], f32)
    mdl = ekf_model.EkfModel(**GATES)
    mdl.upload(x, P0)
    lab, margin = mdl.associate(z, RE, want_margin=True)
    assert lab[0] == src and margin[0] > CLEAR, (src, dst, lab, margin)
    x[fd:fd + 2] = x[fs:fs + 2]
    P[fd:fd + 2, :] = P[fs:fs + 2, :]
    P[:, fd:fd + 2] = P[:, fs:fs + 2]
    cross = P[fs:fs + 2, :3] @ np.linalg.solve(P[:3, :3], P[:3, fs:fs + 2])
    P[fs:fs + 2, fd:fd + 2] = P[fd:fd + 2, fs:fs + 2] = 0.5 * (cross + cross.T)
    P = P.astype(f32)
    P = np.tril(P) + np.tril(P, -1).T
    np.linalg.cholesky(P.astype(f64))  # (raises where P is not positive definite)
    assert bits_equal(x[fd:fd + 2], x[fs:fs + 2]) and bits_equal(P[:3, fd:fd + 2], P[:3, fs:fs + 2])
    assert bits_equal(P[fd:fd + 2, fd:fd + 2], P[fs:fs + 2, fs:fs + 2])
    mdl.upload(x, P)
    assert mdl.associate(z, RE)[0] == min(src, dst), (src, dst)
    return x, P, z


@pytest.mark.parametrize("a,b", [(10, 11), (10, 266), (200, 500), (0, 599)])
def test_a_tie_goes_to_the_lower_feature(a, b):
    """600 features; the twins in neighbouring lanes, in one lane's first and second pass, in different lanes and passes, at both
    ends.  Each pair with either of the two as the original: a kernel that never looked at the twin, or that kept the later or the
    higher of two equal candidates, names the wrong one in one of the two"""
    import slam_amd
    s = study(600)
    dev = slam_amd.EkfGpu(600, **GATES)
    for src, dst in ((a, b), (b, a)):
        x, P, z = tie_state(s["x0"], s["P0"], src, dst)
        dev.upload(x, P)
        assert dev.associate(z, RE)[0] == min(a, b), (src, dst)
    dev.close()


ENS_TIES = [(10, 11), (10, 74), (10, 202), (63, 64), (0, 299)]


def test_a_tie_goes_to_the_lower_feature_in_the_ensemble():
    """300 features, one member per pair and role in ONE launch (zero motion, no heading: the gates see the uploaded state).  The
    ensemble has no label readout; the label shows through the state: the matched twin's own block shrinks by its own gain, the other's
    only by the cross block's.  (The reading is noise-free, the innovation a rounding error: x hardly moves under either label, so it
    is P that tells them apart.)  Per member: the float64 model forced to the lower label and forced to the higher one must differ in
    P by at least 100 x the tolerance the device is then held to -- the error rule, the float32 model the yardstick (dim 603) --
    or the construction is void and the test fails; then the device meets the rule against the lower label's model"""
    import slam_amd
    x0, P0 = synthetic_state(300, 2100)
    cases = [(src, dst) for a, b in ENS_TIES for src, dst in ((a, b), (b, a))]
    B = len(cases)
    ens = slam_amd.EkfEnsemble(B, 300, **GATES)
    made = [tie_state(x0, P0, src, dst) for src, dst in cases]
    for k, (x, P, z) in enumerate(made):
        ens.upload(k, x, P)
    ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, DT, np.stack([z for _, _, z in made]), None, RE, RE, 1)
    assert not ens.status().any() and (ens.dims() == 603).all()
    for k, (src, dst) in enumerate(cases):
        x, P, z = made[k]
        lo, hi = min(src, dst), max(src, dst)
        m_lo, m_hi, y_lo = forced_step(f64, x, P, z, [lo]), forced_step(f64, x, P, z, [hi]), forced_step(f32, x, P, z, [lo])
        rx, rP = errors(y_lo.x, y_lo.P, m_lo.x, m_lo.P)
        tol = max(FACTOR * rP, FLOOR)
        gap = errors(m_hi.x, m_hi.P, m_lo.x, m_lo.P)[1]
        assert gap >= 100.0 * tol, (src, dst, gap, tol)
        xd, Pd = ens.state(k)
        assert symmetric(Pd), (src, dst)
        held("tie nf 300 twin %d of %d (labels apart by %.1e of max |P|)" % (dst, src, gap), xd, Pd, m_lo, y_lo.x, y_lo.P)
    ens.close()


# ---- 3. the bearing seam ----------------------------------------------------------------------------------------------------------------
def seam(nf, heading):
    """The state of `study` with the pose heading set, and eight readings, wrapped into (-pi, pi] as the simulator delivers them, of
    the eight landmarks next to the ring's +-pi direction: the four of lowest and the four of highest atan2(dy, dx).  heading = +0.1:
    the first four are predicted below -pi and read near +pi, z1 - zp[1] is near +2 pi before ekf_trig_offset; heading = -0.1: the last
    four are predicted above pi and read near -pi, the difference is near -2 pi.  (ONE heading cannot put four landmarks below -pi and
    four above pi - 0.05: the two windows together are 0.05 rad wide and the ring of 600 has a landmark every 0.0105 rad.)"""
    x, P = synthetic_state(nf, 7 * nf)
    x = x.copy()
    x[2] = heading
    f = 3 + 2 * np.arange(nf)
    at = np.arctan2(x[f + 1].astype(f64) - f64(x[1]), x[f].astype(f64) - f64(x[0]))
    zp1 = at - f64(x[2])
    assert int((zp1 < -np.pi).sum() if heading > 0 else (zp1 > np.pi - 0.05).sum()) >= 4
    order = np.argsort(at)
    feats = np.concatenate([order[:4], order[-4:]]).astype(np.int32)
    z = observations(x, feats, np.random.default_rng(nf + 2))
    z[:, 1] = ((z[:, 1].astype(f64) + np.pi) % (2 * np.pi) - np.pi).astype(f32)
    raw = z[:, 1] - zp1[feats]
    assert int((raw > 6.0).sum() if heading > 0 else (raw < -6.0).sum()) >= 4, raw  # the seam is crossed before the wrap
    return x, P, feats, z


@pytest.mark.parametrize("heading", [0.1, -0.1])
def test_bearing_seam_single(heading):
    """known association: an unwrapped innovation of 2 pi would move the state by metres, against a bound of parts in 10^7; gated: every
    clear decision is the generating feature or the model's label"""
    import slam_amd
    nf = 600
    x, P, feats, z = seam(nf, heading)
    dev = slam_amd.EkfGpu(nf, **GATES)
    dev.upload(x, P)
    dev.update(z, feats, RE)
    xd, Pd = dev.state()
    m64, m32 = (forced_step(t, x, P, z, feats) for t in (f64, f32))
    assert dev.status() == 0 and symmetric(Pd)
    held("seam single nf %d heading %+.1f" % (nf, heading), xd, Pd, m64, m32.x, m32.P)
    dev.upload(x, P)
    got = dev.associate(z, RE)
    dev.close()
    mdl = ekf_model.EkfModel(**GATES)
    mdl.upload(x, P)
    lab, margin = mdl.associate(z, RE, want_margin=True)
    clear = margin > CLEAR
    print("SCALE seam gates nf %d heading %+.1f: checked %d skipped %d, matched %d" % (nf, heading, clear.sum(), (~clear).sum(), (lab >= 0).sum()))
    assert clear.sum() >= 6 and (lab[clear] >= 0).all(), (lab, margin)  # a reading missed by 2 pi gates with nothing
    assert ((got == feats) | (got == lab))[clear].all(), (got, feats, lab, margin)


def test_bearing_seam_ensemble():
    """300 features, the two headings as two members of one launch, known association (the ids are shared: the same eight features,
    each member's own readings of them)"""
    import slam_amd
    nf = 300
    cases = [seam(nf, h) for h in (0.1, -0.1)]
    assert np.array_equal(cases[0][2], cases[1][2])
    ens = slam_amd.EkfEnsemble(2, nf, association_known=True, **GATES)
    for b, (x, P, feats, z) in enumerate(cases):
        ens.upload(b, x, P)
    ens.sim(np.zeros((2, 2), f32), np.zeros(2, f32), Q0, DT, np.stack([c[3] for c in cases]), cases[0][2], RE, RE, 1)
    assert not ens.status().any() and (ens.dims() == 3 + 2 * nf).all()
    for b, (x, P, feats, z) in enumerate(cases):
        xd, Pd = ens.state(b)
        m64, m32 = (forced_step(t, x, P, z, feats) for t in (f64, f32))
        assert symmetric(Pd), b
        held("seam ensemble nf %d heading %+.1f" % (nf, x[2]), xd, Pd, m64, m32.x, m32.P)
    ens.close()


# ---- 4. ensemble: steps past 256 columns, up to the capacity ---------------------------------------------------------------------------
# dims 255 / 257 / 259, one member crossing 256 in its augment, two chunks; dims on both sides of 512, two and three passes of the
# 256-lane loops; the largest member ends at 512 landmarks, dim 1027 = the handle's capacity, ld 1056: the heading's 2 ld floats of LDS at
# its largest beside the update's 64 KB
SCALE_CASES = [((126, 127, 128), 65, 1), ((254, 255, 383), 100, 2), ((0, 256, 507), 64, 5)]


@pytest.mark.parametrize("nfs,m,nnew", SCALE_CASES)
def test_tiles_and_chunks_at_scale(nfs, m, nnew):
    tiles_and_chunks(nfs, m, nnew)


def test_gated_members_of_three_sizes():
    """65, 257 and 500 features in one launch with room for 512, each member given the packet made from its own state (zero motion, no
    heading: the gates see the uploaded state): the wave's `j += 64` loop runs up to eight times.  A member is compared -- dimension,
    and the error rule with the float32 model given the float64 labels as the yardstick -- unless one of its decisions is unclear"""
    import slam_amd
    nfs = (65, 257, 500)
    packs = [study(nf) for nf in nfs]
    ens = slam_amd.EkfEnsemble(3, 512, **GATES)
    for b, s in enumerate(packs):
        caps(s)
        ens.upload(b, s["x0"], s["P0"])
    ens.sim(np.zeros((3, 2), f32), np.zeros(3, f32), Q0, DT, np.stack([s["z"] for s in packs]), None, RE, RE, 1)
    dims = ens.dims()
    assert not ens.status().any()
    skipped = 0
    for b, s in enumerate(packs):
        if not s["clear"].all():
            skipped += 1
            continue
        m64 = ekf_model.EkfModel(chunk=64, **GATES)  # the float64 model with its own gates
        m64.upload(s["x0"], s["P0"])
        lab = m64.sim(0.0, 0.0, Q0, DT, 0.0, s["z"], None, RE, RE, 1)
        assert np.array_equal(lab, s["lab"])
        m32 = forced_step(f32, s["x0"], s["P0"], s["z"], lab)
        xd, Pd = ens.state(b)
        assert dims[b] == m64.dim == xd.shape[0] == 3 + 2 * (s["nf"] + int((lab == NEW).sum())), (b, dims)
        assert symmetric(Pd), b
        held("gated member nf %d (%d matched, %d new)" % (s["nf"], (lab >= 0).sum(), (lab == NEW).sum()), xd, Pd, m64, m32.x, m32.P)
    ens.close()
    print("SCALE gated members: compared %d skipped %d" % (3 - skipped, skipped))
    assert skipped <= 1


def test_capacity_at_scale():
    """test_gpu_ekf_ens.py's test_edges at 510 landmarks: the gates open three landmarks in both members; the one of 510 has room for two
    (SLAMGPU_EKF_STATUS_CAPACITY, neither its update nor its augment applied: bit for bit a one-member ensemble's predict and heading of
    the same inputs with nothing observed), the one of 100 applies the step and is held to the rule, the host filter the yardstick"""
    import slam_amd
    sim, hekf, nz = known_host()
    c = sim.conf
    cfg = cfg_of(c, association_known=False)
    (xb, Pb), (xs, Ps) = synthetic_state(510, 3570), synthetic_state(100, 700)
    rng = np.random.default_rng(510)
    znew = np.array([[90.0, 2.5], [95.0, -2.0], [100.0, 0.5]], f32)
    zb, zs = np.concatenate([observations(xb, [0, 1], rng), znew]), np.concatenate([observations(xs, [0, 1], rng), znew])
    V, G, phi = 3.0, -0.02, 0.1
    VG, ph = tile([V, G], 2), np.full(2, phi, f32)
    ref = slam_amd.EkfEnsemble(1, 512, **cfg)
    ref.upload(0, xb, Pb)
    ref.sim(VG[:1], ph[:1], nz["Qe"], nz["dt"], None, None, nz["Re"], nz["R"], 1)
    ens = slam_amd.EkfEnsemble(2, 512, **cfg)
    ens.upload(0, xb, Pb)
    ens.upload(1, xs, Ps)
    ens.sim(VG, ph, nz["Qe"], nz["dt"], np.stack([zb, zs]), None, nz["Re"], nz["R"], 1)
    assert list(ens.status()) == [slam_amd.EKF_STATUS_CAPACITY, 0] and list(ens.dims()) == [1023, 209]
    (xa, Pa), (xr, Pr) = ens.state(0), ref.state(0)
    assert bits_equal(xa, xr) and bits_equal(Pa, Pr) and not bits_equal(Pa, Pb) and symmetric(Pa)
    # the small member: the float64 model's own gates, clear by its own margin
    probe = make_model(c, association_known=False)
    probe.upload(xs, Ps)
    probe.predict(V, G, nz["Qe"], nz["dt"])
    probe.observe_heading(phi)
    lab, margin = probe.associate(zs, nz["Re"], want_margin=True)
    assert list(lab) == [0, 1, NEW, NEW, NEW] and (margin > CLEAR).all(), (lab, margin)
    mdl = make_model(c, association_known=False, chunk=64)
    mdl.upload(xs, Ps)
    mdl.sim(V, G, nz["Qe"], nz["dt"], phi, zs, None, nz["Re"], nz["R"], 1)
    hekf.upload(xs, Ps)  # (its association is the known one: the ids that give the same labels)
    hekf.sim_step(V, G, nz["Qe"], nz["dt"], phi, zs, [0, 1, 100, 101, 102], nz["Re"], nz["R"], 1)
    xh, Ph = hekf.state(cap=209)
    xd, Pd = ens.state(1)
    assert xd.shape[0] == mdl.dim == xh.shape[0] == 209 and symmetric(Pd)
    held("capacity at scale, the member of 100 beside the refused one of 510", xd, Pd, mdl, xh, Ph)
    ens.close()
    ref.close()


# ---- 5. single filter: a gated step at ten tiles ------------------------------------------------------------------------------------------
def test_gated_step_at_ten_tiles():
    """600 features, dim 1203: 10 x 10 tiles of ekf_syrk_kernel, five workgroups of the predict, heading and innovation kernels, 38 of the
    gain.  The packet and 40 readings of further features: about 96 matches, two chunks, and 8 new landmarks.  The gates decide on the
    state AFTER predict and heading, so the margins are the float64 model's at that state"""
    sim, _, nz = known_host()
    c = sim.conf
    assert (c.GATE_REJECT, c.GATE_AUGMENT) == (4.0, 25.0)
    nf = 600
    s = study(nf, extra=40)
    caps(s)
    x0, P0, z = s["x0"], s["P0"], s["z"]
    ctl, phi = (3.0, 0.05, nz["Qe"], nz["dt"]), float(x0[2]) + 0.004
    mdl = make_model(c, association_known=False, chunk=64)
    m32 = make_model(c, association_known=False, chunk=64, dtype=f32)
    for m in (mdl, m32):
        m.upload(x0, P0)
        m.predict(*ctl)
        m.observe_heading(phi)
    lab, margin = mdl.associate(z, nz["Re"], want_margin=True)
    unclear = int((margin <= CLEAR).sum())
    print("SCALE ten tiles nf %d: %d decisions, %d unclear, match / new / discard %d / %d / %d, smallest margin %.2e" %
          (nf, lab.shape[0], unclear, (lab >= 0).sum(), (lab == NEW).sum(), (lab == DISCARD).sum(), margin.min()))
    if unclear:
        pytest.skip("%d of %d decisions of the float64 model are within %g of a gate or of a rival" % (unclear, lab.shape[0], CLEAR))
    nm, nn = int((lab >= 0).sum()), int((lab == NEW).sum())
    assert nm > 64 and nn >= 6
    for m in (mdl, m32):  # the float32 yardstick is given the float64 labels
        m.update(z[lab >= 0], lab[lab >= 0], nz["R"])
        m.augment(z[lab == NEW], nz["Re"])
    D = 3 + 2 * (nf + nn)
    cap_lm = nf + nn + 2
    cap = 3 + 2 * cap_lm
    devs = [make_dev(c, cap_lm, association_known=False) for _ in range(2)]
    for d in devs:  # what lies beyond dim must stay as it was uploaded
        d.upload(np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))
        d.upload(x0, P0)
    a, b = devs
    a.sim(*ctl, phi, z, None, nz["Re"], nz["R"], 1)
    xa, Pa = a.state()
    b.predict(*ctl)
    assert symmetric(b.state()[1])
    b.observe_heading(phi)
    assert symmetric(b.state()[1])
    got = b.associate(z, nz["Re"])
    assert np.array_equal(got, lab), (got, lab, margin)
    b.update(z[got >= 0], got[got >= 0], nz["R"])
    assert symmetric(b.state()[1])
    b.augment(z[got == NEW], nz["Re"])
    xb, Pb = b.state()
    assert symmetric(Pb) and xb.shape[0] == D == mdl.dim
    assert bits_equal(xa, xb) and bits_equal(Pa, Pb)  # sim == the stages in order
    assert a.status() == 0 and b.status() == 0
    full = a.block(np.arange(cap, dtype=np.int32))
    assert bits_equal(full[:D, :D], Pa) and (full[D:, :] == SENTINEL).all() and (full[:, D:] == SENTINEL).all()
    for d in devs:
        d.close()
    held("ten tiles nf %d, %d matched in two chunks, %d new" % (nf, nm, nn), xa, Pa, mdl, m32.x, m32.P)


# ---- 6. K steps per launch at these sizes -------------------------------------------------------------------------------------------------
def test_run_of_three_steps_at_scale():
    """tests/test_gpu_ekf_ens_run.py's method at its smallest scale: members of 127 and 300 features, a tape of an observation of 70
    shared ids (two chunks for the larger member), a control step, an observation with one id new to everybody; noise off.  run_noise
    leaves bit for bit what three sim_noise calls leave on a twin"""
    import slam_amd
    sim, _, nz = known_host()
    xb, Pb = synthetic_state(300, 2100)
    # (noise off, every member is fed the same readings: the smaller member holds the larger one's first 127 features, so that the
    # readings of the ids it shares are readings of its own map -- a principal block of a positive definite P is one)
    states = [(xb[:257].copy(), np.ascontiguousarray(Pb[:257, :257])), (xb, Pb)]
    rng = np.random.default_rng(300)
    handles = []
    for _ in range(2):
        e = slam_amd.EkfEnsemble(2, 301, **cfg_of(sim.conf), seed=1234)
        for b in (0, 1):  # the largest last: the shared table then knows every feature
            e.upload(b, *states[b])
        handles.append(e)
    one, twin = handles
    big = states[1][0]
    ids0, ids2 = rng.permutation(300)[:70].astype(np.int32), np.concatenate([rng.permutation(300)[:9], [300]]).astype(np.int32)
    z2 = np.concatenate([observations(big, ids2[:9], rng), np.array([[31.0, 0.7]], f32)])
    tape = [M.step_dict(0, 2.0, 0.02, 0.1, nz["dt"], truth=big[:3], observe=1, z_true=observations(big, ids0, rng), ids=ids0),
            M.step_dict(1, 2.0, 0.02, 0.1, nz["dt"], truth=big[:3]),
            M.step_dict(2, 2.0, 0.01, 0.1, nz["dt"], truth=big[:3], observe=1, z_true=z2, ids=ids2)]
    M.drive_run(one, tape, nz, noise=0)
    M.drive_single(twin, tape, nz, noise=0)
    a, t = M.snapshot(one), M.snapshot(twin)
    assert not M.identical(a, t), M.identical(a, t)
    assert not t["status"].any() and list(t["dims"]) == [3 + 2 * 128, 3 + 2 * 301]
    for b in (0, 1):
        P = one.state(b)[1]
        assert symmetric(P) and not bits_equal(P[:states[b][1].shape[0], :states[b][1].shape[0]], states[b][1]), b
    one.close()
    twin.close()
