"""The device EKF ensemble (include/slamgpu.h: slamgpu_ens_*; slam_amd/csrc/ekf_ens.cpp) on the GPU.
  1. teacher-forced steps of the two host runs tests/test_gpu_ekf.py drives, eight states of different dimension in ONE launch;
  2. tile and chunk edges on synthetic states, three members of three sizes per launch: the error rule, P == P^T bit for bit, the
     padding and the neighbours' slabs;
  3. the reference's association decisions (tests/golden/kat_assoc.npz) through the ensemble's gates;
  4. invariance: a member does not depend on the ensemble's size, on its place in it, or on the run;
  5. the noise rule of sim_noise against its model;  6. the consistency accumulators;  7. a whole run;  8. edges.
The error rule is the single filter's, unchanged (tests/test_gpu_ekf.py): x relative to max |x| and P relative to max |P| of the
float64 model, at most max(4 x yardstick, 8 * 2^-24); the yardstick is the host filter's error from the same state, or the float32
model's where the device's chunks are a deviation of its own (m > 64).  The factor 4 was fixed before the single filter's first run.
The measured ratios are printed and kept in profiles/ekf_ensemble.txt."""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN, bits_equal, load_golden

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FLOOR = 8.0 * 2.0 ** -24
FACTOR = 4.0
SENTINEL = f32(777.25)
Q0 = np.zeros((2, 2), f32)


def cfg_of(c, **over):
    kw = dict(use_heading=c.SWITCH_HEADING_KNOWN == 1, batch_update=c.SWITCH_BATCH_UPDATE == 1, association_known=c.SWITCH_ASSOCIATION_KNOWN != 0,
              wheel_base=c.WHEELBASE, sigma_phi=c.sigmaT, gate_reject=c.GATE_REJECT, gate_augment=c.GATE_AUGMENT)
    kw.update(over)
    return kw


def errors(x, P, xm, Pm):
    return float(np.abs(x - xm).max() / np.abs(xm).max()), float(np.abs(P - Pm).max() / np.abs(Pm).max())


def within(dev, ref):
    return dev <= max(FACTOR * ref, FLOOR)


def ratio(dev, ref):
    return dev / max(ref, FLOOR / FACTOR)


def symmetric(P):
    return bits_equal(P, P.T.copy())


def mirrored(P):
    return np.tril(P) + np.tril(P, -1).T


def tile(a, B):
    return np.repeat(np.asarray(a, f32)[None], B, axis=0)


# ---- 1. teacher-forced, ragged -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["loop1", "webmap"])
def test_teacher_forced_ragged(key):
    """Eight forced steps of a host run, of eight different dimensions (the first observation, 3 -> 3 + 2 n, and steps where the
    dimension grows among them): member k holds step k's state (its lower triangle mirrored, as test_gpu_ekf.py explains).  nz is
    shared, so launch k feeds EVERY member step k's inputs: eight members of eight dimensions per launch; member k of launch k is
    the teacher-forced step and is held to the rule and to the host's dimension, the others to P == P^T."""
    import slam_amd
    import ekf_model
    import test_gpu_ekf as T
    from slam_amd import host
    run = T.host_run(key)
    c, nz = run["conf"], run["noise"]
    grows = [f for f in run["forced"] if f["x1"].shape[0] != f["x0"].shape[0]]
    picked, dims = [], set()
    for f in [run["forced"][0]] + grows + run["forced"]:
        if f["x0"].shape[0] not in dims and len(picked) < 8:
            picked.append(f)
            dims.add(f["x0"].shape[0])
    assert len(picked) == 8 and picked[0]["x0"].shape[0] == 3 and picked[0]["x1"].shape[0] > 3 and sum(f["x1"].shape[0] != f["x0"].shape[0] for f in picked) >= 2
    B = 8
    ens = slam_amd.EkfEnsemble(B, run["nlm"] + 40, **cfg_of(c))  # (room for whatever the gates make of a foreign step's observations)
    hsim = host.HostSim(["-m", os.path.join(DATA, T.RUNS[key][0] + ".mat"), "-method", "EKF1"])
    hekf = host.HostEkf(hsim)
    worst = dict(x=0.0, P=0.0)
    for k, f in enumerate(picked):
        s = run["steps"][f["k"]]
        for j, g in enumerate(picked):
            ens.upload(j, g["x0"], mirrored(g["P0"]))
        n, before = s["z"].shape[0], ens.status()
        ens.sim(tile([s["V"], s["G"]], B), np.full(B, s["phi"], f32), nz["Qe"], nz["dt"], tile(s["z"], B), s["vis"], nz["Re"], nz["R"], 1)
        dims_after = ens.dims()
        assert not (ens.status()[k] & ~before[k]), k
        for j in range(B):
            assert symmetric(ens.state(j)[1]), (k, j)
        args = (s["V"], s["G"], nz["Qe"], nz["dt"], s["phi"], s["z"], s["vis"], nz["Re"], nz["R"], 1)
        x0, P0 = f["x0"], mirrored(f["P0"])
        mdl = ekf_model.EkfModel(**cfg_of(c))
        mdl.upload(x0, P0)
        mdl.sim(*args)
        hekf.upload(x0, P0)
        hekf.sim_step(*args)
        xh, Ph = hekf.state()
        xd, Pd = ens.state(k)
        assert dims_after[k] == xd.shape[0] == xh.shape[0] == mdl.dim == f["x1"].shape[0], (k, n)
        hx, hP = errors(xh, Ph, mdl.x, mdl.P)
        dx, dP = errors(xd, Pd, mdl.x, mdl.P)
        worst["x"], worst["P"] = max(worst["x"], ratio(dx, hx)), max(worst["P"], ratio(dP, hP))
        assert within(dx, hx) and within(dP, hP), (k, dx, hx, dP, hP)
    ens.close()
    hekf.close()
    hsim.close()
    print("ENS teacher-forced %s: 8 members of dims %s, worst device / host error ratio x %.3f P %.3f" % (key, sorted(dims), worst["x"], worst["P"]))


# ---- 2. tile and chunk edges --------------------------------------------------------------------------------------------------------
def synthetic_state(nf, seed):
    """test_gpu_ekf.py's generator: a pose near the origin, nf landmarks on a ring, a covariance shaped like a SLAM posterior (every
    landmark inherits the pose's uncertainty through a Jacobian of its own and adds a small block): symmetric positive definite"""
    rng = np.random.default_rng(seed)
    D = 3 + 2 * nf
    ang = np.linspace(0, 2 * np.pi, nf, endpoint=False) + 0.05
    rad = 20.0 + 5.0 * rng.random(nf)
    x = np.zeros(D)
    x[:3] = (0.3, -0.2, 0.1)
    x[3::2], x[4::2] = x[0] + rad * np.cos(ang), x[1] + rad * np.sin(ang)
    J = np.zeros((D, 3))
    J[:3] = np.eye(3)
    J[3:] = rng.normal(0, 1.0, (2 * nf, 3))
    P = J @ np.diag([0.05, 0.05, 0.002]) @ J.T
    for j in range(nf):
        a = rng.normal(0, 0.15, (2, 2))
        P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] += a @ a.T + 0.01 * np.eye(2)
    return x.astype(f32), mirrored(P.astype(f32))


def observations(x, idf, rng):
    f = 3 + 2 * np.asarray(idf, np.int64)
    dx, dy = x[f] - x[0], x[f + 1] - x[1]
    z = np.stack([np.sqrt(dx * dx + dy * dy) + rng.normal(0, 0.1, len(f)), np.arctan2(dy, dx) - x[2] + rng.normal(0, 0.01, len(f))], axis=1)
    return z.astype(f32)


_known = {}


def known_host():
    """a host filter with the association known and the heading observed (its simulator is only where its settings come from)"""
    if not _known:
        from slam_amd import host
        sim = host.HostSim(["-m", os.path.join(DATA, "example_loop1.mat"), "-method", "EKF1", "-SWITCH_ASSOCIATION_KNOWN", 1])
        _known.update(sim=sim, ekf=host.HostEkf(sim), noise=sim.sim_noise())
        assert sim.conf.SWITCH_ASSOCIATION_KNOWN == 1 and sim.conf.SWITCH_HEADING_KNOWN == 1
    return _known["sim"], _known["ekf"], _known["noise"]


# (the three members' landmark counts, observations of mapped features, new features): every nf of {0, 1, 14, 15, 30, 31, 62, 63, 64} --
# dimensions on both sides of 32, 64 and 128 floats --, every m of {0, 1, 3, 35, 64, 65, 100}, 0 / 1 / 5 new features
EDGE_CASES = [((0, 14, 64), 3, 1), ((1, 15, 63), 1, 5), ((30, 31, 62), 35, 0), ((14, 63, 64), 64, 1), ((15, 62, 64), 65, 0), ((31, 63, 64), 100, 5),
              ((0, 1, 30), 0, 1)]


HOST_DIM_MOST = 523  # the host's heading update is two naive dense D^3 products: beyond this dimension the float32 model is the yardstick


def tiles_and_chunks(nfs, m, nnew):
    """Known association, heading observed, three members of three sizes in one launch.  The ids are shared: the m observed ids are drawn
    from the largest member's features (with repeats once m exceeds them), a member observes those it holds and ignores the rest (the
    header's rule), and the new ids are new to everybody.  Per member the yardstick is the host filter on that member's own
    observations (its single batch, m <= 64, and a dimension of at most HOST_DIM_MOST before the step) or the float32 model with the
    device's chunks.  Shared with tests/test_gpu_ekf_scale.py"""
    import slam_amd
    import ekf_model
    sim, hekf, nz = known_host()
    c = sim.conf
    rng = np.random.default_rng(1000 * nfs[2] + m)
    nmax = max(nfs)
    cap_lm = nmax + 5
    big_x, _ = synthetic_state(nmax, 7 * nmax + m)
    ids_f = np.concatenate([rng.permutation(nmax) for _ in range(m // max(nmax, 1) + 1)])[:m].astype(np.int32) if nmax else np.zeros(0, np.int32)
    ids = np.concatenate([ids_f, nmax + np.arange(nnew)]).astype(np.int32)
    znew = np.stack([17.0 + np.arange(nnew), 0.4 - 0.3 * np.arange(nnew)], axis=1).astype(f32).reshape(-1, 2)
    B = 3
    ens = slam_amd.EkfEnsemble(B, cap_lm, **cfg_of(c))
    cap, ld = ens.cap_dim, ens.ld
    states, zs = [], []
    for b, nf in enumerate(nfs):
        x0, P0 = synthetic_state(nf, 7 * nf + m)
        states.append((x0, P0))
        # the member's own readings of the shared ids: real ones for the features it holds, anything for those it ignores
        zb = observations(big_x, ids_f, rng) if m else np.zeros((0, 2), f32)
        own = ids_f < nf
        if own.any():
            zb[own] = observations(x0, ids_f[own], rng)
        zs.append(np.concatenate([zb, znew]))
    for b in np.argsort(nfs):  # the largest last: the shared table then knows every feature
        ens.upload(b, np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))
        ens.upload(b, *states[b])
    V, G, phi = 3.0, 0.05, 0.104
    ens.sim(tile([V, G], B), np.full(B, phi, f32), nz["Qe"], nz["dt"], np.stack(zs), ids, nz["Re"], nz["R"], 1)
    assert not ens.status().any()
    dims = ens.dims()
    for b, nf in enumerate(nfs):
        x0, P0 = states[b]
        own = np.concatenate([ids_f < nf, np.ones(nnew, bool)])
        zo, io = zs[b][own], ids[own]
        mo = int((ids_f < nf).sum())
        args = (V, G, nz["Qe"], nz["dt"], phi, zo, io, nz["Re"], nz["R"], 1)
        mdl = ekf_model.EkfModel(**cfg_of(c), chunk=64)
        mdl.upload(x0, P0)
        mdl.sim(*args)
        D = 3 + 2 * (nf + nnew)
        assert mdl.dim == D == dims[b], (b, nf)
        if mo <= 64 and x0.shape[0] <= HOST_DIM_MOST:
            hekf.upload(x0, P0)
            hekf.sim_step(*args)
            xr, Pr = hekf.state(cap=D)
        else:
            m32 = ekf_model.EkfModel(**cfg_of(c), chunk=64, dtype=f32)
            m32.upload(x0, P0)
            m32.sim(*args)
            xr, Pr = m32.x, m32.P
            if mo <= 64:  # (the host's single batch exists and is merely slow, 1.5 s at dim 1017: its error beside the yardstick's, printed only)
                hekf.upload(x0, P0)
                hekf.sim_step(*args)
                print("ENS tiles nf %d m %d (+%d new): the host filter's error x %.3e P %.3e" % ((nf, mo, nnew) + errors(*hekf.state(cap=D), mdl.x, mdl.P)))
        xd, Pd = ens.state(b)
        assert xd.shape[0] == D and symmetric(Pd), (b, nf)
        # the padding: beyond dim the sentinel, beyond the capacity (never uploaded) the zeros the slab was made with
        xs, Ps = ens.slab(b)
        assert bits_equal(xs[:D], xd) and bits_equal(Ps[:D, :D], Pd)
        assert (xs[D:cap] == SENTINEL).all() and (xs[cap:] == 0).all()
        assert (Ps[D:, :cap] == SENTINEL).all() and (Ps[:, D:cap] == SENTINEL).all() and (Ps[:, cap:] == 0).all()
        rx, rP = errors(xr, Pr, mdl.x, mdl.P)
        dx, dP = errors(xd, Pd, mdl.x, mdl.P)
        print("ENS tiles nf %d m %d (+%d new): device x %.3e P %.3e, yardstick x %.3e P %.3e, ratio x %.3f P %.3f" %
              (nf, mo, nnew, dx, dP, rx, rP, ratio(dx, rx), ratio(dP, rP)))
        assert within(dx, rx) and within(dP, rP), (b, nf, dx, rx, dP, rP)
    ens.close()


@pytest.mark.parametrize("nfs,m,nnew", EDGE_CASES)
def test_tiles_and_chunks(nfs, m, nnew):
    tiles_and_chunks(nfs, m, nnew)


def test_a_neighbours_slab_is_untouched():
    """The gates, zero motion (V = 0, Q = 0: the predict stage is the identity, bit for bit), three members: only the middle one holds a
    feature the observation gates with; with the augment gate out of reach the others discard it, and their slabs -- state, padding
    and all -- keep every bit"""
    import slam_amd
    ens = slam_amd.EkfEnsemble(3, 6, gate_reject=4.0, gate_augment=1e30)
    cap = ens.cap_dim
    x1, P1 = synthetic_state(4, 11)
    z = observations(x1, [2], np.random.default_rng(2))
    x0 = x1.copy()
    x0[3:] += 300.0  # the same map far away: nothing gates
    for b, x in enumerate((x0, x1, x0)):
        ens.upload(b, np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))
        ens.upload(b, x, P1)
    before = [ens.slab(b) for b in range(3)]
    R = np.array([[0.01, 0], [0, 0.0003]], f32)
    ens.sim(np.zeros((3, 2), f32), np.zeros(3, f32), Q0, 0.025, tile(z, 3), None, R, R, 1)
    after = [ens.slab(b) for b in range(3)]
    for b in (0, 2):
        assert bits_equal(before[b][0], after[b][0]) and bits_equal(before[b][1], after[b][1]), b
    assert not bits_equal(before[1][1], after[1][1]) and list(ens.dims()) == [11, 11, 11] and not ens.status().any()
    D = 11
    assert (after[1][1][D:, :cap] == SENTINEL).all() and (after[1][1][:, D:cap] == SENTINEL).all() and symmetric(after[1][1][:D, :D])
    ens.close()


# ---- 3. gates -----------------------------------------------------------------------------------------------------------------------
def test_gates_match_the_reference_decisions():
    """tests/golden/kat_assoc.npz through the ensemble: the particles of a group are the members of one launch (pose known: P =
    blockdiag(0, Pf_j)), zero motion.  batch_update = 0: the new dimension and the appended features are the NEW labels'.  batch_update =
    1: the matches show through the changed state, which must be the float64 model's given the reference's labels -- a wrong or a
    missed match moves a landmark by the size of an innovation, decimetres, against the 1e-3 (of max |x|, of max |P|) allowed here
    for a float32 update of at most 11 observations.  The single filter's clear-margin rule and caps: margin > 1e-3, >= 1 600 decisions
    checked, <= 40 skipped; a member with an unclear decision is not looked at."""
    import slam_amd
    import assoc_float64 as A
    import ekf_model
    kat = np.load(os.path.join(GOLDEN, "kat_assoc.npz"))
    g1, g2 = (float(x) for x in kat["gates"])
    R = np.array([[0.1 ** 2, 0], [0, 0.017453292519943 ** 2]], f32)
    checked = skipped = 0
    for g in range(int(kat["n_groups"])):
        xv, xf, Pf, z, lab = (kat["g%d_%s" % (g, k)] for k in ("xv", "xf", "Pf", "z", "lab"))
        N, nf, nzg = xv.shape[0], xf.shape[1], z.shape[0]
        assert N <= 64
        D = 3 + 2 * nf
        states = []
        for i in range(N):
            x = np.concatenate([xv[i], xf[i].reshape(-1)]).astype(f32)
            P = np.zeros((D, D), f32)
            for j in range(nf):
                P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] = Pf[i][j]
            states.append((x, mirrored(P)))
        clear = np.array([A.associate(xv[i], xf[i], Pf[i], z, R, g1, g2, want_margin=True)[1] > 1e-3 for i in range(N)])
        for batch in (0, 1):
            ens = slam_amd.EkfEnsemble(N, nf + nzg, batch_update=bool(batch), gate_reject=g1, gate_augment=g2)
            for i in range(N):
                ens.upload(i, *states[i])
            ens.sim(np.zeros((N, 2), f32), np.zeros(N, f32), Q0, 0.025, tile(z, N), None, R, R, 1)
            dims = ens.dims()
            assert not ens.status().any()
            for i in range(N):
                if not clear[i].all():
                    continue
                new = lab[i] == -1
                assert dims[i] == D + 2 * int(new.sum()), (g, i, batch)
                xd, Pd = ens.state(i)
                mdl = ekf_model.EkfModel(batch_update=bool(batch), association_known=True)  # the reference's labels, forced
                mdl.upload(*states[i])
                ids =np.where(lab[i] >= 0, lab[i], np.where(new, 1000 + np.arange(nzg), -5)).astype(np.int64)
                keep = lab[i] != -2
                mdl.sim(0.0, 0.0, Q0, 0.025, 0.0, z[keep], ids[keep], R, R, 1)
                assert mdl.dim == dims[i]
                ex, eP = errors(xd, Pd, mdl.x, mdl.P)
                assert ex <= 1e-3 and eP <= 1e-3, (g, i, batch, ex, eP)
            ens.close()
        checked += int(clear.sum())
        skipped += int((~clear).sum())
    print("ENS decisions: checked %d skipped %d" % (checked, skipped))
    assert checked >= 1600 and skipped <= 40, (checked, skipped)


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------
def _scenario(B, seed=4):
    """B members' inputs for three steps on a ten-landmark state: (states, steps)"""
    rng = np.random.default_rng(seed)
    x0, P0 = synthetic_state(10, 21)
    states = []
    for b in range(B):
        x = x0.copy()
        x[:3] += rng.normal(0, 0.02, 3).astype(f32)
        states.append((x, P0))
    steps = []
    for k in range(3):
        idf = rng.permutation(10)[:6]
        z = np.stack([np.concatenate([observations(states[b][0], idf, rng), np.array([[30.0 + k, 1.0 + 0.1 * k]], f32)]) for b in range(B)])
        steps.append(dict(VG=np.stack([3.0 + rng.normal(0, 0.3, B), rng.normal(0, 0.05, B)], axis=1).astype(f32), phi=(0.1 + rng.normal(0, 0.01, B)).astype(f32),
                          z=z, truth=np.array([0.3 + 0.07 * k, -0.2, 0.1], f32), ob=k != 1))
    return states, steps


def _run(members, states, steps, pick):
    """an ensemble of len(pick) members holding members `pick` of the scenario; returns per member (x, P, dim, accumulators)"""
    import slam_amd
    sim, _, nz = known_host()
    ens = slam_amd.EkfEnsemble(len(pick), 14, **cfg_of(sim.conf, association_known=False))
    for j, b in enumerate(pick):
        ens.upload(j, *states[b])
    for s in steps:
        ens.sim(s["VG"][pick], s["phi"][pick], nz["Qe"], nz["dt"], s["z"][pick], None, nz["Re"], nz["R"], s["ob"], truth=s["truth"])
    dims, acc = ens.dims(), ens.consistency()
    out = [ens.state(j) + (dims[j], acc[j]) for j in range(len(pick))]
    assert not ens.status().any()
    ens.close()
    return out


def same(a, b):
    return a[2] == b[2] and bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


def test_invariance():
    B = 64
    states, steps = _scenario(B)
    full = _run(B, states, steps, np.arange(B))
    assert full[0][2] > 3 + 2 * 10 and full[0][3][0] == 3  # landmarks appended, three steps counted
    assert not same(full[0], full[1])
    again = _run(B, states, steps, np.arange(B))
    assert all(same(a, b) for a, b in zip(full, again))  # two identical runs
    for b in (0, 1, 31, 63):  # a member alone
        assert same(_run(1, states, steps, np.array([b]))[0], full[b]), b
    perm = np.random.default_rng(8).permutation(B)
    moved = _run(B, states, steps, perm)
    assert all(same(moved[j], full[perm[j]]) for j in range(B))


# ---- 5. noise -----------------------------------------------------------------------------------------------------------------------
def test_noise_rule(oracle):
    """sim_noise's draws against ekf_ens_model.draw (the oracle's Philox integers, float64 Box-Muller).  Per normal g the device may be
    off by 6 * 2^-20: u01 >= 2^-25 bounds the amplitude sqrt(-2 ln u) by 5.9; the float angle 2 pi u is off by <= 2^-22 rad; logf,
    sinf and cosf are off by <= 2 ulp each, sqrtf and the products by half an ulp; in all < 5.9 * 2^-20.8, and the bound is twice
    that.  It enters the input scaled by its sigma (L00; |L10| and L11; sqrt R00, sqrt R11).  ON TOP of that |dg| rule, which speaks of
    the normal alone, storing the input in float32 adds half an ulp of the value per operation: 2 * 2^-24 |value| covers the product
    and the sum (twice that for G, two products).  The uniform is exact (u01 of the same word), and phi is held to 2^-24 relative."""
    import slam_amd
    import ekf_ens_model as E
    sim, _, nz = known_host()
    c = sim.conf
    B, seed, step = 8, 0xC0FFEE1234567, 3
    x0, P0 = synthetic_state(5, 9)
    zt = observations(x0, np.arange(5), np.random.default_rng(1))
    ids = np.arange(5, dtype=np.int32)
    Qc = np.array([[0.09, 0.004], [0.004, 0.0027]], f32)
    V, G, phit = 3.0, 0.1, 0.104

    def make(members=B, sd=seed):
        e = slam_amd.EkfEnsemble(members, 6, **cfg_of(c), seed=sd)
        for b in range(members):
            e.upload(b, x0, P0)
        return e

    def noisy(e, st=step, flags=7):
        e.sim_noise(V, G, phit, Qc, nz["dt"], st, zt, ids, nz["Re"], nz["R"], 1, Qe=nz["Qe"], noise=flags)
        return e.last_inputs()

    a = make()
    VGd, phid, zd = noisy(a)
    VGm, phim, zm, _ = E.draw(oracle.philox, seed, B, step, V, G, phit, zt, Qc, nz["R"], c.sigmaT, 7)
    l00, l10, l11 = E.chol2(Qc)
    bg, ul = 6.0 * 2.0 ** -20, 2.0 * 2.0 ** -24
    sr = np.sqrt(np.diag(nz["R"]).astype(f64))
    assert (np.abs(VGd[:, 0] - VGm[:, 0]) <= bg * l00 + ul * np.abs(VGm[:, 0])).all()
    assert (np.abs(VGd[:, 1] - VGm[:, 1]) <= bg * (abs(l10) + l11) + 2 * ul * np.abs(VGm[:, 1])).all()
    assert (np.abs(phid - phim) <= 2.0 ** -24 * np.abs(phim)).all() and c.sigmaT > 0, np.abs(phid - phim) / np.abs(phim)
    assert (np.abs(zd - zm) <= bg * sr + ul * np.abs(zm)).all()
    assert len({tuple(v) for v in VGd}) == B and len(set(phid)) == B and len({tuple(v.reshape(-1)) for v in zd}) == B
    # a second handle fed the read-back inputs through the explicit sim ends bit-identical
    b = make()
    b.sim(VGd, phid, nz["Qe"], nz["dt"], zd, ids, nz["Re"], nz["R"], 1)
    for m in range(B):
        (xa, Pa), (xb, Pb) = a.state(m), b.state(m)
        assert bits_equal(xa, xb) and bits_equal(Pa, Pb), m
    # all three noises off: the true values bit for bit, the members equal each other and the noise-free explicit step
    VG0, phi0, z0 = noisy(a, flags=0)
    assert bits_equal(VG0, tile([V, G], B)) and bits_equal(phi0, np.full(B, phit, f32)) and bits_equal(z0, tile(zt, B))
    b.sim(tile([V, G], B), np.full(B, phit, f32), nz["Qe"], nz["dt"], tile(zt, B), ids, nz["Re"], nz["R"], 1)
    for m in range(B):
        (xa, Pa), (xb, Pb) = a.state(m), b.state(m)
        assert bits_equal(xa, xb) and bits_equal(Pa, Pb), m
    # one noise at a time leaves the other inputs alone
    VG1, phi1, z1 = noisy(a, flags=1)
    assert not bits_equal(VG1, VG0) and bits_equal(phi1, phi0) and bits_equal(z1, z0)
    VG4, phi4, z4 = noisy(a, flags=4)
    assert bits_equal(VG4, VG0) and bits_equal(phi4, phi0) and not bits_equal(z4, z0)
    # another step, another seed: other draws; the same step again: the same draws; member b's draw does not depend on B
    assert not bits_equal(noisy(a, st=step + 1)[0], VGd) and bits_equal(noisy(a)[0], VGd)
    other = make(sd=seed + 1)
    assert not bits_equal(noisy(other)[0], VGd)
    small = make(members=3)
    VGs, phis, zs = noisy(small)
    assert bits_equal(VGs, VGd[:3]) and bits_equal(phis, phid[:3]) and bits_equal(zs, zd[:3])
    for e in (a, b, other, small):
        e.close()


# ---- 6. accumulators ----------------------------------------------------------------------------------------------------------------
def test_consistency_accumulators():
    """40 steps of a B = 8 run with `truth` (no heading update; at rest for the first three steps, so that Pvv = Gu Q Gu^T has rank 1 exactly
    and the steps are not counted): consistency() equals the float64 model (ekf_ens_model.accumulate: pose_model.nees's definitions)
    evaluated on poses() fetched after every step -- the counts exactly, the sums within 1e-12 relative: both are double evaluations of
    the same 3 x 3 formulas from the same float inputs"""
    import slam_amd
    import ekf_ens_model as E
    sim, _, nz = known_host()
    B = 8
    ens = slam_amd.EkfEnsemble(B, 4, **cfg_of(sim.conf, use_heading=False), seed=77)
    lm = np.array([[15.0, 5.0], [10.0, -12.0], [-8.0, 14.0], [25.0, 20.0]])
    acc = np.zeros((B, 6))
    t = np.zeros(3, f32)
    dt = nz["dt"]
    for k in range(40):
        V, G = (0.0, 0.0) if k < 3 else (3.0, 0.04)
        t = np.array([t[0] + V * dt * np.cos(G + t[2]), t[1] + V * dt * np.sin(G + t[2]), t[2] + V * dt * np.sin(G) / sim.conf.WHEELBASE], f32)
        ob = k % 8 == 7
        d = lm - t[:2].astype(f64)
        zt = np.stack([np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0]) - t[2]], axis=1).astype(f32)
        ens.sim_noise(V, G, float(t[2]), nz["Q"], dt, k, zt, np.arange(4), nz["Re"], nz["R"], ob, truth=t, Qe=nz["Qe"], noise=6 if k < 3 else 7)
        xyt, Pvv = ens.poses()
        E.accumulate(acc, xyt, Pvv, t)
    got = ens.consistency()
    assert np.array_equal(got[:, [0, 1, 3]], acc[:, [0, 1, 3]]), (got, acc)
    # the three steps at rest are not counted, whatever else is (the first step that moves leaves Pvv of rank 2 in exact arithmetic --
    # the vehicle starts at heading 0, where e_x and the two columns of Gu are dependent -- and rounding decides)
    assert (got[:, 1] >= 3).all() and (got[:, 1] <= 5).all() and (got[:, 0] + got[:, 1] == 40).all() and (ens.dims() == 11).all()
    assert np.allclose(got[:, [2, 4, 5]], acc[:, [2, 4, 5]], rtol=1e-12, atol=0), (got, acc)
    assert len(set(got[:, 2])) == B  # every member its own noise
    # a step without truth leaves them alone; the reset zeroes them
    ens.sim_noise(3.0, 0.0, float(t[2]), nz["Q"], dt, 40, None, None, nz["Re"], nz["R"], 0, truth=None, Qe=nz["Qe"])
    assert np.array_equal(ens.consistency(), got)
    ens.consistency_reset()
    assert not ens.consistency().any()
    ens.close()


# ---- 7. a whole run -----------------------------------------------------------------------------------------------------------------
def test_whole_run_matches_the_reference():
    """example_loop1 seed 3, B = 4: every member is fed the host run's own tape through the explicit sim.  The four members stay
    bit-identical, and member 0 meets the bounds test_gpu_ekf.py holds the single device filter to: the reference's dimension on every
    control step and the goldens' trajectory bounds"""
    import slam_amd
    import test_gpu_ekf as T
    run = T.host_run("loop1")
    g = load_golden(run["golden"])
    c, nz = run["conf"], run["noise"]
    B = 4
    ens = slam_amd.EkfEnsemble(B, run["nlm"], **cfg_of(c))
    assert len(run["steps"]) == g["x"].shape[0]
    for k, s in enumerate(run["steps"]):
        z = tile(s["z"], B) if s["ob"] else None
        ens.sim(tile([s["V"], s["G"]], B), np.full(B, s["phi"], f32), nz["Qe"], nz["dt"], z, s["vis"] if s["ob"] else None, nz["Re"], nz["R"], s["ob"])
        assert (ens.dims() == g["dim"][k]).all(), k
        xyt, _ = ens.poses()
        assert np.abs(xyt[0] - g["x"][k]).max() <= 1e-3, k
        if k % 50 == 0:
            _, P = ens.state(0)
            tr = np.trace(P.astype(f64))
            assert abs(tr - g["trace"][k]) <= 1e-3 * max(g["trace"][k], 1e-9), k
    x, P = ens.state(0)
    assert not ens.status().any() and symmetric(P)
    assert np.abs(x - g["final_x"]).max() <= 2e-3 and np.abs(P - g["final_P"]).max() <= 1e-3 * np.abs(g["final_P"]).max()
    for b in range(1, B):
        xb, Pb = ens.state(b)
        assert bits_equal(xb, x) and bits_equal(Pb, P), b
    ens.close()


# ---- 8. edges -----------------------------------------------------------------------------------------------------------------------
def test_edges():
    import slam_amd
    import ekf_ens_model as E
    sim, hekf, nz = known_host()
    c = sim.conf
    ctl = dict(Q=nz["Qe"], dt=nz["dt"])
    R, Re = nz["R"], nz["Re"]
    x0, P0 = synthetic_state(6, 3)
    rng = np.random.default_rng(11)
    z6 = observations(x0, np.arange(6), rng)

    # capacity overflow in one member only (the gates): member 1 is full, the observation is new to everybody
    B = 3
    ens = slam_amd.EkfEnsemble(B, 6, **cfg_of(c, association_known=False))
    x5, P5 = synthetic_state(5, 3)
    for b, (x, P) in enumerate(((x5, P5), (x0, P0), (x5, P5))):
        ens.upload(b, x, P)
    znew = np.array([[60.0, 2.5]], f32)
    VG, phi = tile([3.0, -0.02], B), np.full(B, 0.1, f32)
    ref = slam_amd.EkfEnsemble(1, 6, **cfg_of(c, association_known=False))  # member 1 with nothing observed: predict and heading alone
    ref.upload(0, x0, P0)
    ref.sim(VG[:1], phi[:1], ctl["Q"], ctl["dt"], None, None, Re, R, 1)
    z5 = observations(x5, [0, 1], rng)  # every member observes two features of its own and the new landmark
    zb = np.stack([np.concatenate([z5, znew]), np.concatenate([z6[:2], znew]), np.concatenate([z5, znew])])
    ens.sim(VG, phi, ctl["Q"], ctl["dt"], zb, None, Re, R, 1)
    assert list(ens.status()) == [0, slam_amd.EKF_STATUS_CAPACITY, 0] and list(ens.dims()) == [15, 15, 15]
    (xa, Pa), (xr, Pr) = ens.state(1), ref.state(0)
    assert bits_equal(xa, xr) and bits_equal(Pa, Pr)  # neither its update nor its augment was applied; its predict and heading were
    assert not bits_equal(ens.state(0)[1][:13, :13], P5)
    # nz = 0 with observe set is predict + heading: what `ref` just did equals a step without observe
    ref2 = slam_amd.EkfEnsemble(1, 6, **cfg_of(c, association_known=False))
    ref2.upload(0, x0, P0)
    ref2.sim(VG[:1], phi[:1], ctl["Q"], ctl["dt"], None, None, Re, R, 0)
    (xb, Pb) = ref2.state(0)
    assert bits_equal(xb, xr) and bits_equal(Pb, Pr) and not bits_equal(Pb, P0)
    # the next step goes on for everybody, the bit is sticky
    ens.sim(VG, phi, ctl["Q"], ctl["dt"], zb[:, :2], None, Re, R, 1)
    assert list(ens.status()) == [0, slam_amd.EKF_STATUS_CAPACITY, 0] and not bits_equal(ens.state(1)[1], Pa)
    ens.close()
    ref2.close()

    # NOT_PD in one member only: an indefinite P makes S indefinite, the chunk is skipped and flagged, the neighbours update
    ens = slam_amd.EkfEnsemble(B, 6, **cfg_of(c, use_heading=False))
    Pbad = P0.copy()
    Pbad[3:, 3:] = -4.0 * np.eye(12, dtype=f32)
    for b, P in enumerate((P0, Pbad, P0)):
        ens.upload(b, x0, P)
    ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:3], B), [0, 1, 2], Re, R, 1)
    assert list(ens.status()) == [0, 1, 0]
    xs, Ps = ens.state(1)
    assert bits_equal(xs, x0) and bits_equal(Ps, Pbad) and np.isfinite(Ps).all()
    (xa, Pa), (xc, Pc) = ens.state(0), ens.state(2)
    assert bits_equal(xa, xc) and bits_equal(Pa, Pc) and not bits_equal(Pa, P0) and symmetric(Pa)
    # bad arguments: SLAMGPU_ERR_INVALID, the state keeps every bit
    keep = [ens.state(b) for b in range(B)]
    bad = (lambda: ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), None, ctl["dt"], None, None, Re, R, 0),
           lambda: ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:1], B), None, Re, R, 1),      # known association, no ids
           lambda: ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:1], B), [-1], Re, R, 1),
           lambda: ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:1], B), [1 << 20], Re, R, 1),    # ids index a table
           lambda: ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:2], B), [9, 9], Re, R, 1),      # an unseen id twice
           lambda: ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:1], B), [0], None, R, 1),
           lambda: ens.sim_noise(1.0, 0.0, 0.0, Q0, ctl["dt"], 0, noise=1),                                              # Q has no Cholesky factor
           lambda: ens.sim_noise(1.0, 0.0, 0.0, ctl["Q"], ctl["dt"], 0, noise=8),
           lambda: ens.upload(3, x0, P0), lambda: ens.upload(-1, x0, P0), lambda: ens.upload(0, x0[:4], P0[:4, :4]),
           lambda: ens.upload(0, np.zeros(17, f32), np.zeros((17, 17), f32)), lambda: ens.state(3),
           lambda: slam_amd.EkfEnsemble(0, 4), lambda: slam_amd.EkfEnsemble(4, 513), lambda: slam_amd.EkfEnsemble(65536, 4))
    for call in bad:
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            call()
        assert ei.value.code == -1
    for b in range(B):
        xs, Ps = ens.state(b)
        assert bits_equal(xs, keep[b][0]) and bits_equal(Ps, keep[b][1]), b
    assert list(ens.status()) == [0, 1, 0]
    # (a refused call has not taught the table id 9:) the shared table is full -- six features handed out, capacity six -- so a new id is
    # refused for EVERY member, the smaller one included, and table and members stay together: predict alone (V = 0, Q = 0: the identity)
    x4, P4 = synthetic_state(4, 3)
    ens.upload(0, x4, P4)
    ens.upload(2, x0, P0)  # (the largest last: the table knows ids 0 .. 5)
    ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:1], B), [9], Re, R, 1)
    assert list(ens.status()) == [2, 3, 2] and list(ens.dims()) == [11, 15, 15]
    assert bits_equal(ens.state(0)[1], P4) and bits_equal(ens.state(2)[1], P0)
    ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, ctl["dt"], tile(z6[:1], B), [0], Re, R, 1)  # a known id goes on updating
    assert list(ens.dims()) == [11, 15, 15] and not bits_equal(ens.state(2)[1], P0)
    ens.close()

    # members = 1 and max_landmarks = 0: a filter of the pose alone; an observation of anything new does not fit
    one = slam_amd.EkfEnsemble(1, 0, **cfg_of(c, association_known=False))
    mdl = E.Ensemble(1, 0, **cfg_of(c, association_known=False))
    assert one.cap_dim == 3 and one.ld == 32
    for k in range(5):
        args = ([[3.0, 0.03]], [0.01 * k], ctl["Q"], ctl["dt"], z6[None, :1], None, Re, R, int(k == 3))
        one.sim(*args)
        mdl.sim(*args)
    xd, Pd = one.state(0)
    assert xd.shape[0] == 3 and symmetric(Pd) and list(one.status()) == [slam_amd.EKF_STATUS_CAPACITY] == list(mdl.status)
    ex, eP = errors(xd, Pd, mdl.m[0].x, mdl.m[0].P)
    assert ex <= 1e-5 and eP <= 1e-4, (ex, eP)  # five float32 steps of a 3-state filter against float64
    one.close()
    ref.close()
