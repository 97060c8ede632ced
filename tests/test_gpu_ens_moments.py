"""slamgpu_ens_moments on the GPU (include/slamgpu.h; slam_amd/csrc/ekf_ens.cpp: ekf_ens_mom_*): the sample mean and covariance of the
members' states and the mean of their P, against the float64 model of tests/ens_moments_model.py.  States are set with upload, so no
run is needed to reach a shape.
  1. exact data: every sum exact, every output the model's bits;  2. generic data within bounds derived here;  3. the same far from the
  origin (the pivot's doing);  4. the set J;  5. headings around +-pi;  6. read-only, deterministic, chunked;  7. after real steps;
  8. the gates;  9. refusals;  10. slam-backend.
The bounds of 2, 3 (ens_moments_model.bounds): u = 2^-53, factor 8, n the members counted, R_a the range of component a over J:
mean 8 n u (R_a + |mu_a|), scatter 8 n u R_a R_b, Pbar 8 n u max |P|.  The worst error / bound ratios are printed and kept in
profiles/ens_moments.txt."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

import ekf_ens_run_model as R
import ens_moments_model as M
from test_gpu_ekf_ens import Q0, cfg_of, known_host, observations, synthetic_state, tile

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NOT_PD, CAPACITY = 1, 2
DS = (3, 5, 15, 17, 31, 33, 73)  # 15 -> 17: a second 16-column block of d_ext; 31 -> 33: ld 32 -> 64


def same(a, b):
    return R.same_bits(np.ascontiguousarray(a, f64), np.ascontiguousarray(b, f64))


def make(B, max_landmarks, **over):
    import slam_amd
    return slam_amd.EkfEnsemble(B, max_landmarks, **cfg_of(known_host()[0].conf, **over))


def fill(ens, x, P):
    for b in range(x.shape[0]):
        ens.upload(b, x[b], P[b])


def model_of(ens, D, exclude=0):
    """(the model fed the device's own slabs, the largest finite |P| in them)"""
    xs, Ps = zip(*(ens.slab(b) for b in range(ens.members)))
    Ps = np.stack(Ps)
    return M.moments(np.stack(xs), Ps, ens.dims(), ens.status(), D, exclude), float(np.abs(Ps[np.isfinite(Ps)]).max())


def check_bits(got, m, what):
    assert (got["counted"], got["left_out"], got["pivot"]) == (m["counted"], m["left_out"], m["pivot"]), what
    for k in ("mean", "C", "Pbar"):
        assert same(got[k], m[k]), (what, k, np.abs(got[k] - m[k]).max())


def check_bounds(got, m, P_max, what):
    """(worst error / bound ratio of the mean, of C, of Pbar); the counts are exact"""
    assert (got["counted"], got["left_out"], got["pivot"]) == (m["counted"], m["left_out"], m["pivot"]), what
    bm, bC, bP = M.bounds(m, P_max)
    em = np.abs(got["mean"] - m["mean"])
    em[2] = abs(math.remainder(got["mean"][2] - m["mean"][2], M.TWO_PI))
    eC, eP = np.abs(got["C"] - m["C"]), np.abs(got["Pbar"] - m["Pbar"])
    assert (got["C"] == got["C"].T).all() and (got["Pbar"] == got["Pbar"].T).all(), what
    with np.errstate(divide="ignore", invalid="ignore"):
        r = [float(np.nanmax(np.where(b > 0, e / b, np.where(e > 0, np.inf, 0.0)))) for e, b in ((em, bm), (eC, bC), (eP, np.full_like(eP, bP)))]
    print("ENS moments %s: n %d, worst error / bound: mean %.4f C %.4f Pbar %.4f" % (what, m["counted"], *r))
    assert (em <= bm).all() and (eC <= bC).all() and (eP <= bP).all(), (what, r)
    return r


# ---- 1. exact data ------------------------------------------------------------------------------------------------------------------------
def dyadic(B, D, seed):
    """integers x 2^-6: positions within +-4, headings within +-0.5 (so within +-1 of the pivot's: the remainder is exact), P symmetric"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-256, 257, (B, D)) / 64.0
    x[:, 2] = rng.integers(-32, 33, B) / 64.0
    A = rng.integers(-256, 257, (B, D, D)) / 64.0
    P = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)
    return x.astype(f32), P.astype(f32)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", [1, 2, 64, 256, 1024])
def test_exact_data_gives_the_models_bits(B, D):
    """n a power of two, every entry a small dyadic number: every sum, product and division is exact in double, so the order of the sums
    does not matter and every output equals the model's bits -- a wrong lane map of the matrix instruction or a wrong mirror cannot
    pass.  The handle's capacity is D (D = capacity), and the next smaller D of the list is asked of the same handle (D < capacity)"""
    x, P = dyadic(B, D, 100 * D + B)
    ens = make(B, (D - 3) // 2)
    fill(ens, x, P)
    dims, st = np.full(B, D), np.zeros(B, int)
    check_bits(ens.moments(D), M.moments(x, P, dims, st, D), (B, D))
    if D > 3:
        Ds = DS[DS.index(D) - 1]
        check_bits(ens.moments(Ds), M.moments(x, P, dims, st, Ds), (B, D, Ds))
    assert ens.moments()["mean"].shape == (D,)  # the default D: the smallest member's dimension
    ens.close()


@pytest.mark.parametrize("B, D, room", [(64, 131, 2), (16, 323, 0)])
def test_exact_data_wide(B, D, room):
    """the Gram pass is compiled for d_ext of up to 128, 320 and 1 088 columns: D = 131 (nine 16-column blocks, 45 block pairs in three
    groups, ld 160, capacity two landmarks above D) and D = 323 (21 blocks, 231 block pairs, ld 352) take the second and the third form"""
    x, P = dyadic(B, D, 7)
    ens = make(B, (D - 3) // 2 + room)
    fill(ens, x, P)
    check_bits(ens.moments(D), M.moments(x, P, np.full(B, D), np.zeros(B, int), D), (B, D))
    ens.close()


# ---- 2, 3. generic data, and the same far from the origin ------------------------------------------------------------------------------------
def generic(B, D, seed, shift):
    """random float32 states around one SLAM-like state (positions metres apart, headings within a radian), one symmetric positive P
    per member; shift: every position -- the pose's and the landmarks' -- moved by (1e5, -1e5) m before the rounding to float32"""
    rng = np.random.default_rng(seed)
    x = 20.0 * rng.standard_normal(D) + rng.standard_normal((B, D)) * rng.uniform(0.05, 2.0, D)
    x[:, 2] = 0.4 + 0.3 * rng.standard_normal(B)
    if shift:
        x[:, 0] += 1e5
        x[:, 1] -= 1e5
        x[:, 3::2] += 1e5
        x[:, 4::2] -= 1e5
    A = rng.standard_normal((D, D)) / math.sqrt(D)
    P0 = A @ A.T + 0.05 * np.eye(D)
    P = (P0[None] * rng.uniform(0.5, 1.5, (B, 1, 1))).astype(f32)
    return x.astype(f32), np.tril(P) + np.tril(P, -1).transpose(0, 2, 1)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("B", [3, 63, 65, 255, 257, 1025])
def test_generic_data_within_the_bounds(B, D, shift):
    """sizes on both sides of a sub-tile of four, of a wave and of a tile (two tiles at 257, five at 1 025).  shift: the scatter stays
    inside the same bound 8 n u R_a R_b, which has no |mu| in it: the deviations are taken from the pivot member in double before
    anything is squared, so 1e5 m of offset cost nothing"""
    x, P = generic(B, D, 1000 * D + B, shift)
    ens = make(B, (D - 3) // 2)
    fill(ens, x, P)
    m = M.moments(x, P, np.full(B, D), np.zeros(B, int), D)
    check_bounds(ens.moments(D), m, float(np.abs(P).max()), "generic B %d D %d%s" % (B, D, " shifted" if shift else ""))
    ens.close()


# ---- 4. the set J ----------------------------------------------------------------------------------------------------------------------------
def test_set_J():
    """Known association, eight members of 6 landmarks.  Member 1 refuses a chunk for real (an indefinite P: SLAMGPU_EKF_STATUS_NOT_PD);
    then member 0 gets a NaN in x[7], member 2 an Inf in x[1], member 3 a state of 4 landmarks (dim 11), member 4 a NaN at P[4][4]; later a
    new id finds the shared table full and EVERY member carries SLAMGPU_EKF_STATUS_CAPACITY.  A second handle with the gates has one
    full member that refuses a step alone"""
    import slam_amd
    sim, _, nz = known_host()
    B = 8
    ens = make(B, 6, use_heading=False)
    x0, P0 = synthetic_state(6, 3)
    x4, P4 = synthetic_state(4, 3)
    rng = np.random.default_rng(4)
    Pbad = P0.copy()
    Pbad[3:, 3:] = -4.0 * np.eye(12, dtype=f32)
    xs = (x0[None] + rng.normal(0, 0.05, (B, 15))).astype(f32)
    for b in range(B):
        ens.upload(b, xs[b], Pbad if b == 1 else (P0 * f32(1.0 + 0.1 * b)))
    z = observations(x0, np.arange(3), rng)
    ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, nz["dt"], tile(z, B), [0, 1, 2], nz["Re"], nz["R"], 1)
    assert list(ens.status()) == [0, NOT_PD] + [0] * 6
    xa, Pa = ens.state(0)
    xa[7] = np.nan
    xc, Pc = ens.state(2)
    xc[1] = np.inf
    xe, Pe = ens.state(4)
    Pe[4, 4] = np.nan
    ens.upload(3, x4, P4)
    ens.upload(0, xa, Pa)
    ens.upload(2, xc, Pc)
    ens.upload(4, xe, Pe)  # (a member of 6 landmarks last: the table knows ids 0 .. 5)
    assert list(ens.dims()) == [15, 15, 15, 11, 15, 15, 15, 15]
    want = {(15, 0): [1, 5, 6, 7], (15, NOT_PD): [5, 6, 7], (11, 0): [1, 3, 5, 6, 7], (7, 0): [0, 1, 3, 5, 6, 7], (3, 0): [0, 1, 3, 4, 5, 6, 7],
            (3, NOT_PD): [0, 3, 4, 5, 6, 7], (15, CAPACITY): [1, 5, 6, 7]}
    for (D, mask), J in want.items():
        m, P_max = model_of(ens, D, mask)
        assert (m["counted"], m["left_out"], m["pivot"]) == (len(J), B - len(J), J[0]), (D, mask)
        check_bounds(ens.moments(D, exclude_status=mask), m, P_max, "set J D %d mask %d" % (D, mask))
    # the shared table is full: a new id is refused for every member, whatever its state
    ens.sim(np.zeros((B, 2), f32), np.zeros(B, f32), Q0, nz["dt"], tile(z[:1], B), [9], nz["Re"], nz["R"], 1)
    assert list(ens.status()) == [CAPACITY, NOT_PD | CAPACITY] + [CAPACITY] * 6
    check_bounds(ens.moments(15), *model_of(ens, 15), "set J after the refusal, mask 0")
    got = ens.moments(15, exclude_status=NOT_PD)
    assert (got["counted"], got["left_out"], got["pivot"]) == (3, 5, 5)
    for mask in (CAPACITY, NOT_PD | CAPACITY):  # everyone excluded: NaN, (0, B, -1), and the call succeeds
        got = ens.moments(15, exclude_status=mask)
        assert (got["counted"], got["left_out"], got["pivot"]) == (0, B, -1), mask
        assert np.isnan(got["mean"]).all() and np.isnan(got["C"]).all() and np.isnan(got["Pbar"]).all(), mask
    ens.close()

    # the gates: member 1 is full and the observation is new to everybody -- it alone refuses (tests/test_gpu_ekf_ens.py: test_edges)
    c = sim.conf
    g = slam_amd.EkfEnsemble(3, 6, **cfg_of(c, association_known=False))
    x5, P5 = synthetic_state(5, 3)
    x6, P6 = synthetic_state(6, 3)
    for b, (x, P) in enumerate(((x5, P5), (x6, P6), (x5, P5))):
        g.upload(b, x, P)
    z5, z6 = observations(x5, [0, 1], rng), observations(x6, [0, 1], rng)
    znew = np.array([[60.0, 2.5]], f32)
    zb = np.stack([np.concatenate([z5, znew]), np.concatenate([z6, znew]), np.concatenate([z5, znew])])
    VG, phi = tile([3.0, -0.02], 3), np.full(3, 0.1, f32)
    g.sim(VG, phi, nz["Qe"], nz["dt"], zb, None, nz["Re"], nz["R"], 1)
    assert list(g.status()) == [0, CAPACITY, 0] and list(g.dims()) == [15, 15, 15]
    for mask, J in ((0, [0, 1, 2]), (NOT_PD, [0, 1, 2]), (CAPACITY, [0, 2]), (NOT_PD | CAPACITY, [0, 2])):
        m, P_max = model_of(g, 3, mask)
        assert (m["counted"], m["pivot"]) == (len(J), J[0]), mask
        check_bounds(g.moments(3, exclude_status=mask), m, P_max, "gates mask %d" % mask)
    # n = 1: member 0 loses its state, member 1 its status: member 2 alone -- C is exactly 0, the mean is its state, Pbar its P
    xa, Pa = g.state(0)
    xa[0] = np.nan
    g.upload(0, xa, Pa)
    got = g.moments(15, exclude_status=CAPACITY)
    x2, P2 = g.state(2)
    assert (got["counted"], got["left_out"], got["pivot"]) == (1, 2, 2)
    assert same(got["C"], np.zeros((15, 15))) and same(got["mean"], x2.astype(f64)) and same(got["Pbar"], P2.astype(f64))
    g.close()


# ---- 5. heading ------------------------------------------------------------------------------------------------------------------------------
def test_headings_around_pi():
    """257 members with headings within 0.3 rad of +-pi, on both sides: every deviation is taken the short way round, so the spread is
    that of 0.6 rad (a single u off by 2 pi would add (2 pi)^2 / 257 = 0.15 to C_22, whose largest honest value is 0.3^2), and the mean
    heading is the model's within the bound, modulo 2 pi"""
    B, D = 257, 5
    x, P = generic(B, D, 55, False)
    rng = np.random.default_rng(56)
    th = math.pi + rng.uniform(-0.3, 0.3, B)
    x[:, 2] = np.where(th > math.pi, th - 2 * math.pi, th).astype(f32)
    assert (x[:, 2] > 2.8).sum() > 50 and (x[:, 2] < -2.8).sum() > 50
    ens = make(B, 1)
    fill(ens, x, P)
    m = M.moments(x, P, np.full(B, D), np.zeros(B, int), D)
    got = ens.moments(D)
    check_bounds(got, m, float(np.abs(P).max()), "headings around pi")
    assert 0.0 < got["C"][2, 2] <= 0.09 and -math.pi < got["mean"][2] <= math.pi and abs(abs(got["mean"][2]) - math.pi) < 0.1
    ens.close()


# ---- 6. read-only and deterministic --------------------------------------------------------------------------------------------------------
def test_read_only_deterministic_and_chunked(monkeypatch):
    """600 members (three tiles), D = 73 (15 block pairs, 15 row blocks of P).  A step first, so that the accumulators, the trace and
    last_inputs hold something.  Nothing in the handle changes; two calls, chunks of 1 and of 3 (SLAMGPU_ENS_MOMENTS_CHUNK) and the calls
    without C or without Pbar give the same bits"""
    B, D = 600, 73
    x, P = generic(B, D, 66, False)
    ens = make(B, 35)
    fill(ens, x, P)
    ens.trace_enable(4)
    nz = known_host()[2]
    ens.sim_noise(1.0, 0.01, 0.4, nz["Q"], nz["dt"], 0, None, None, nz["Re"], nz["R"], 0, truth=x[0, :3], Qe=nz["Qe"])
    before = R.snapshot(ens)
    a = ens.moments(D)
    b = ens.moments(D)
    for k in ("mean", "C", "Pbar"):
        assert same(a[k], b[k]), k
    for chunk in ("1", "3"):
        monkeypatch.setenv("SLAMGPU_ENS_MOMENTS_CHUNK", chunk)
        c = ens.moments(D)
        monkeypatch.delenv("SLAMGPU_ENS_MOMENTS_CHUNK")
        for k in ("mean", "C", "Pbar"):
            assert same(a[k], c[k]), (chunk, k)
        assert (c["counted"], c["left_out"], c["pivot"]) == (B, 0, 0)
    noC, noP, neither = ens.moments(D, want_C=False), ens.moments(D, want_Pbar=False), ens.moments(D, want_C=False, want_Pbar=False)
    assert noC["C"] is None and noP["Pbar"] is None and neither["C"] is None and neither["Pbar"] is None
    assert same(noC["mean"], a["mean"]) and same(noC["Pbar"], a["Pbar"]) and same(noP["mean"], a["mean"]) and same(noP["C"], a["C"])
    assert same(neither["mean"], a["mean"]) and neither["counted"] == B
    assert same(ens.moments(D)["C"], a["C"])  # ... and after them
    assert not R.identical(before, R.snapshot(ens))
    check_bounds(a, *model_of(ens, D), "after a step, B 600 D 73")
    ens.close()


# ---- 7. after real steps -----------------------------------------------------------------------------------------------------------------------
def test_after_real_steps():
    """eight members, known association: 20 steps of sim_noise, then 12 more in one run_noise; moments() against the model fed from
    state(b), and its pose block against poses()"""
    from test_gpu_ekf_ens_run import LM
    sim, _, nz = known_host()
    B = 8
    ens = make(B, 8, seed=77)
    ob = {2: [0, 1], 5: [1, 2, 3], 9: [0, 4], 14: [2, 5, 6], 19: [0, 1, 7], 24: [3, 4, 5], 30: [0, 6, 7]}
    tape = R.world_tape(32, ob, nz["dt"], sim.conf.WHEELBASE, LM, seed=5)
    R.drive_single(ens, tape[:20], nz)
    R.drive_run(ens, tape[20:], nz)
    dims = ens.dims()
    D = int(dims[0])
    assert (dims == D).all() and D == 19 and not ens.status().any()
    x, P = zip(*(ens.state(b) for b in range(B)))
    x, P = np.stack(x), np.stack(P)
    m = M.moments(x, P, dims, np.zeros(B, int), D)
    got = ens.moments()
    P_max = float(np.abs(P).max())
    check_bounds(got, m, P_max, "after 32 real steps")
    xyt, Pvv = ens.poses()
    assert np.abs(got["mean"][:2] - xyt[:, :2].mean(0)).max() <= 8 * B * M.U * np.abs(xyt[:, :2]).max() * 2
    assert abs(math.remainder(got["mean"][2] - xyt[:, 2].mean(), M.TWO_PI)) <= 8 * B * M.U * 4  # (the headings of this run lie together)
    assert np.abs(got["Pbar"][:3, :3] - Pvv.mean(0)).max() <= 8 * B * M.U * P_max
    assert got["C"][0, 0] > 0 and got["C"][3, 3] > 0  # every member its own noise: a real spread
    ens.close()


# ---- 8. the gates --------------------------------------------------------------------------------------------------------------------------------
def test_gates_members_of_different_dimensions():
    """five members of 2, 4, 4, 6 and 3 landmarks: D = 3 counts them all; D = smallest + 2 leaves the short one out; D = 15 keeps one"""
    nfs = (2, 4, 4, 6, 3)
    ens = make(len(nfs), 6, association_known=False)
    for b, nf in enumerate(nfs):
        xb, Pb = synthetic_state(nf, 10 + b)
        ens.upload(b, xb, Pb)
    assert list(ens.dims()) == [7, 11, 11, 15, 9]
    for D, J in ((3, [0, 1, 2, 3, 4]), (9, [1, 2, 3, 4]), (11, [1, 2, 3]), (15, [3])):
        m, P_max = model_of(ens, D)
        assert (m["counted"], m["pivot"]) == (len(J), J[0]), D
        check_bounds(ens.moments(D), m, P_max, "gates D %d" % D)
    assert ens.moments()["mean"].shape == (7,) and ens.moments()["counted"] == 5
    ens.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import slam_amd
    ens = make(4, 6)
    L = ens.L
    mean, Cm, Pb = np.full(15, 7.5), np.full((15, 15), 7.5), np.full((15, 15), 7.5)
    n = [C.c_int32(-9), C.c_int32(-9), C.c_int32(-9)]

    def call(D, mean_p=mean.ctypes.data):
        return L.slamgpu_ens_moments(ens.h, D, 0, mean_p, Cm.ctypes.data, Pb.ctypes.data, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]))

    for D in (4, 14, 2, 1, 0, -3, 17, 16):  # even, below 3, above the capacity of 15
        assert call(D) == -1 and ("D %d" % D).encode() in L.slamgpu_last_error(), D
    assert call(15, None) == -1 and b"null mean" in L.slamgpu_last_error()
    assert (mean == 7.5).all() and (Cm == 7.5).all() and (Pb == 7.5).all() and [v.value for v in n] == [-9, -9, -9]
    with pytest.raises(slam_amd.SlamGpuError) as ei:
        ens.moments(4)
    assert ei.value.code == -1
    assert call(15) == 0 and [v.value for v in n] == [0, 4, -1] and np.isnan(mean).all()  # fresh members have dim 3: nobody reaches D = 15
    assert call(3) == 0 and [v.value for v in n] == [4, 0, 0] and (mean[:3] == 0).all() and np.isnan(mean[3:]).all()
    ens.close()


# ---- 10. slam-backend ----------------------------------------------------------------------------------------------------------------------------
def read_moments(path):
    rows = open(path).read().split("\n")
    D = int(rows[0])
    mean = np.array(rows[1].split(), f64)
    mats = np.array([r.split() for r in rows[2:2 + 2 * D]], f64)
    return D, mean, mats[:D], mats[D:]


@pytest.mark.parametrize("known", [0, 1])
def test_backend_prints_the_summary_of_what_it_writes(tmp_path, known):
    """the first 300 control steps of example_loop1, 8 members (the run of the existing ensemble CLI test), with the gates (D = 3) and with the
    known association (the whole state, the landmark bias).  The printed figures are moments_summary of the file; the file is what a
    Python-driven twin gets -- the simulator's noise-free tape replayed through sim_noise on a handle with the backend's settings --
    within the bounds of case 2"""
    import slam_amd
    from slam_amd import host
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    m, out = os.path.join(DATA, "example_loop1.mat"), str(tmp_path / "moments.txt")
    extra = ["-SWITCH_ASSOCIATION_KNOWN", "1"] if known else []
    r = subprocess.run([exe, "-m", m, "-method", "EKF1", "-ekf", "device", "-runs", "8", "-maxsteps", "300", "-RUNS_MOMENTS", "1", "-RUNS_MOMENTS_OUT", out,
                        *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ensemble moments:")]
    assert len(line) == 1, r.stdout
    line = line[0]
    D, mean, Cm, Pb = read_moments(out)
    assert "D %d, members counted 8, left out 0;" % D in line
    # the twin
    args = ["-m", m, "-method", "EKF1", *extra]
    user = host.HostSim(args)
    flags = (1 if user.conf.SWITCH_CONTROL_NOISE else 0) | 2 | (4 if user.conf.SWITCH_SENSOR_NOISE else 0)
    user.close()
    sim = host.HostSim(args + ["-SWITCH_CONTROL_NOISE", 0, "-SWITCH_SENSOR_NOISE", 0])
    nz, c = sim.sim_noise(), sim.conf
    assert bool(c.SWITCH_ASSOCIATION_KNOWN) == bool(known)
    ens = slam_amd.EkfEnsemble(8, sim.nlm if known else sim.nlm + 8, **cfg_of(c), seed=int(c.SWITCH_SEED_RANDOM))
    order, truth = [], None
    for k in range(300):
        rr, _, _, phi = sim.control()
        assert rr >= 0
        V, G = sim.true_controls()
        z, vis = None, None
        if rr == 1:
            sim.observe(0)
            z, vis = sim.last_z()
            order += [int(i) for i in vis if int(i) not in order]
        truth = sim.true_pose()
        ens.sim_noise(V, G, phi, nz["Q"], nz["dt"], k, z, vis, nz["Re"], nz["R"], rr, truth=truth, Qe=nz["Qe"], noise=flags)
    assert D == (int(ens.dims().min()) if known else 3) and (D > 3) == bool(known)
    twin = ens.moments(D)
    x, P = zip(*(ens.state(b) for b in range(8)))
    mdl = M.moments(np.stack([v[:D] for v in x]), np.stack([v[:D, :D] for v in P]), np.full(8, D), np.zeros(8, int), D)
    check_bounds(dict(twin, mean=mean, C=Cm, Pbar=Pb), mdl, float(max(np.abs(v).max() for v in P)), "backend file, known %d" % known)
    lm = sim.map()[0].astype(f64)[:, order[:(D - 3) // 2]].T if known else None  # (feature f is the f-th id the run named)
    s = slam_amd.moments_summary(mean, Cm, Pb, truth_pose=truth, truth_landmarks=lm)
    num = r"(-?[0-9.]+|-?nan|-?inf)"
    g = re.search(r"position %s, heading %s, per feature mean %s smallest %s largest %s; largest \|correlation\| of C %s, of Pbar %s; "
                  r"bias of the mean: position %s m, heading %s rad" % ((num,) * 9), line)
    assert g, line
    keys = ("pos_ratio", "heading_ratio", "feature_ratio_mean", "feature_ratio_min", "feature_ratio_max", "max_corr_C", "max_corr_Pbar", "bias_pos",
            "bias_heading")
    for k, txt in zip(keys, g.groups()):
        v = float(txt)
        assert (math.isnan(v) and math.isnan(s[k])) or abs(v - s[k]) <= 5.1e-7 + 1e-6 * abs(s[k]), (k, txt, s[k])
    if not known:
        assert "landmarks: not summarised (D = 3)" in line
    else:
        g = re.search(r"mean landmark distance %s m" % num, line)
        assert g, line
        assert abs(float(g.group(1)) - s["bias_landmarks"]) <= 5.1e-7
    ens.close()
    sim.close()
