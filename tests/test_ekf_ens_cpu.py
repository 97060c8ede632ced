"""The device EKF ensemble (include/slamgpu.h: slamgpu_ens_*), what can be checked without a GPU: the model the GPU tests measure
against (tests/ekf_ens_model.py) against itself -- one member on explicit inputs IS ekf_model.EkfModel, the noise rule has the
moments Q and R imply, the accumulators count what they should --, the symbols and the binding, slam-backend's refusals, and
ekf_ens.cpp compiled for gfx950 with a private segment of 0 bytes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

f32 = np.float32
Q = np.array([[0.3 ** 2, 0.0], [0.0, (3.0 * np.pi / 180) ** 2]], f32)
R = np.array([[0.1 ** 2, 0.0], [0.0, (1.0 * np.pi / 180) ** 2]], f32)
ENS_SYMBOLS = ["slamgpu_ens_create", "slamgpu_ens_destroy", "slamgpu_ens_sync", "slamgpu_ens_sim", "slamgpu_ens_sim_noise", "slamgpu_ens_last_inputs",
               "slamgpu_ens_dims", "slamgpu_ens_poses", "slamgpu_ens_state", "slamgpu_ens_slab", "slamgpu_ens_upload", "slamgpu_ens_status",
               "slamgpu_ens_consistency", "slamgpu_ens_consistency_reset"]


@pytest.mark.parametrize("heading", [False, True])
def test_one_member_on_explicit_inputs_is_the_single_model(heading):
    """B = 1: the ensemble model and EkfModel, fed the same 60 steps (known association, heading observed, landmarks appearing), agree bit
    for bit in x, P and the labels"""
    import ekf_ens_model as E
    import ekf_model
    cfg = dict(use_heading=heading, association_known=True, sigma_phi=0.01)
    ens, one = E.Ensemble(1, 6, **cfg), ekf_model.EkfModel(**cfg)
    rng = np.random.default_rng(5)
    lm = rng.uniform(-20, 20, (6, 2))
    truth = np.zeros(3)
    for k in range(60):
        V, G = (3.0 + 0.1 * rng.normal(), 0.05 * rng.normal()) if k >= 3 else (0.0, 0.0)  # at rest first: Pvv has rank 1, exactly
        truth = np.array([truth[0] + V * 0.025 * np.cos(G + truth[2]), truth[1] + V * 0.025 * np.sin(G + truth[2]), truth[2] + V * 0.025 * np.sin(G) / 4.0])
        ob = k % 8 == 7
        ids = np.arange(min(6, 1 + k // 10), dtype=np.int32)
        d = lm[ids] - truth[:2]
        z = np.stack([np.hypot(d[:, 0], d[:, 1]) + 0.1 * rng.normal(size=len(ids)), np.arctan2(d[:, 1], d[:, 0]) - truth[2]], axis=1)
        one.sim(V, G, Q, 0.025, truth[2], z, ids, R, R, ob)
        ens.sim([[V, G]], [truth[2]], Q, 0.025, z[None], ids, R, R, ob, truth=truth)
        assert ens.m[0].dim == one.dim and np.array_equal(ens.m[0].x, one.x) and np.array_equal(ens.m[0].P, one.P), k
    assert one.nf == 6 and ens.status[0] == 0
    # P = 0 at the start and a vehicle at rest: the first steps are not counted (the heading update's eps I makes them countable); later ones are
    assert ens.acc[0, 1] == (0 if heading else 3) and ens.acc[0, 0] + ens.acc[0, 1] == 60
    assert 0 <= ens.acc[0, 3] <= ens.acc[0, 0] and ens.acc[0, 2] > 0 and ens.acc[0, 4] > 0


def test_accumulator_model_is_the_pose_nees_definition():
    """ekf_ens_model.nees3 (the 3 x 3 Cholesky written out, the order the device evaluates) against pose_model.nees (the header's
    definitions through LAPACK) on random positive definite blocks; a singular, an indefinite and a NaN block are not counted"""
    import ekf_ens_model as E
    import pose_model
    rng = np.random.default_rng(3)
    for _ in range(50):
        A = rng.normal(size=(3, 3))
        P = (A @ A.T + 0.01 * np.eye(3)).astype(f32).astype(np.float64)
        P = np.tril(P) + np.tril(P, -1).T
        x, t = rng.normal(size=3).astype(f32), rng.normal(size=3).astype(f32)
        acc = np.zeros((1, 6))
        E.accumulate(acc, x[None].astype(np.float64), P[None], t)
        s = np.zeros(pose_model.STRIDE)
        s[1:4] = x
        s[6:12] = [P[0, 0], P[1, 0], P[1, 1], P[2, 0], P[2, 1], P[2, 2]]
        val, err, bad = pose_model.nees(s, t)
        assert bad == 0 and acc[0, 0] == 1 and abs(acc[0, 2] - val[0]) <= 1e-9 * val[0]
        assert abs(acc[0, 4] - (err[0, 0] ** 2 + err[0, 1] ** 2)) <= 1e-15 + 1e-12 * acc[0, 4] and abs(acc[0, 5] - err[0, 2] ** 2) <= 1e-15
        assert acc[0, 3] == (val[0] <= pose_model.CHI2_3_95)
    for P in (np.zeros((3, 3)), np.diag([1.0, 1.0, 0.0]), np.diag([1.0, -1.0, 1.0]), np.diag([1.0, np.nan, 1.0])):
        acc = np.zeros((1, 6))
        E.accumulate(acc, np.zeros((1, 3)), P[None], np.zeros(3, f32))
        assert list(acc[0]) == [0, 1, 0, 0, 0, 0]
    # a heading error across +-pi is the short way round
    acc = np.zeros((1, 6))
    E.accumulate(acc, np.array([[0.0, 0.0, np.pi - 0.05]]), np.eye(3)[None], np.array([0, 0, -np.pi + 0.05], f32))
    assert abs(acc[0, 5] - 0.01) < 1e-6 and abs(acc[0, 2] - 0.01) < 1e-6


def test_capacity_is_per_member_in_the_model():
    import ekf_ens_model as E
    ens = E.Ensemble(2, 1, association_known=True)
    z = np.array([[[10.0, 0.1], [12.0, -0.2]]] * 2)
    ens.sim(np.zeros((2, 2)), np.zeros(2), Q, 0.025, z[:, :1], [0], R, R, 1)
    assert list(ens.dims()) == [5, 5] and not ens.status.any()
    x0 = ens.m[0].x.copy()
    ens.sim(np.zeros((2, 2)), np.zeros(2), Q, 0.025, z, [0, 1], R, R, 1)  # a second landmark does not fit: the update is not applied either
    assert list(ens.dims()) == [5, 5] and list(ens.status) == [E.STATUS_CAPACITY] * 2 and np.array_equal(ens.m[0].x, x0)


def test_noise_rule_has_the_moments_of_Q_and_R(oracle):
    """4 096 members x 8 steps of the model's draws: every mean within 5 standard errors of its value (0 for the normals, sigma_phi / 2
    for the heading: the reference's draw is uncentred), every variance within 5 standard errors of the value Q and R imply
    (sigma^2 sqrt(2 / (N - 1)) for a normal, sigma_phi^2 / 12 with the uniform's fourth moment for the heading); and a noise that
    is off leaves the true value as it is"""
    import ekf_ens_model as E
    B, steps, sig = 4096, 8, 0.05
    Qc = np.array([[0.09, 0.004], [0.004, 0.0027]], f32)  # correlated: L10 matters
    zt = np.array([[12.5, 0.3]], f32)
    dv = []
    for s in range(steps):
        VG, phi, z, _ = E.draw(oracle.philox, 0x123456789ABCDEF, B, s, 3.0, 0.1, 0.7, zt, Qc, R, sig, 7)
        dv.append(np.concatenate([VG - np.array([float(f32(3.0)), float(f32(0.1))]), (phi - float(f32(0.7)))[:, None], z[:, 0] - zt[0].astype(np.float64)], axis=1))
    d = np.concatenate(dv)
    N = d.shape[0]
    var = np.array([Qc[0, 0], Qc[1, 1], sig * sig / 12.0, R[0, 0], R[1, 1]], np.float64)
    mean = np.array([0, 0, float(f32(sig)) / 2, 0, 0])
    kurt = np.array([2.0, 2.0, 0.8, 2.0, 2.0])  # var(s^2) = (m4 / sigma^4 - 1) sigma^4 / N: 2 for a normal, 0.8 for a uniform
    assert (np.abs(d.mean(0) - mean) <= 5 * np.sqrt(var / N)).all(), (d.mean(0), mean)
    assert (np.abs(d.var(0, ddof=1) - var) <= 5 * var * np.sqrt(kurt / (N - 1))).all(), (d.var(0, ddof=1), var)
    cov = np.mean(d[:, 0] * d[:, 1])
    assert abs(cov - Qc[0, 1]) <= 5 * np.sqrt((var[0] * var[1] + Qc[0, 1] ** 2) / N)
    VG, phi, z, g = E.draw(oracle.philox, 9, 4, 3, 3.0, 0.1, 0.7, zt, Qc, R, sig, 0)
    assert (VG == [float(f32(3.0)), float(f32(0.1))]).all() and (phi == float(f32(0.7))).all() and (z == zt.astype(np.float64)).all() and np.isnan(g).all()
    # streams: another step, another seed, another member draw something else; member b's draw does not depend on the ensemble's size
    a = E.draw(oracle.philox, 9, 4, 3, 3.0, 0.1, 0.7, zt, Qc, R, sig, 7)
    for other in (E.draw(oracle.philox, 9, 4, 4, 3.0, 0.1, 0.7, zt, Qc, R, sig, 7), E.draw(oracle.philox, 10, 4, 3, 3.0, 0.1, 0.7, zt, Qc, R, sig, 7)):
        assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[2], other[2])
    big = E.draw(oracle.philox, 9, 9, 3, 3.0, 0.1, 0.7, zt, Qc, R, sig, 7)
    assert np.array_equal(big[0][:4], a[0]) and np.array_equal(big[1][:4], a[1]) and np.array_equal(big[2][:4], a[2])
    assert len({tuple(r) for r in big[0]}) == 9


def test_library_exports_and_binds_the_ensemble():
    import slam_amd
    from slam_amd import ekf_ens
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    stable = hdr[:hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")]
    assert sorted(set(re.findall(r"\b(slamgpu_ens_[a-z_0-9]+)\s*\(", stable))) == sorted(ENS_SYMBOLS)
    assert stable.index("int slamgpu_ekf_sync(") < stable.index("typedef struct slamgpu_ekf_ens slamgpu_ekf_ens;")
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr) and re.search(r"#define SLAMGPU_EKF_STATUS_CAPACITY 2\b", stable)
    out = subprocess.run(["nm", "-D", "--defined-only", slam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    for s in ENS_SYMBOLS:
        assert s in slam_amd.DECLARED_SYMBOLS and re.search(r"\bT %s$" % s, out, re.M), s
    doc = stable[stable.index("EKF-SLAM ensemble"):stable.index("typedef struct slamgpu_ekf_ens slamgpu_ekf_ens;")]
    for piece in ("nz and ids are SHARED", "UNCENTRED", "counter (member, step, 5, q)", "DEVIATIONS", "SLAMGPU_EKF_STATUS_CAPACITY", "no atomics"):
        assert piece in doc, piece
    assert callable(slam_amd.EkfEnsemble) and slam_amd.EKF_STATUS_CAPACITY == 2
    for m in ("sim", "sim_noise", "last_inputs", "dims", "poses", "state", "upload", "status", "consistency", "consistency_reset", "sync"):
        assert callable(getattr(slam_amd.EkfEnsemble, m)), m
    # null handles and a bad struct_size are refused; without a GPU the constructor fails loudly
    L = ekf_ens._lib()
    assert L.slamgpu_ens_sync(None) == -1 and L.slamgpu_ens_dims(None, None) == -1 and L.slamgpu_ens_consistency_reset(None) == -1
    cfg = ekf_ens.EkfEnsConfig(C.sizeof(ekf_ens.EkfEnsConfig) - 8, 0, 4, 8, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0, 0)
    h = C.c_void_p()
    assert L.slamgpu_ens_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    for bad in (dict(members=0), dict(members=65536), dict(max_landmarks=513), dict(max_landmarks=-1), dict(wheel_base=0.0)):
        kw = dict(members=4, max_landmarks=8)
        kw.update(bad)
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            slam_amd.EkfEnsemble(**kw)
        assert ei.value.code == -1, bad  # SLAMGPU_ERR_INVALID: judged before the device is looked for
    if slam_amd.device_count() == 0:
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            slam_amd.EkfEnsemble(4, 8)
        assert ei.value.code == -4 and "no CPU fallback" in str(ei.value)  # SLAMGPU_ERR_NO_DEVICE


def test_backend_refuses_what_the_ensemble_cannot_do():
    import slam_amd
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    m = os.path.join(DATA, "example_loop1.mat")

    def run(*args):
        return subprocess.run([exe, "-m", m, *args], capture_output=True, text=True, timeout=60)

    r = run("-method", "EKF1", "-runs", "8")
    assert r.returncode != 0 and "-runs B: with -ekf device" in r.stderr
    r = run("-method", "EKF1", "-ekf", "host", "-runs", "8")
    assert r.returncode != 0 and "-runs B: with -ekf device" in r.stderr
    for method in ("FASTSLAM1", "FASTSLAM2"):
        r = run("-method", method, "-runs", "8")
        assert r.returncode != 0 and "-runs B: with -method EKF1 only" in r.stderr
    r = run("-method", "EKF1", "-ekf", "device", "-runs", "8", "-plot", "tcp://127.0.0.1:1")
    assert r.returncode != 0 and "-runs B: not with -plot" in r.stderr
    for b in ("0", "-3", "65536", "many"):
        r = run("-method", "EKF1", "-ekf", "device", "-runs", b)
        assert r.returncode != 0 and "-runs B: B must be 1 .. 65535" in r.stderr, b
    r = run("-method", "EKF1", "-ekf", "device", "-RUNS_SEED", "5")
    assert r.returncode != 0 and "-RUNS_SEED s: with -runs B" in r.stderr
    assert "-runs B [-RUNS_SEED s]" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    if slam_amd.device_count() == 0:
        r = run("-method", "EKF1", "-ekf", "device", "-runs", "8")
        assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_ensemble_kernels_compile_for_gfx950_with_no_private_segment(tmp_path):
    """ekf_ens.cpp cross-compiled to assembly as the Makefile compiles it: every kernel reports a private segment of 0 bytes (an indexed
    register array the compiler cannot keep in registers would land there)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "slam_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    rule = re.search(r"^\$\(BUILD\)/ekf_ens\.o:.*\n\t\$\(HIPCC\) \$\(COMMON\) (.*) -x hip -c", mk, re.M)
    assert rule and rule.group(1).split() == ["-ffp-contract=on", "-fno-slp-vectorize"]  # as ekf.o
    assert "$(BUILD)/ekf_ens.o" in re.search(r"^HOSTOBJS := (.*)$", mk, re.M).group(1)
    out = str(tmp_path / "ekf_ens.s")
    subprocess.run([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + src, "-I" + os.path.join(ROOT, "include"), *rule.group(1).split(),
                    "-x", "hip", "-S", "--cuda-device-only", "-o", out, os.path.join(src, "ekf_ens.cpp")], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = open(out).read()
    sizes = dict(zip(re.findall(r"\.amdhsa_kernel\s+(\S+)", asm), map(int, re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm))))
    assert any("ekf_ens_kernel" in k for k in sizes) and any("ekf_ens_pose_kernel" in k for k in sizes), sizes
    for kernel, size in sizes.items():
        assert size == 0, (kernel, size)
