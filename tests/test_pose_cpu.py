"""Pose posterior (slamgpu_pose_summary, slamgpu_pose_history_*, slamhost_pose_nees): the entry points are declared, exported and
bound; the float64 model the GPU tests use (tests/pose_model.py) knows the answers of sets built by hand; slamhost_pose_nees agrees
with the model's NEES; slam-backend offers -pose and refuses what it cannot do with it -- no GPU needed for any of it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pose_model
from conftest import DATA

ROOT = os.path.dirname(DATA)
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
f32, f64 = np.float32, np.float64

DECLS = {
    "slamgpu_pose_summary": r"int slamgpu_pose_summary\(slamgpu_ctx \*ctx, double out\[SLAMGPU_POSE_STRIDE\]\);",
    "slamgpu_pose_history_enable": r"int slamgpu_pose_history_enable\(slamgpu_ctx \*ctx, int32_t capacity\);",
    "slamgpu_pose_history_record": r"int slamgpu_pose_history_record\(slamgpu_ctx \*ctx\);",
    "slamgpu_pose_history_info": r"int slamgpu_pose_history_info\(slamgpu_ctx \*ctx, int64_t \*first, int64_t \*next, int32_t \*capacity\);",
    "slamgpu_pose_history_fetch": r"int slamgpu_pose_history_fetch\(slamgpu_ctx \*ctx, int64_t first, int32_t count, double \*out\);",
}


def test_entries_declared_and_exported():
    import slam_amd
    from slam_amd import host
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    stable = hdr[:hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")]
    L = slam_amd.load_library()
    for name, decl in DECLS.items():
        assert re.search(decl, stable), name  # declared in the stable part, not behind SLAMGPU_EXPERIMENTAL
        assert name in slam_amd.DECLARED_SYMBOLS and hasattr(L, name), name
    assert re.search(r"#define SLAMGPU_POSE_STRIDE 18\b", stable)
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # additions to the stable part: the version stays
    assert L.slamgpu_abi_version() == 3
    # the header says when the heading moments mean something
    doc = stable[stable.index("pose posterior: weighted mean"):stable.index("int slamgpu_pose_summary")]
    assert "spans less than pi" in doc and "[4..5]" in doc
    hh = open(os.path.join(ROOT, "include", "slamhost.h")).read()
    assert re.search(r"int32_t slamhost_pose_nees\(const double \*summary, int32_t count, const float \*xtrue", hh)
    assert "slamhost_pose_nees" in host.DECLARED_SYMBOLS and hasattr(host.load_library(), "slamhost_pose_nees")


def test_capi_binds_them_and_refuses_a_null_context():
    from slam_amd import capi, host
    L = capi.load_library()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.slamgpu_pose_summary.argtypes == [vp, vp]
    assert L.slamgpu_pose_history_enable.argtypes == [vp, i32]
    assert L.slamgpu_pose_history_record.argtypes == [vp]
    assert L.slamgpu_pose_history_info.argtypes == [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    assert L.slamgpu_pose_history_fetch.argtypes == [vp, i64, i32, vp]
    assert capi.POSE_STRIDE == 18 == host.POSE_STRIDE == pose_model.STRIDE
    for m in ("pose_summary", "pose_history_enable", "pose_history_record", "pose_history_info", "pose_history_fetch"):
        assert callable(getattr(capi.SlamGpu, m)), m
    assert callable(host.pose_nees)
    out = np.zeros((4, 18), f64)
    a, b, cap = i64(-5), i64(-6), i32(-7)
    p = lambda x: x.ctypes.data_as(vp)
    assert L.slamgpu_pose_summary(None, p(out)) < 0 and L.slamgpu_last_error()
    assert L.slamgpu_pose_history_enable(None, 8) < 0
    assert L.slamgpu_pose_history_record(None) < 0
    assert L.slamgpu_pose_history_info(None, C.byref(a), C.byref(b), C.byref(cap)) < 0 and (a.value, b.value, cap.value) == (-5, -6, -7)
    assert L.slamgpu_pose_history_fetch(None, 0, 4, p(out)) < 0
    assert not out.any()


def test_model_knows_its_answers():
    assert pose_model.self_check()


def test_model_against_plain_numpy():
    """the fsum model against numpy's own sums on a random set (uneven weights with zeros, non-zero Pv), linear and log-weights, and
    through a pending gather"""
    rng = np.random.default_rng(5)
    N = 300
    xv = np.stack([rng.normal(40.0, 0.5, N), rng.normal(-7.0, 0.3, N), rng.normal(3.1, 0.05, N)], axis=1).astype(f32)  # headings across pi
    A = rng.normal(0.0, 0.1, (N, 3, 3))
    Pv = (A @ A.transpose(0, 2, 1)).astype(f32)
    w = rng.uniform(0.0, 1.0, N).astype(f32)
    w[::7] = 0.0
    for logw, ww in ((False, w), (True, rng.normal(-500.0, 3.0, N).astype(f32))):
        o = pose_model.summary(xv, Pv, ww, logw)
        wd = ww.astype(f64)
        wh = np.exp(wd - wd.max()) if logw else wd
        wh = wh / wh.sum()
        th = xv[:, 2].astype(f64)
        u = np.arctan2(np.sin(th - th[0]), np.cos(th - th[0]))
        m = np.array([wh @ xv[:, 0], wh @ xv[:, 1], wh @ u])
        d = np.stack([xv[:, 0] - m[0], xv[:, 1] - m[1], u - m[2]], axis=1)
        S = np.einsum("i,ij,ik->jk", wh, d, d)
        assert abs(o[0] - wh @ wh) < 1e-15
        np.testing.assert_allclose(o[1:4], [m[0], m[1], th[0] + m[2]], rtol=0, atol=1e-11)
        np.testing.assert_allclose(o[6:12], [S[0, 0], S[0, 1], S[1, 1], S[0, 2], S[1, 2], S[2, 2]], rtol=0, atol=1e-12)
        np.testing.assert_allclose(pose_model.covariance(o), S + np.einsum("i,ijk->jk", wh, Pv.astype(f64)), rtol=0, atol=1e-12)
        assert o[11] < 0.01, "the heading scatter of a 0.05 rad cloud across pi"
        b = pose_model.bounds(xv, Pv, o)
        assert np.all(b > 0) and np.all(b[6:9] < 1e-9)
    keep = np.sort(rng.integers(0, N, N))
    a, b, c = pose_model.present_set(xv, Pv, w, keep)
    o = pose_model.summary(a, b, c)
    assert abs(o[0] - 1.0 / N) < 1e-9 and abs(o[1] - xv[keep, 0].astype(f64).mean()) < 1e-11


def _summary(mean, P, pv_share=0.5):
    s = np.zeros(18, f64)
    s[1:4] = mean
    tri = np.array([P[0][0], P[1][0], P[1][1], P[2][0], P[2][1], P[2][2]], f64)
    s[6:12] = (1.0 - pv_share) * tri
    s[12:18] = pv_share * tri
    s[0] = 0.01
    return s


def test_pose_nees_against_the_model():
    from slam_amd import host
    # a diagonal P with a known e: NEES = sum (e_i / sigma_i)^2
    s0 = _summary([1.0, 2.0, 0.5], np.diag([0.04, 0.16, 0.01]))
    t0 = np.array([0.8, 2.4, 0.4], f32)
    # a heading error across +-pi
    s1 = _summary([1.0, 2.0, math.pi - 0.05], np.diag([0.04, 0.16, 0.01]))
    t1 = np.array([1.0, 2.0, -math.pi + 0.05], f32)
    # a full P
    A = np.array([[0.3, 0.0, 0.0], [0.1, 0.2, 0.0], [-0.05, 0.02, 0.1]])
    s2 = _summary([-3.0, 7.0, -2.0], A @ A.T, pv_share=0.25)
    t2 = np.array([-3.2, 7.1, -1.9], f32)
    # N = 1 (no scatter, no Pv: P = 0), a P that is not positive definite, and a NaN summary
    s3 = _summary([0.0, 0.0, 0.0], np.zeros((3, 3)))
    s4 = _summary([0.0, 0.0, 0.0], np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    s5 = np.full(18, np.nan)
    S = np.stack([s0, s1, s2, s3, s4, s5])
    T = np.stack([t0, t1, t2, np.zeros(3, f32), np.zeros(3, f32), np.zeros(3, f32)])
    v, e, bad = host.pose_nees(S, T)
    mv, me, mbad = pose_model.nees(S, T)
    print("pose_nees:", v, "model:", mv)
    assert bad == mbad == 3 and np.array_equal(np.isnan(v), [False, False, False, True, True, True]) and np.array_equal(np.isnan(v), np.isnan(mv))
    np.testing.assert_allclose(v[:3], mv[:3], rtol=1e-12)
    np.testing.assert_allclose(e[:5], me[:5], rtol=0, atol=1e-15)
    assert abs(v[0] - 3.0) < 1e-5 and abs(e[1, 2] + 0.1) < 1e-6 and abs(v[1] - 1.0) < 1e-4
    # err may be NULL, count 0 does nothing, bad arguments are -1
    L = host.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n2 = np.zeros(6, f64)
    assert L.slamhost_pose_nees(p(S), 6, p(T), p(n2), None) == 3 and np.array_equal(n2, v, equal_nan=True)
    assert L.slamhost_pose_nees(None, 0, None, None, None) == 0
    assert L.slamhost_pose_nees(p(S), -1, p(T), p(n2), None) == -1 and L.slamhost_pose_nees(p(S), 2, p(T), None, None) == -1


# ---- slam-backend ----------------------------------------------------------------------------------------------------------------
BASE = [EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-rng", "philox", "-NPARTICLES", "512", "-maxsteps", "10"]


def test_slam_backend_names_the_option():
    out = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-pose none|posterior" in out and "-POSE_RECORDS" in out and "7.8147" in out


@pytest.mark.parametrize("extra", [("-method", "EKFSLAM"), ("-method", "FASTSLAM2", "-gpus", "2")], ids=["ekf", "gpus2"])
def test_slam_backend_refuses_misuse(extra):
    """decided from the arguments alone, before a context is created: holds without a GPU"""
    r = subprocess.run(BASE + list(extra) + ["-pose", "posterior"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-pose posterior" in r.stderr and "control steps" not in r.stdout and "no CPU fallback" not in r.stderr, r.stderr


def test_slam_backend_refuses_unknown_values():
    r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-pose", "everything"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-pose none|posterior" in r.stderr and "control steps" not in r.stdout, r.stderr
    r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-pose", "posterior", "-POSE_RECORDS", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-pose posterior" in r.stderr and "-POSE_RECORDS" in r.stderr, r.stderr


def test_no_gpu_no_pose_posterior():
    """no CPU fallback: without a GPU there is no context to summarise, and the failure is the loud one of every other entry"""
    import slam_amd
    if slam_amd.device_count() == 0:
        for call in (lambda s: s.pose_summary(), lambda s: s.pose_history_enable(8)):
            with pytest.raises(slam_amd.SlamGpuError) as e:
                call(slam_amd.SlamGpu(100, 35))
            assert e.value.code == -4 and "no CPU fallback" in str(e.value)
        r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-pose", "posterior"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr and "pose posterior:" not in r.stdout
