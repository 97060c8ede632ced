"""Innovation posterior (slamgpu_innovation_summary, slamgpu_innovation_*, slamhost_innovation_nis): the entry points are declared in
both headers, exported and bound; the float64 model the GPU tests use (tests/innovation_model.py) knows the answers of sets built by
hand; slamhost_innovation_nis agrees with the model's NIS, error returns included; slam-backend offers -innovation and refuses what it
cannot do with it -- no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import innovation_model
from conftest import DATA

ROOT = os.path.dirname(DATA)
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
f32, f64 = np.float32, np.float64

DECLS = {
    "slamgpu_innovation_summary": r"int slamgpu_innovation_summary\(slamgpu_ctx \*ctx, const float \*zf, const int32_t \*idf, int32_t m, const float R\[4\],\s*"
                                  r"double \*out /\* \[m\]\[SLAMGPU_INNOV_STRIDE\] \*/, int32_t \*holders /\* \[m\], may be NULL \*/\);",
    "slamgpu_innovation_history_enable": r"int slamgpu_innovation_history_enable\(slamgpu_ctx \*ctx, int32_t capacity\);",
    "slamgpu_innovation_record": r"int slamgpu_innovation_record\(slamgpu_ctx \*ctx, const float \*zf, const int32_t \*idf, int32_t m, const float R\[4\]\);",
    "slamgpu_innovation_history_info": r"int slamgpu_innovation_history_info\(slamgpu_ctx \*ctx, int64_t \*first, int64_t \*next, int32_t \*capacity, int64_t \*records\);",
    "slamgpu_innovation_history_fetch": r"int slamgpu_innovation_history_fetch\(slamgpu_ctx \*ctx, int64_t first, int32_t count, double \*out, int32_t \*record, "
                                        r"int32_t \*slot\);",
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
    assert re.search(r"#define SLAMGPU_INNOV_STRIDE 10\b", stable)
    assert stable.index("int slamgpu_pose_history_fetch") < stable.index("int slamgpu_innovation_summary"), "next to the pose posterior"
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # additions to the stable part: the version stays
    assert L.slamgpu_abi_version() == 3
    # the header states the formula and its order, and says which entry points are not recorded
    doc = stable[stable.index("innovation posterior: per-observation moments"):stable.index("int slamgpu_innovation_history_enable")]
    for piece in ("d2 = dx dx + dy dy", "IEEE remainder(z_b - (atan2(dy, dx) - theta), 2 pi)", "R[1] is not read", "slamgpu_run_particle are NOT recorded"):
        assert piece in doc, piece
    hh = open(os.path.join(ROOT, "include", "slamhost.h")).read()
    assert re.search(r"int32_t slamhost_innovation_nis\(const double \*entries, int32_t count, double \*nis\);", hh)
    assert "slamhost_innovation_nis" in host.DECLARED_SYMBOLS and hasattr(host.load_library(), "slamhost_innovation_nis")


def test_capi_binds_them_and_refuses_a_null_context():
    from slam_amd import capi, host
    L = capi.load_library()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.slamgpu_innovation_summary.argtypes == [vp, vp, vp, i32, vp, vp, vp]
    assert L.slamgpu_innovation_history_enable.argtypes == [vp, i32]
    assert L.slamgpu_innovation_record.argtypes == [vp, vp, vp, i32, vp]
    assert L.slamgpu_innovation_history_info.argtypes == [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]
    assert L.slamgpu_innovation_history_fetch.argtypes == [vp, i64, i32, vp, vp, vp]
    assert capi.INNOV_STRIDE == 10 == host.INNOV_STRIDE == innovation_model.STRIDE
    for m in ("innovation_summary", "innovation_history_enable", "innovation_record", "innovation_history_info", "innovation_history_fetch"):
        assert callable(getattr(capi.SlamGpu, m)), m
    assert callable(host.innovation_nis)
    out = np.zeros((4, 10), f64)
    zf, idf, R = np.ones((4, 2), f32), np.zeros(4, np.int32), np.array([0.01, 0, 0, 0.0004], f32)
    a, b, cap, rec = i64(-5), i64(-6), i32(-7), i64(-8)
    p = lambda x: x.ctypes.data_as(vp)
    assert L.slamgpu_innovation_summary(None, p(zf), p(idf), 4, p(R), p(out), None) < 0 and L.slamgpu_last_error()
    assert L.slamgpu_innovation_history_enable(None, 8) < 0
    assert L.slamgpu_innovation_record(None, p(zf), p(idf), 4, p(R)) < 0
    assert L.slamgpu_innovation_history_info(None, C.byref(a), C.byref(b), C.byref(cap), C.byref(rec)) < 0
    assert (a.value, b.value, cap.value, rec.value) == (-5, -6, -7, -8)
    assert L.slamgpu_innovation_history_fetch(None, 0, 4, p(out), None, None) < 0
    assert not out.any()


def test_model_knows_its_answers():
    assert innovation_model.self_check()
    assert set(innovation_model.known_sets()) >= {"symmetric", "ahead_behind", "half", "one", "zero_weights", "inf_weight"}


def test_model_against_plain_numpy():
    """the fsum model against numpy's own vectorised evaluation on a random set (uneven weights with zeros, a slot only some hold),
    linear and log-weights; its bounds are positive and small"""
    rng = np.random.default_rng(9)
    N, nf = 200, 3
    xv = np.stack([rng.normal(3.0, 0.3, N), rng.normal(-2.0, 0.3, N), rng.normal(0.4, 0.05, N)], axis=1).astype(f32)
    lm = np.array([[20.0, 5.0], [-15.0, -1.0], [4.0, 12.0]])
    xf = (lm[None] + rng.normal(0.0, 0.2, (N, nf, 2))).astype(f32)
    A = rng.normal(0.0, 0.15, (N, nf, 2, 2))
    Pf = (A @ A.transpose(0, 1, 3, 2)).astype(f32)
    xf[::3, 2] = np.nan
    Pf[::3, 2] = np.nan
    R = np.array([0.01, 0.0, 0.0, 0.0004], f32)
    idf = np.array([2, 0, 1, 0], np.int32)
    zf = np.array([[12.5, 1.2], [17.5, -0.05], [18.0, 2.7], [17.0, 0.0]], f32)
    w = rng.uniform(0.0, 1.0, N).astype(f32)
    w[::7] = 0.0
    for logw, ww in ((False, w), (True, rng.normal(-500.0, 2.0, N).astype(f32))):
        out, holders, terms = innovation_model.summary(xv, ww, xf, Pf, zf, idf, R, logw)
        wd = ww.astype(f64)
        wh = np.exp(wd - wd.max()) if logw else wd
        wh = wh / wh.sum()
        for q, l in enumerate(idf):
            held = ~np.isnan(xf[:, l, 0])
            assert holders[q] == held.sum()
            x = xv[held].astype(f64)
            f = xf[held, l].astype(f64)
            P = Pf[held, l].astype(f64)
            ww_ = wh[held]
            dx, dy = f[:, 0] - x[:, 0], f[:, 1] - x[:, 1]
            d2 = dx * dx + dy * dy
            d = np.sqrt(d2)
            v = np.stack([zf[q, 0] - d, np.remainder(zf[q, 1] - (np.arctan2(dy, dx) - x[:, 2]) + np.pi, 2 * np.pi) - np.pi], axis=1)
            H = np.stack([np.stack([dx / d, dy / d], 1), np.stack([-dy / d2, dx / d2], 1)], 1)
            S = H @ P @ H.transpose(0, 2, 1) + np.array([[R[0], R[2]], [R[2], R[3]]], f64)
            nis = np.einsum("ij,ijk,ik->i", v, np.linalg.inv(S), v)
            s = ww_.sum()
            mean = ww_ @ v / s
            dv = v - mean
            exp = [s, mean[0], mean[1], ww_ @ (dv[:, 0] ** 2) / s, ww_ @ (dv[:, 0] * dv[:, 1]) / s, ww_ @ (dv[:, 1] ** 2) / s,
                   ww_ @ S[:, 0, 0] / s, ww_ @ S[:, 1, 0] / s, ww_ @ S[:, 1, 1] / s, ww_ @ nis / s]
            np.testing.assert_allclose(out[q], exp, rtol=1e-9, atol=1e-12)
        assert np.all(out[:, 0] > 0) and out[0, 0] < 0.8 and abs(out[1, 0] - 1.0) < 1e-12
        assert out[1].tobytes() != out[3].tobytes() and np.array_equal(out[1, 6:9], out[3, 6:9])  # the same slot twice: the same S, another v
        b = innovation_model.bounds(terms, N, out)
        assert np.all(b > 0) and np.all(b[:, :9] < 1e-9) and np.all(b[:, 9] < 1e-6), b.max(0)
        mix, bad = innovation_model.nis(out)
        assert bad == 0 and np.all(mix >= 0) and np.all(mix <= out[:, 9] * (1 + 1e-9)), "the mixture's covariance is no smaller than a particle's"


def test_innovation_nis_against_the_model():
    from slam_amd import host
    good = [1.0, 0.3, -0.2, 0.01, 0.0, 0.02, 0.09, 0.0, 0.03, 2.0]   # P = diag(0.1, 0.05): NIS = 0.09 / 0.1 + 0.04 / 0.05 = 1.7
    full = [0.6, -0.1, 0.05, 0.02, 0.004, 0.001, 0.05, -0.006, 0.002, 3.0]
    nobody = [0.0] + [np.nan] * 9
    notpd = [1.0, 0.3, -0.2, 0.01, 0.5, 0.02, 0.09, 0.0, 0.03, 2.0]
    nan = list(good)
    nan[9] = np.nan
    zero_share = list(good)
    zero_share[0] = 0.0
    E = np.array([good, full, nobody, notpd, nan, zero_share], f64)
    v, bad = host.innovation_nis(E)
    mv, mbad = innovation_model.nis(E)
    print("innovation_nis:", v, "model:", mv)
    assert bad == mbad == 4 and np.array_equal(np.isnan(v), [False, False, True, True, True, True]) and np.array_equal(np.isnan(v), np.isnan(mv))
    np.testing.assert_allclose(v[:2], mv[:2], rtol=1e-13)
    assert abs(v[0] - 1.7) < 1e-14
    P = np.array([[0.07, -0.002], [-0.002, 0.003]])
    e = np.array([-0.1, 0.05])
    assert abs(v[1] - e @ np.linalg.inv(P) @ e) < 1e-12
    # one entry as [10], count 0 does nothing, bad arguments are -1
    assert host.innovation_nis(np.array(good))[0].shape == (1,)
    L = host.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n2 = np.zeros(6, f64)
    assert L.slamhost_innovation_nis(None, 0, None) == 0
    assert L.slamhost_innovation_nis(p(E), -1, p(n2)) == -1 and L.slamhost_innovation_nis(p(E), 2, None) == -1 and L.slamhost_innovation_nis(None, 2, p(n2)) == -1
    assert not n2.any()


# ---- slam-backend ----------------------------------------------------------------------------------------------------------------
BASE = [EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-rng", "philox", "-NPARTICLES", "512", "-maxsteps", "10"]


def test_slam_backend_names_the_option():
    out = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-innovation none|posterior" in out and "-INNOVATION_RECORDS" in out and "5.9915" in out and "65536" in out


@pytest.mark.parametrize("extra,why", [(("-method", "EKFSLAM"), "FastSLAM only"), (("-method", "FASTSLAM2", "-gpus", "2"), "single GPU only"),
                                       (("-method", "FASTSLAM2", "-observe", "device"), "-observe device"),
                                       (("-method", "FASTSLAM2", "-assoc", "particle"), "-assoc particle"),
                                       (("-method", "FASTSLAM2", "-INNOVATION_RECORDS", "0"), "-INNOVATION_RECORDS"),
                                       (("-method", "FASTSLAM2", "-INNOVATION_RECORDS", "-4"), "-INNOVATION_RECORDS")],
                         ids=["ekf", "gpus2", "observe_device", "assoc_particle", "records0", "records_negative"])
def test_slam_backend_refuses_misuse(extra, why):
    """decided from the arguments alone, before a context is created: holds without a GPU, and nothing runs"""
    r = subprocess.run(BASE + list(extra) + ["-innovation", "posterior"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-innovation posterior" in r.stderr and why in r.stderr, r.stderr
    assert r.stdout == "" and "no CPU fallback" not in r.stderr, r.stdout


def test_slam_backend_refuses_unknown_values():
    r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-innovation", "everything"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-innovation none|posterior" in r.stderr and r.stdout == "", r.stderr
    r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-INNOVATION_RECORDS", "100"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-INNOVATION_RECORDS n: with -innovation posterior" in r.stderr and r.stdout == "", r.stderr


def test_no_gpu_no_innovation_posterior():
    """no CPU fallback: without a GPU there is no context to summarise, and the failure is the loud one of every other entry"""
    import slam_amd
    if slam_amd.device_count() == 0:
        for call in (lambda s: s.innovation_summary(np.ones((1, 2), f32), [0], [0.01, 0, 0, 0.0004]), lambda s: s.innovation_history_enable(8)):
            with pytest.raises(slam_amd.SlamGpuError) as e:
                call(slam_amd.SlamGpu(100, 35))
            assert e.value.code == -4 and "no CPU fallback" in str(e.value)
        r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-innovation", "posterior"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr and "innovation posterior:" not in r.stdout
