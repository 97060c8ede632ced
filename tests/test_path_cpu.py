"""Path posterior (slamgpu_path_*): the entry points are declared, exported and bound; the float64 model the GPU tests use
(tests/path_model.py) agrees with a brute-force enumeration of descendants; slam-backend offers -path and refuses what it cannot do
with it -- no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import path_model
from conftest import DATA

ROOT = os.path.dirname(DATA)
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
f32, f64 = np.float32, np.float64

DECLS = {
    "slamgpu_path_enable": r"int slamgpu_path_enable\(slamgpu_ctx \*ctx, int32_t capacity\);",
    "slamgpu_path_record": r"int slamgpu_path_record\(slamgpu_ctx \*ctx\);",
    "slamgpu_path_info": r"int slamgpu_path_info\(slamgpu_ctx \*ctx, int64_t \*first, int64_t \*next, int32_t \*capacity\);",
    "slamgpu_path_fetch": r"int slamgpu_path_fetch\(slamgpu_ctx \*ctx, int64_t r, float \*xyt, int32_t \*parent\);",
    "slamgpu_path_trace": r"int slamgpu_path_trace\(slamgpu_ctx \*ctx, int32_t particle, int64_t first, int32_t count, float \*xyt, int32_t \*index\);",
    "slamgpu_path_summary": r"int slamgpu_path_summary\(slamgpu_ctx \*ctx, int64_t first, int32_t count, double \*out, int32_t \*distinct\);",
}


def test_entries_declared_and_exported():
    import slam_amd
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    stable = hdr[:hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")]
    L = slam_amd.load_library()
    for name, decl in DECLS.items():
        assert re.search(decl, stable), name  # declared in the stable part, not behind SLAMGPU_EXPERIMENTAL
        assert name in slam_amd.DECLARED_SYMBOLS and hasattr(L, name), name
    assert re.search(r"#define SLAMGPU_PATH_STRIDE 7\b", stable)
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # additions to the stable part: the version stays
    assert L.slamgpu_abi_version() == 3


def test_capi_binds_them_and_refuses_a_null_context():
    from slam_amd import capi
    L = capi.load_library()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.slamgpu_path_enable.argtypes == [vp, i32]
    assert L.slamgpu_path_record.argtypes == [vp]
    assert L.slamgpu_path_info.argtypes == [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    assert L.slamgpu_path_fetch.argtypes == [vp, i64, vp, vp]
    assert L.slamgpu_path_trace.argtypes == [vp, i32, i64, i32, vp, vp]
    assert L.slamgpu_path_summary.argtypes == [vp, i64, i32, vp, vp]
    assert capi.PATH_STRIDE == 7
    for m in ("path_enable", "path_record", "path_info", "path_fetch", "path_trace", "path_summary"):
        assert callable(getattr(capi.SlamGpu, m)), m
    out = np.zeros((4, 7), f64)
    idx = np.zeros(4, np.int32)
    xyt = np.zeros((4, 3), f32)
    a, b, cap = i64(-5), i64(-6), i32(-7)
    p = lambda x: x.ctypes.data_as(vp)
    assert L.slamgpu_path_enable(None, 8) < 0 and L.slamgpu_last_error()
    assert L.slamgpu_path_record(None) < 0
    assert L.slamgpu_path_info(None, C.byref(a), C.byref(b), C.byref(cap)) < 0 and (a.value, b.value, cap.value) == (-5, -6, -7)
    assert L.slamgpu_path_fetch(None, 0, p(xyt), p(idx)) < 0
    assert L.slamgpu_path_trace(None, -1, 0, 4, p(xyt), p(idx)) < 0
    assert L.slamgpu_path_summary(None, 0, 4, p(out), p(idx)) < 0
    assert not out.any() and not idx.any() and not xyt.any()


# ---- the model against brute force ----------------------------------------------------------------------------------------------
def _brute(records, origin, w, logw=False):
    """every present particle's ancestor in every record by walking its own chain; the sums as plain Python loops over the present
    particles (float64; math.fsum: the exactly rounded sum)"""
    import math
    R, N = len(records), len(origin)
    w = np.asarray(w).astype(f64)
    if logw:
        w = np.exp(w - w.max())
    tot = math.fsum(w) if np.isfinite(w).all() else float("nan")
    ok = tot > 0 and math.isfinite(tot)
    anc = np.zeros((R, N), np.int64)
    for i in range(N):
        a = int(origin[i])
        for r in range(R - 1, -1, -1):
            anc[r, i] = a
            a = int(records[r][1][a])
    mean, scatter, cs = np.full((R, 2), np.nan), np.full((R, 3), np.nan), np.full((R, 2), np.nan)
    distinct = np.array([len(set(anc[r].tolist())) for r in range(R)], np.int32)
    for r in range(R if ok else 0):
        pose = np.asarray(records[r][0]).astype(f64)
        x, y, th = pose[anc[r], 0], pose[anc[r], 1], pose[anc[r], 2]
        wh = w / tot
        mx, my = math.fsum(wh * x), math.fsum(wh * y)
        mean[r] = mx, my
        scatter[r] = math.fsum(wh * (x - mx) ** 2), math.fsum(wh * (x - mx) * (y - my)), math.fsum(wh * (y - my) ** 2)
        cs[r] = math.fsum(wh * np.cos(th)), math.fsum(wh * np.sin(th))
    return anc, dict(mean=mean, scatter=scatter, cs=cs, distinct=distinct)


def _genealogy(rng, N, R, resample_every=2, monotone=True):
    recs = []
    for r in range(R):
        pose = np.stack([rng.normal(3.0 * r, 1.0, N), rng.normal(-2.0 * r, 0.5, N), rng.uniform(-np.pi, np.pi, N)], axis=1).astype(f32)
        if r == 0 or r % resample_every:
            parent = np.arange(N, dtype=np.int32)
        else:
            parent = rng.integers(0, N, N).astype(np.int32)
            if monotone:
                parent.sort()
        recs.append((pose, parent))
    return recs


def _agree(recs, origin, w, logw=False):
    anc, b = _brute(recs, origin, w, logw)
    m = path_model.summary(recs, origin, w, logw)
    assert np.array_equal(path_model.lineages(recs, origin), anc)
    assert np.array_equal(m["distinct"], b["distinct"])
    for q in ("mean", "scatter", "cs"):
        assert np.array_equal(np.isnan(m[q]), np.isnan(b[q])), q
        np.testing.assert_allclose(m[q], b[q], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=q)
    for i in (0, len(origin) // 2, len(origin) - 1):
        xyt, idx = path_model.trace(recs, origin, i)
        assert np.array_equal(idx, anc[:, i])
        assert all(np.array_equal(xyt[r], recs[r][0][anc[r, i]]) for r in range(len(recs)))
    return m, b


def test_model_against_brute_force():
    rng = np.random.default_rng(11)
    N, R = 48, 9
    # stratified-like (non-decreasing) parents, identity origin
    recs = _genealogy(rng, N, R)
    w = rng.uniform(0.1, 1.0, N)
    m, _ = _agree(recs, np.arange(N), w)
    assert m["distinct"][-1] == N and m["distinct"][0] < N and np.all(np.diff(m["distinct"]) >= 0)
    # a NON-MONOTONE parent array (nothing in the definitions needs the order stratified resampling happens to give)
    recs = _genealogy(rng, N, R, monotone=False)
    assert any(np.any(np.diff(p) < 0) for _, p in recs)
    _agree(recs, np.arange(N), w)
    # an un-recorded resample folded into origin: the present set descends from a few particles of the newest record
    origin = np.sort(rng.integers(0, N, N)).astype(np.int32)
    m, _ = _agree(recs, origin, w)
    assert m["distinct"][-1] == len(set(origin.tolist())) < N
    # log-weights
    _agree(recs, origin, rng.normal(-700.0, 30.0, N).astype(f32), logw=True)


def test_zero_weight_with_descendants_counts_as_distinct():
    N = 6
    pose = lambda s: np.stack([np.arange(N) * 1.0 + s, np.arange(N) * -2.0, np.linspace(-3, 3, N)], axis=1).astype(f32)
    recs = [(pose(0.0), np.arange(N, dtype=np.int32)), (pose(10.0), np.array([0, 0, 0, 4, 4, 5], np.int32))]
    w = np.array([0.5, 0.25, 0.25, 0.0, 0.0, 0.0])  # particles 3, 4 (ancestor 4) and 5 (ancestor 5) carry no weight
    m, b = _agree(recs, np.arange(N), w)
    assert m["distinct"].tolist() == [3, 6]
    np.testing.assert_allclose(m["mean"][0], recs[0][0][0, :2].astype(f64))  # all of the weight descends from particle 0
    np.testing.assert_allclose(m["scatter"][0], 0.0, atol=1e-15)


@pytest.mark.parametrize("w", [np.zeros(5), np.array([1.0, np.inf, 1.0, 1.0, 1.0]), np.array([1.0, 1.0, np.nan, 1.0, 1.0])])
def test_degenerate_weights(w):
    rng = np.random.default_rng(3)
    recs = _genealogy(rng, 5, 4)
    m, b = _agree(recs, np.arange(5), w)
    assert all(np.isnan(m[q]).all() for q in ("mean", "scatter", "cs")) and np.all(m["distinct"] >= 1)


# ---- slam-backend ----------------------------------------------------------------------------------------------------------------
BASE = [EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-rng", "philox", "-NPARTICLES", "512", "-maxsteps", "10"]


def test_slam_backend_names_the_option():
    out = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-path none|smoothed" in out and "-PATH_RECORDS" in out


@pytest.mark.parametrize("extra", [("-method", "EKFSLAM"), ("-method", "FASTSLAM2", "-gpus", "2"),
                                   ("-method", "FASTSLAM2", "-assoc", "particle", "-observe", "device")],
                         ids=["ekf", "gpus2", "particle_device"])
def test_slam_backend_refuses_misuse(extra):
    """decided from the arguments alone, before a context is created: holds without a GPU"""
    r = subprocess.run(BASE + list(extra) + ["-path", "smoothed"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-path smoothed" in r.stderr and "control steps" not in r.stdout and "no CPU fallback" not in r.stderr, r.stderr


def test_slam_backend_refuses_unknown_values():
    r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-path", "everything"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-path none|smoothed" in r.stderr and "control steps" not in r.stdout, r.stderr
    r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-path", "smoothed", "-PATH_RECORDS", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-path smoothed" in r.stderr and "-PATH_RECORDS" in r.stderr, r.stderr


def test_no_gpu_no_path():
    """no CPU fallback: without a GPU there is no context to record, and the failure is the loud one of every other entry"""
    import slam_amd
    if slam_amd.device_count() == 0:
        with pytest.raises(slam_amd.SlamGpuError) as e:
            slam_amd.SlamGpu(100, 35).path_enable(8)
        assert e.value.code == -4 and "no CPU fallback" in str(e.value)
        r = subprocess.run(BASE + ["-method", "FASTSLAM2", "-path", "smoothed"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr and "smoothed path:" not in r.stdout
