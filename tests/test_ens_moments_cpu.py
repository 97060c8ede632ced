"""slamgpu_ens_moments (include/slamgpu.h), what can be checked without a GPU: the symbol and its binding, the float64 model the GPU
tests measure against (tests/ens_moments_model.py) on a set worked by hand, moments_summary on a case with known ratios, and
slam-backend's refusals."""
import math
import os
import re
import subprocess

import numpy as np

from conftest import DATA, ROOT

f32 = np.float32


def test_symbol_is_declared_stable_exported_and_bound():
    import slam_amd
    from slam_amd import ekf_ens
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    after = hdr[hdr.index("#endif /* SLAMGPU_EXPERIMENTAL */"):]
    assert re.search(r"\bint slamgpu_ens_moments\s*\(slamgpu_ekf_ens \*e, int32_t D, uint32_t exclude_status,", after)
    assert "slamgpu_ens_moments" not in hdr[hdr.index("#ifdef SLAMGPU_EXPERIMENTAL"):hdr.index("#endif /* SLAMGPU_EXPERIMENTAL */")]
    for piece in ("POPULATION form", "n / (n - 1)", "EACH MEMBER'S OWN", "no atomics", "SLAMGPU_ENS_MOMENTS_CHUNK", "n = 1: C is exactly 0", "only grows"):
        assert piece in after, piece
    out = subprocess.run(["nm", "-D", "--defined-only", slam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT slamgpu_ens_moments$", out, re.M) and "slamgpu_ens_moments" in slam_amd.DECLARED_SYMBOLS
    assert callable(slam_amd.EkfEnsemble.moments) and callable(slam_amd.moments_summary) and slam_amd.moments_summary is ekf_ens.moments_summary
    # a null handle is refused before anything else is looked at, and the outputs are untouched
    L = ekf_ens._lib()
    mean = np.full(3, 7.0)
    assert L.slamgpu_ens_moments(None, 3, 0, mean.ctypes.data, None, None, None, None, None) == -1
    assert (mean == 7.0).all() and b"null EKF ensemble handle" in L.slamgpu_last_error()


def test_model_on_a_set_worked_by_hand():
    """three members, D = 5, member 1 excluded (a NaN in its state), headings 3 and -3.125 across +-pi.  With n = 2 and the pivot member 0:
    v_2 = (2, -2, u, 4, 0), u = 2 pi - 6.125; delta = v_2 / 2; C = v_2 v_2^T / 2 - v_2 v_2^T / 4 = v_2 v_2^T / 4"""
    import ens_moments_model as M
    x = np.array([[1, 2, 3.0, 4, 5], [9, 9, np.nan, 9, 9], [3, 0, -3.125, 8, 5]], f32)
    P = np.zeros((3, 5, 5), f32)
    P[0], P[1], P[2] = np.diag([1, 2, 3, 4, 5]), 100.0, np.diag([3, 2, 1, 0, 5]) + 0.5
    m = M.moments(x, P, [5, 5, 5], [0, 0, 0], 5)
    assert (m["counted"], m["left_out"], m["pivot"]) == (2, 1, 0)
    u = 2 * math.pi - 6.125
    v = np.array([2, -2, u, 4, 0])
    assert np.allclose(m["mean"], [2, 1, 3 + u / 2, 6, 5], rtol=0, atol=1e-15) and 3 < m["mean"][2] < math.pi
    assert np.allclose(m["C"], np.outer(v, v) / 4, rtol=0, atol=1e-15) and (m["C"] == m["C"].T).all()
    assert m["C"][0, 0] == 1 and m["C"][3, 0] == 2 and m["C"][1, 0] == -1 and (m["C"][4] == 0).all()
    assert (m["Pbar"] == (np.diag([2, 2, 2, 2, 5]) + 0.25)).all()  # (P_0 + P_2) / 2: member 1's hundreds are not in it
    # the heading is taken the short way round: -3.125 is 0.158 rad AHEAD of 3, not 6.125 behind
    assert abs(m["v"][1, 2] - u) < 1e-15 and m["v"][1, 2] > 0
    # the status word excludes; dim < D excludes; everyone excluded: NaN and (0, B, -1); n = 1: C == 0
    m = M.moments(x, P, [5, 5, 5], [2, 0, 0], 5, exclude=2)
    assert (m["counted"], m["left_out"], m["pivot"]) == (1, 2, 2) and (m["C"] == 0).all() and (m["mean"] == x[2].astype(np.float64)).all()
    m = M.moments(x, P, [3, 5, 3], [0, 0, 0], 5)
    assert (m["counted"], m["left_out"], m["pivot"]) == (0, 3, -1) and np.isnan(m["mean"]).all() and np.isnan(m["C"]).all() and np.isnan(m["Pbar"]).all()
    Pd = P.copy()
    Pd[0, 4, 4] = np.inf  # a non-finite diagonal entry of P inside [0, D) excludes; outside it does not
    assert M.moments(x, Pd, [5, 5, 5], [0, 0, 0], 5)["pivot"] == 2 and M.moments(x, Pd, [5, 5, 5], [0, 0, 0], 3)["pivot"] == 0
    # tiles: 600 members are three tiles; on dyadic data the tiled sums are the plain ones exactly
    rng = np.random.default_rng(1)
    xb = (rng.integers(-64, 64, (600, 5)) / 64.0).astype(f32)
    Pb = (rng.integers(-64, 64, (600, 5, 5)) / 64.0).astype(f32)
    m = M.moments(xb, Pb, np.full(600, 5), np.zeros(600, int), 5)
    d = xb.astype(np.float64) - xb[0].astype(np.float64)
    assert (m["Pbar"] == np.tril(Pb.astype(np.float64).sum(0) / 600) + np.tril(Pb.astype(np.float64).sum(0) / 600, -1).T).all()
    assert np.allclose(m["C"], np.cov(d.T, bias=True), rtol=0, atol=1e-12) and np.allclose(m["mean"], xb.astype(np.float64).mean(0), rtol=0, atol=1e-12)


def test_moments_summary_on_known_ratios():
    import slam_amd
    C = np.diag([2.0, 4.0, 0.5, 1.0, 3.0, 9.0, 1.0])
    Pb = np.diag([1.0, 2.0, 2.0, 2.0, 2.0, 1.0, 1.0])
    C[0, 1] = C[1, 0] = 0.5 * math.sqrt(8.0)  # correlation 0.5
    Pb[3, 6] = Pb[6, 3] = -0.25 * math.sqrt(2.0)  # correlation -0.25
    mean = np.array([1.0, 2.0, math.pi - 0.01, 10.0, 0.0, 0.0, 5.0])
    s = slam_amd.moments_summary(mean, C, Pb, truth_pose=[4.0, 6.0, -math.pi + 0.01], truth_landmarks=[[10.0, 3.0], [0.0, 1.0]])
    assert s["pos_ratio"] == 2.0 and s["heading_ratio"] == 0.25
    assert (s["feature_ratio_mean"], s["feature_ratio_min"], s["feature_ratio_max"]) == (3.0, 1.0, 5.0)
    assert abs(s["max_corr_C"] - 0.5) < 1e-15 and abs(s["max_corr_Pbar"] - 0.25) < 1e-15
    assert s["bias_pos"] == 5.0 and abs(s["bias_heading"] + 0.02) < 1e-12 and s["bias_landmarks"] == 3.5
    s = slam_amd.moments_summary(mean[:3], C[:3, :3], Pb[:3, :3])  # the pose alone: no features, no truths
    assert s["pos_ratio"] == 2.0 and math.isnan(s["feature_ratio_mean"]) and "bias_pos" not in s and "bias_landmarks" not in s
    assert math.isnan(slam_amd.moments_summary(mean[:3], np.zeros((3, 3)), Pb[:3, :3])["max_corr_C"])


def test_backend_refuses_the_moments_without_runs():
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    m = os.path.join(DATA, "example_loop1.mat")

    def run(*args):
        return subprocess.run([exe, "-m", m, *args], capture_output=True, text=True, timeout=60)

    r = run("-method", "EKF1", "-ekf", "device", "-RUNS_MOMENTS", "1")
    assert r.returncode != 0 and "-RUNS_MOMENTS 1: with -runs B" in r.stderr
    r = run("-method", "EKF1", "-ekf", "device", "-RUNS_MOMENTS_OUT", "x.txt")
    assert r.returncode != 0 and "-RUNS_MOMENTS_OUT file: with -runs B -RUNS_MOMENTS 1" in r.stderr
    r = run("-method", "EKF1", "-ekf", "device", "-runs", "8", "-RUNS_MOMENTS_OUT", "x.txt")
    assert r.returncode != 0 and "-RUNS_MOMENTS_OUT file: with -runs B -RUNS_MOMENTS 1" in r.stderr
    assert "-RUNS_MOMENTS 1 [-RUNS_MOMENTS_OUT file]" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
