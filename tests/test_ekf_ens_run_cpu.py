"""The ensemble's K-step run and trace (include/slamgpu.h: slamgpu_ens_run_noise, slamgpu_ens_trace_*), what can be checked without a
GPU: pack_tape and the layout of slamgpu_ens_tape_step against a compiled C program, the symbols, the trace's float64 model, and
slam-backend's refusals of -RUNS_BATCH / -RUNS_TRACE from the arguments alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

f32 = np.float32
RUN_SYMBOLS = ["slamgpu_ens_run_noise", "slamgpu_ens_trace_enable", "slamgpu_ens_trace_info", "slamgpu_ens_trace_fetch"]
FIELDS = ("V", "G", "phi_true", "dt", "truth", "has_truth", "observe", "nz", "first", "step")


def test_pack_tape_and_the_struct_layout(tmp_path):
    import slam_amd
    dt = slam_amd.TAPE_STEP_DTYPE
    assert dt.itemsize == 48
    # the C struct's own offsets, printed by a program compiled against the header
    src = tmp_path / "offsets.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <slamgpu.h>\nint main(void) {\n" +
                   "".join('    printf("%s %%zu\\n", offsetof(slamgpu_ens_tape_step, %s));\n' % (f, f) for f in FIELDS) +
                   '    printf("size %zu\\n", sizeof(slamgpu_ens_tape_step));\n    return 0;\n}\n')
    exe = tmp_path / "offsets"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got.pop("size")) == 48
    assert {k: int(v) for k, v in got.items()} == {f: dt.fields[f][1] for f in FIELDS}
    # three steps by hand: one that observes two landmarks, one that carries observations but does not observe, one that observes one
    z0 = np.array([[10.0, 0.1], [20.0, -0.2]], f32)
    tape = [dict(V=3.0, G=0.1, phi_true=0.5, dt=0.025, step=7, truth=[1.0, 2.0, 0.5], observe=1, z_true=z0, ids=[4, 9]),
            dict(V=2.0, G=0.0, phi_true=0.6, dt=0.025, step=8, truth=None, observe=0, z_true=z0, ids=[4, 9]),
            dict(V=1.0, G=-0.1, phi_true=0.7, dt=0.05, step=9, observe=1, z_true=[[5.0, 1.0]], ids=[2])]
    steps, z_true, ids = slam_amd.pack_tape(tape)
    assert steps.dtype == dt and steps.shape == (3,) and z_true.dtype == f32 and ids.dtype == np.int32
    assert list(steps["nz"]) == [2, 0, 1] and list(steps["first"]) == [0, 2, 2] and list(steps["observe"]) == [1, 0, 1]
    assert list(steps["has_truth"]) == [1, 0, 0] and list(steps["step"]) == [7, 8, 9]
    assert np.array_equal(steps["truth"], np.array([[1, 2, 0.5], [0, 0, 0], [0, 0, 0]], f32))
    assert np.array_equal(steps["V"], np.array([3, 2, 1], f32)) and np.array_equal(steps["dt"], np.array([0.025, 0.025, 0.05], f32))
    assert np.array_equal(z_true, np.array([[10.0, 0.1], [20.0, -0.2], [5.0, 1.0]], f32)) and list(ids) == [4, 9, 2]
    empty = slam_amd.pack_tape([])
    assert empty[0].shape == (0,) and empty[1].shape == (0, 2) and empty[2].shape == (0,)
    with pytest.raises(ValueError):
        slam_amd.pack_tape([dict(V=1, G=0, phi_true=0, dt=0.1, step=0, observe=1, z_true=z0, ids=[1])])


def test_library_declares_exports_and_binds_the_run_and_the_trace():
    import slam_amd
    from slam_amd import ekf_ens
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    # stable: declared outside the #ifdef SLAMGPU_EXPERIMENTAL ... #endif block
    block = hdr[hdr.index("#ifdef SLAMGPU_EXPERIMENTAL"):hdr.index("#endif /* SLAMGPU_EXPERIMENTAL */")]
    out = subprocess.run(["nm", "-D", "--defined-only", slam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    for s in RUN_SYMBOLS:
        assert re.search(r"^int %s\(slamgpu_ekf_ens \*e," % s, hdr, re.M) and s + "(" not in block, s
        assert s in slam_amd.DECLARED_SYMBOLS and re.search(r"\bT %s$" % s, out, re.M), s
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr) and "refused WHOLE" in hdr
    for m in ("run_noise", "trace_enable", "trace_info", "trace_fetch"):
        assert callable(getattr(slam_amd.EkfEnsemble, m)), m
    L = ekf_ens._lib()
    assert L.slamgpu_ens_run_noise(None, None, 0, None, None, 0, None, None, None, None, 0) == -1
    assert L.slamgpu_ens_trace_enable(None, 4) == -1 and L.slamgpu_ens_trace_info(None, None, None, None) == -1
    assert L.slamgpu_ens_trace_fetch(None, 0, 0, None, None) == -1


def test_trace_model_counts_and_sums():
    """the model's records from per-member values, and slam_amd.trace_summary (the figures of a consistency plot) on them"""
    import slam_amd
    import ekf_ens_model as E
    import ekf_ens_run_model as M
    rng = np.random.default_rng(5)
    B, truth = 6, np.array([1.0, -2.0, 0.3], f32)
    xyt = truth.astype(np.float64) + rng.normal(0, 0.05, (B, 3))
    A = rng.normal(0, 0.1, (B, 3, 3))
    Pvv = A @ A.transpose(0, 2, 1) + 0.01 * np.eye(3)
    Pvv[2] = 0.0  # a member that has not moved yet: not counted
    xyt[4, 0] = np.nan  # a non-finite state: not counted
    vals = np.zeros((B, 6))
    E.accumulate(vals, xyt.astype(f32), Pvv.astype(f32), truth)
    rec = M.trace_record(vals)
    assert rec.dtype == np.float64 and rec[0] == 4 and rec[1] == 2 and rec[0] + rec[1] == B
    assert rec[3] == (vals[:, 3] == 1).sum() and 0 <= rec[3] <= rec[0]
    assert rec[2] == vals[:, 2].sum() and rec[2] > 0 and rec[4] == vals[:, 4].sum() and rec[5] == vals[:, 5].sum()
    assert (vals[[2, 4], 2:] == 0).all()  # a member that is not counted adds nothing to the sums
    recs = M.trace_records([vals, np.zeros((B, 6))])
    assert recs.shape == (2, 6) and np.array_equal(recs[0], rec) and not recs[1].any()
    assert M.same_bits(rec, rec.copy()) and not M.same_bits(rec, rec.astype(f32))
    # the product's summary of those records: per step the mean NEES, the share inside, the rms position error and the two counts
    s = slam_amd.trace_summary(recs)
    counted = vals[:, 0] == 1
    assert s.shape == (2, 5) and s.dtype == np.float64 and list(s[0, 3:]) == [4, 2] and list(s[1, 3:]) == [0, 0] and np.isnan(s[1, :3]).all()
    assert s[0, 0] == vals[:, 2].sum() / 4 and s[0, 1] == vals[:, 3].sum() / 4 and s[0, 2] == np.sqrt(vals[:, 4].sum() / 4)
    assert np.isclose(s[0, 0], vals[counted, 2].mean(), rtol=1e-15) and 0 <= s[0, 1] <= 1
    assert slam_amd.trace_summary(np.zeros((0, 6))).shape == (0, 5)


def test_backend_refuses_batch_and_trace_from_the_arguments():
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    m = os.path.join(DATA, "example_loop1.mat")

    def run(*args):
        return subprocess.run([exe, "-m", m, *args], capture_output=True, text=True, timeout=60)

    dev = ("-method", "EKF1", "-ekf", "device", "-runs", "8")
    r = run("-RUNS_BATCH", "4")
    assert r.returncode != 0 and "-RUNS_BATCH K: with -runs B" in r.stderr
    r = run("-method", "EKF1", "-ekf", "device", "-RUNS_BATCH", "4")
    assert r.returncode != 0 and "-RUNS_BATCH K: with -runs B" in r.stderr
    for k in ("0", "4097"):
        r = run(*dev, "-RUNS_BATCH", k)
        assert r.returncode != 0 and "-RUNS_BATCH K: K must be 1 .. 4096" in r.stderr and "no CPU fallback" not in r.stderr, k
    r = run("-RUNS_TRACE", "f")
    assert r.returncode != 0 and "-RUNS_TRACE file: with -runs B" in r.stderr
    assert not os.path.exists("f")
    h = subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    assert "-RUNS_BATCH K [-RUNS_TRACE file]" in h
