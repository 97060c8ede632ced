"""Posterior map summary (slamgpu_map_summary): the entry point is declared, exported and bound, slam-backend offers -map and refuses
what it cannot do with it -- no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA

ROOT = os.path.dirname(DATA)
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")


def test_entry_declared_and_exported():
    import slam_amd
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    assert re.search(r"int slamgpu_map_summary\(slamgpu_ctx \*ctx, int32_t first_slot, int32_t count, double \*out, int32_t \*holders\);", hdr)
    assert re.search(r"#define SLAMGPU_MAP_STRIDE 9\b", hdr)
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # an addition to the stable part: the version stays
    # declared in the stable part, not behind SLAMGPU_EXPERIMENTAL
    assert hdr.index("int slamgpu_map_summary(") < hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")
    L = slam_amd.load_library()
    assert "slamgpu_map_summary" in slam_amd.DECLARED_SYMBOLS and hasattr(L, "slamgpu_map_summary")


def test_capi_binds_it_and_refuses_a_null_context():
    from slam_amd import capi
    L = capi.load_library()
    assert L.slamgpu_map_summary.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    assert capi.MAP_STRIDE == 9 and callable(capi.SlamGpu.map_summary)
    out = np.zeros((4, 9), np.float64)
    hold = np.zeros(4, np.int32)
    assert L.slamgpu_map_summary(None, 0, 4, out.ctypes.data_as(C.c_void_p), hold.ctypes.data_as(C.c_void_p)) < 0
    assert L.slamgpu_last_error()
    assert not out.any() and not hold.any()


def test_no_gpu_no_summary():
    """no CPU fallback: without a GPU there is no context to summarise, and the failure is the loud one of every other entry"""
    import slam_amd
    if slam_amd.device_count() == 0:
        with pytest.raises(slam_amd.SlamGpuError) as e:
            slam_amd.SlamGpu(100, 35).map_summary()
        assert e.value.code == -4 and "no CPU fallback" in str(e.value)
        r = subprocess.run([EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-map", "posterior"], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr and "posterior map:" not in r.stdout


def test_slam_backend_names_the_option_and_refuses_misuse():
    out = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-map best|posterior" in out
    base = [EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-rng", "philox", "-NPARTICLES", "512", "-maxsteps", "10"]
    r = subprocess.run(base + ["-map", "posterior", "-gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-map posterior" in r.stderr and "control steps" not in r.stdout, r.stderr
    r = subprocess.run(base + ["-map", "everything"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-map best|posterior" in r.stderr and "control steps" not in r.stdout, r.stderr
