"""Data association sampling (slamgpu_set_particle_assoc_sampling / slamgpu_particle_sample_stats / slamgpu_particle_labels): the entry
points are declared, exported and bound, and slam-backend offers the option -- no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import DATA

ROOT = os.path.dirname(DATA)
ENTRIES = ("slamgpu_set_particle_assoc_sampling", "slamgpu_particle_sample_stats", "slamgpu_particle_labels")


def test_entries_declared_and_exported():
    import slam_amd
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    assert re.search(r"int slamgpu_set_particle_assoc_sampling\(slamgpu_ctx \*ctx, int32_t on\);", hdr)
    assert re.search(r"int slamgpu_particle_sample_stats\(slamgpu_ctx \*ctx, int64_t out\[3\]\);", hdr)
    assert re.search(r"int slamgpu_particle_labels\(slamgpu_ctx \*ctx, int32_t \*labels, int64_t max_count, int32_t \*nz\);", hdr)
    L = slam_amd.load_library()
    for s in ENTRIES:
        assert s in slam_amd.DECLARED_SYMBOLS and hasattr(L, s), s


def test_capi_binds_them_and_refuses_a_null_context():
    from slam_amd import capi
    L = capi.load_library()
    assert L.slamgpu_set_particle_assoc_sampling.argtypes == [C.c_void_p, C.c_int32]
    assert L.slamgpu_particle_sample_stats.argtypes == [C.c_void_p, C.c_void_p]
    assert L.slamgpu_particle_labels.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    for m in ("set_particle_assoc_sampling", "particle_sample_stats", "particle_labels"):
        assert callable(getattr(capi.SlamGpu, m)), m
    assert L.slamgpu_set_particle_assoc_sampling(None, 1) < 0
    out = np.zeros(3, np.int64)
    assert L.slamgpu_particle_sample_stats(None, out.ctypes.data_as(C.c_void_p)) < 0
    n = C.c_int32(7)
    lab = np.zeros(4, np.int32)
    assert L.slamgpu_particle_labels(None, lab.ctypes.data_as(C.c_void_p), 4, C.byref(n)) < 0
    assert L.slamgpu_last_error()


def test_slam_backend_usage_names_the_option():
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    out = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-PARTICLE_ASSOC_SAMPLE" in out
