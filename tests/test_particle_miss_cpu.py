"""Negative information for the per-particle steps (slamgpu_set_particle_miss / slamgpu_particle_missed / slamgpu_particle_miss_stats):
the entries are declared in the stable part of the header, exported and bound; slam-backend names its two keys and refuses one without
the other -- no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import DATA

ROOT = os.path.dirname(DATA)
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
ENTRIES = ("slamgpu_set_particle_miss", "slamgpu_particle_missed", "slamgpu_particle_miss_stats")


def test_entries_declared_stable_and_exported():
    import slam_amd
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    assert re.search(r"int slamgpu_set_particle_miss\(slamgpu_ctx \*ctx, float p_miss, float view_range, float view_front\);", hdr)
    assert re.search(r"int slamgpu_particle_missed\(slamgpu_ctx \*ctx, int32_t \*count, int32_t max_count, int32_t \*n\);", hdr)
    assert re.search(r"int slamgpu_particle_miss_stats\(slamgpu_ctx \*ctx, int64_t out\[3\]\);", hdr)
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # additions to the stable part: the version stays
    L = slam_amd.load_library()
    for name in ENTRIES:
        # in the stable part, next to the other per-particle setters
        assert hdr.index("int slamgpu_set_particle_assoc_sampling(") < hdr.index("int %s(" % name) < hdr.index("#ifdef SLAMGPU_EXPERIMENTAL"), name
        assert name in slam_amd.DECLARED_SYMBOLS and hasattr(L, name), name
    # the diagnostic counter of the box test is exported, and not part of the stable ABI
    assert hdr.index("int slamgpu_particle_miss_visited(") > hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")
    assert hasattr(L, "slamgpu_particle_miss_visited")


def test_capi_binds_them_and_a_null_context_is_refused():
    from slam_amd import capi
    L = capi.load_library()
    assert L.slamgpu_set_particle_miss.argtypes == [C.c_void_p, C.c_float, C.c_float, C.c_float]
    assert L.slamgpu_particle_missed.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    assert L.slamgpu_particle_miss_stats.argtypes == [C.c_void_p, C.c_void_p]
    for name in ("set_particle_miss", "particle_missed", "particle_miss_stats"):
        assert callable(getattr(capi.SlamGpu, name)), name
    assert L.slamgpu_set_particle_miss(None, 0.5, 20.0, 1.0) < 0 and L.slamgpu_last_error()
    cnt, n = np.zeros(4, np.int32), C.c_int32(-1)
    assert L.slamgpu_particle_missed(None, cnt.ctypes.data_as(C.c_void_p), 4, C.byref(n)) < 0 and not cnt.any()
    out = np.zeros(3, np.int64)
    assert L.slamgpu_particle_miss_stats(None, out.ctypes.data_as(C.c_void_p)) < 0 and not out.any()


def test_slam_backend_names_both_keys_and_refuses_one_without_the_other():
    out = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-PARTICLE_MISS p" in out and "-PARTICLE_MISS_MARGIN m" in out
    base = [EXE, "-m", os.path.join(DATA, "example_webmap.mat"), "-method", "FASTSLAM2", "-rng", "philox", "-NPARTICLES", "512", "-maxsteps", "10"]
    for extra in (["-assoc", "particle", "-PARTICLE_MISS", "0.5"],                                   # one key without the other
                  ["-assoc", "particle", "-PARTICLE_MISS_MARGIN", "3"],
                  ["-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "3"],                            # without -assoc particle
                  ["-assoc", "gated", "-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "3"],
                  ["-assoc", "particle", "-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "-1"],     # m >= 0
                  ["-assoc", "particle", "-PARTICLE_MISS", "0.5", "-PARTICLE_MISS_MARGIN", "60"],     # m < MAX_RANGE (60 in the .ini)
                  ["-assoc", "particle", "-PARTICLE_MISS", "0", "-PARTICLE_MISS_MARGIN", "3"],        # 0 < p <= 1
                  ["-assoc", "particle", "-PARTICLE_MISS", "1.5", "-PARTICLE_MISS_MARGIN", "3"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "-PARTICLE_MISS p -PARTICLE_MISS_MARGIN m" in r.stderr and "control steps" not in r.stdout, (extra, r.stderr)
