"""The exclusion rule's radius from the observation spacing (slamgpu_set_particle_excl_spacing / slamgpu_particle_excl_radii): the
entry points are declared, exported and bound, and slam-backend offers the option -- no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import DATA

ROOT = os.path.dirname(DATA)
ENTRIES = ("slamgpu_set_particle_excl_spacing", "slamgpu_particle_excl_radii")


def test_entries_declared_and_exported():
    import slam_amd
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    assert re.search(r"int slamgpu_set_particle_excl_spacing\(slamgpu_ctx \*ctx, float f\);", hdr)
    assert re.search(r"int slamgpu_particle_excl_radii\(slamgpu_ctx \*ctx, float \*rho, int32_t max_count, int32_t \*nz\);", hdr)
    L = slam_amd.load_library()
    for s in ENTRIES:
        assert s in slam_amd.DECLARED_SYMBOLS and hasattr(L, s), s


def test_capi_binds_them_and_refuses_a_null_context():
    from slam_amd import capi
    L = capi.load_library()
    assert L.slamgpu_set_particle_excl_spacing.argtypes == [C.c_void_p, C.c_float]
    assert L.slamgpu_particle_excl_radii.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    assert callable(capi.SlamGpu.set_particle_excl_spacing) and callable(capi.SlamGpu.particle_excl_radii)
    assert L.slamgpu_set_particle_excl_spacing(None, 0.5) < 0
    n = C.c_int32(7)
    rho = np.zeros(4, np.float32)
    assert L.slamgpu_particle_excl_radii(None, rho.ctypes.data_as(C.c_void_p), 4, C.byref(n)) < 0
    assert L.slamgpu_last_error()


def test_slam_backend_usage_names_the_option():
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    out = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "-PARTICLE_EXCL_SPACING" in out
