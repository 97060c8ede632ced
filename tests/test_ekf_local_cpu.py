"""Local periods of the device EKF (include/slamgpu.h: slamgpu_ekf_local_*), what can be checked without a GPU:
  1. the algebra: the float64 local model with its commit (tests/ekf_local_model.py) against the float64 full EkfModel on the same
     stage calls, max abs difference <= 1e-12 x scale (the heading update's eps on the passive diagonal, 2.2e-16 per update, is the
     only term the two do not share), both with the device's chunks of 64 observations, up to three chunks per update; and the
     per-block error rule of tests/test_gpu_ekf_local_scale.py on an ideal device and on wrong tiles;
  2. slamhost_ekf_local_region against numpy, the radius boundary and the overflow included;
  3. the symbols, the binding, the backend's refusals, and the new unit compiled for gfx950 without scratch."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ekf_local_model as LM
from conftest import DATA

ROOT = os.path.dirname(DATA)
f32 = np.float32

# nf, use_heading, periods
CASES = {
    "scattered": (12, True, [dict(features=[1, 4, 5, 9, 11], max_new=2, steps=6, m=3, new=[0, 2])]),
    "pose_only": (9, True, [dict(features=[], max_new=1, steps=4, m=0, new=[0, 1])]),
    "every_feature": (8, True, [dict(features=list(range(8)), max_new=2, steps=4, m=5, new=[1])]),
    "predicts_only": (10, False, [dict(features=[0, 3, 9], max_new=0, steps=5, m=0)]),
    "new_reobserved": (10, False, [dict(features=[0, 2, 7], max_new=3, steps=5, m=2, new=[1, 0, 2])]),
    "two_periods": (12, True, [dict(features=[0, 5, 6], max_new=2, steps=4, m=2, new=[2]),
                               dict(features=[3, 6, 11, 12, 13], max_new=1, steps=4, m=4, new=[0, 1])]),
    # 135, then 136 observations per update: three chunks of the device's rule (64, 64, 7 and 8), both models with chunk = 64
    "three_chunks": (150, True, [dict(features=list(range(5, 145)), max_new=1, steps=2, m=135, new=[1])]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_local_model_is_the_full_filter(name):
    nf, heading, periods = CASES[name]
    x0, P0 = LM.synthetic_state(nf, 17 + nf)
    script, ref = LM.build_script(x0, P0, periods, heading, seed=5 + nf)
    assert sum(1 for n, _ in script if n == "begin") == len(periods)
    if name == "predicts_only":
        assert {n for n, _ in script} == {"begin", "predict", "end"}
    if name in ("new_reobserved", "two_periods"):  # a feature the period (or the one before) created is observed again
        assert any(n == "update" and (a[1] >= nf).any() for n, a in script)
    if name == "three_chunks":
        assert ref.chunk == LM.CHUNK and [a[1].shape[0] for n, a in script if n == "update"] == [135, 136]
    loc = LM.EkfLocalModel(chunk=LM.CHUNK, use_heading=heading, association_known=True, **LM.CONF)
    loc.upload(x0, P0)
    LM.drive(loc, script)
    assert loc.commits == len(periods) and loc.dim == ref.dim
    dx, dP = np.abs(loc.x - ref.x).max(), np.abs(loc.P - ref.P).max()
    print("local model %s: dim %d, max |dx| %.3e, max |dP| %.3e" % (name, ref.dim, dx, dP))
    assert dx <= 1e-12 * np.abs(ref.x).max() and dP <= 1e-12 * np.abs(ref.P).max(), (dx, dP)
    assert not np.array_equal(ref.P[:3, 3 + 2 * nf - 2:3 + 2 * nf], P0[:3, -2:])  # the passive part did move


@pytest.mark.parametrize("nf,k,heading,steps,m,new", [(128, 14, True, 4, 10, [0, 3]), (130, 15, False, 5, 15, [1]), (130, 70, True, 3, 65, [3])])
def test_block_rule_passes_an_ideal_device_and_catches_a_wrong_tile(nf, k, heading, steps, m, new):
    """The per-block rule of tests/test_gpu_ekf_local_scale.py on shapes of tests/test_gpu_ekf_local.py, without a device: the float64
    local model's result rounded ONCE to float32 stands for an ideal device, the float32 full EkfModel with the device's chunks for
    the yardstick, the float64 full model is the reference.  The ideal device meets the rule in all five blocks; a 16 x 16 tile of a
    block that is 1 % wrong, or left as it was uploaded, misses its block's bound tenfold or more (P[A,B], whose float32 yardstick is 2e-5 .. 9e-5 of the
    block's largest entry, at the least by 29 times)"""
    from test_gpu_ekf_local import FACTOR, FLOOR, features_of, within
    x0, P0 = LM.synthetic_state(nf, 7 * nf + k)
    feats = features_of(nf, k, np.random.default_rng(100 * nf + k))
    script, ref = LM.build_script(x0, P0, [dict(features=feats, max_new=sum(new), steps=steps, m=m, new=new)], heading, 9 * nf + k)
    loc = LM.EkfLocalModel(chunk=LM.CHUNK, use_heading=heading, association_known=True, **LM.CONF)
    yard = LM.EkfModel(dtype=f32, chunk=LM.CHUNK, use_heading=heading, association_known=True, **LM.CONF)
    for f in (loc, yard):
        f.upload(x0, P0)
    LM.drive(loc, script)
    LM.drive(yard, script, periods=False)
    A, B = LM.blocks_of(script, x0.shape[0], ref.dim)
    assert A.shape[0] == 3 + 2 * (k + sum(new)) and B.shape[0] == 2 * (nf - k) and np.array_equal(np.sort(np.concatenate([A, B])), np.arange(ref.dim))
    x, P = loc.x.astype(f32), loc.P.astype(f32)
    ey = LM.block_errors(yard.x, yard.P, ref.x, ref.P, A, B)
    ei = LM.block_errors(x, P, ref.x, ref.P, A, B)
    print("ideal device nf %d k %d: " % (nf, k) + ", ".join("%s %.3e against %.3e" % (b, ei[b], ey[b]) for b in LM.BLOCKS))
    assert set(ei) == set(LM.BLOCKS)
    for b in LM.BLOCKS:
        assert within(ei[b], ey[b]), (b, ei[b], ey[b])
    D0 = x0.shape[0]
    for b, (I, J) in (("P[A,A]", (A, A)), ("P[A,B]", (A, B)), ("P[B,B]", (B, B))):
        blk = ref.P[np.ix_(I, J)]
        i, j = np.unravel_index(np.abs(blk).argmax(), blk.shape)  # the tile that holds the block's largest entry
        i, j = min(i // 16 * 16, len(I) - 16), min(j // 16 * 16, len(J) - 16)
        rows, cols = I[i:i + 16], J[j:j + 16]
        for what in ("1 % wrong", "stale"):
            Pw = P.copy()
            if what == "stale":
                if rows.max() >= D0 or cols.max() >= D0:
                    continue
                Pw[np.ix_(rows, cols)] = P0[np.ix_(rows, cols)]
            else:
                Pw[np.ix_(rows, cols)] *= f32(1.01)
            e = LM.block_errors(x, Pw, ref.x, ref.P, A, B)[b]
            assert e >= 10.0 * max(FACTOR * ey[b], FLOOR), (b, what, e, ey[b])


def test_local_model_contract():
    x0, P0 = LM.synthetic_state(6, 3)
    m = LM.EkfLocalModel(association_known=True, **LM.CONF)
    m.upload(x0, P0)
    with pytest.raises(LM.Invalid):
        m.local_end()
    for bad in ([2, 1], [1, 1], [6], [-1]):
        with pytest.raises(LM.Invalid):
            m.local_begin(bad, 0)
    m.local_begin([1, 4], 1)
    with pytest.raises(LM.Invalid):
        m.local_begin([0], 0)
    with pytest.raises(LM.Invalid):
        m.update(np.zeros((1, 2)), [0], LM.R)
    with pytest.raises(LM.Invalid):
        m.upload(x0, P0)
    m.augment([[15.0, 0.3]], LM.R)
    with pytest.raises(LM.Capacity):
        m.augment([[16.0, 1.3]], LM.R)
    assert m.dim == 3 + 2 * 7
    m.update([[15.0, 0.3]], [6], LM.R)  # the new one, by its global index
    m.local_end()
    assert m.x.shape[0] == 17 and np.allclose(m.P, m.P.T, rtol=0, atol=1e-12)


def region(x, radius):
    x = np.asarray(x, f32)
    dx, dy = x[3::2] - x[0], x[4::2] - x[1]
    return np.nonzero(dx * dx + dy * dy <= f32(radius) * f32(radius))[0].astype(np.int32)


def test_host_region_matches_numpy():
    from slam_amd import host
    assert "slamhost_ekf_local_region" in host.DECLARED_SYMBOLS
    rng = np.random.default_rng(4)
    x = np.concatenate([[1.5, -2.0, 0.3], rng.uniform(-60, 60, 2 * 500)]).astype(f32)
    for radius in (0.0, 5.0, 25.0, 40.0, 200.0):
        got = host.ekf_local_region(x, radius)
        assert np.array_equal(got, region(x, radius)) and (np.diff(got) > 0).all(), radius
    assert host.ekf_local_region(x, 40.0).shape[0] > 50
    # the boundary belongs to the region: 3-4-5 triangles around a pose with exact coordinates
    x = np.array([1, 2, 0, 4, 6, -2, -2, 1, 7.0000005, 1, 7], f32)  # features at distance 5, 5, 5 + an ulp, 5
    assert np.array_equal(host.ekf_local_region(x, 5.0), [0, 1, 3]) and np.array_equal(region(x, 5.0), [0, 1, 3])
    assert np.array_equal(host.ekf_local_region(x, np.nextafter(f32(5), f32(0))), [])
    # more than max_count: refused, and exactly max_count is not
    assert host.ekf_local_region(x, 5.0, max_count=2) is None
    assert np.array_equal(host.ekf_local_region(x, 5.0, max_count=3), [0, 1, 3])
    assert host.ekf_local_region(x[:3], 5.0).shape[0] == 0
    for bad in (x[:4], x[:2]):
        with pytest.raises(ValueError):
            host.ekf_local_region(bad, 5.0)
    with pytest.raises(ValueError):
        host.ekf_local_region(x, -1.0)


LOCAL_SYMBOLS = ["slamgpu_ekf_local_begin", "slamgpu_ekf_local_end", "slamgpu_ekf_local_info", "slamgpu_ekf_lookup"]


def test_library_exports_the_local_entry_points():
    import slam_amd
    from slam_amd import ekf
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    a, b = hdr.index("#ifdef SLAMGPU_EXPERIMENTAL"), hdr.index("#endif /* SLAMGPU_EXPERIMENTAL */")
    stable = hdr[:a] + hdr[b:]
    out = subprocess.run(["nm", "-D", "--defined-only", slam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    for s in LOCAL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, stable) and s in slam_amd.DECLARED_SYMBOLS and re.search(r"\bT %s$" % s, out, re.M), s
    for piece in ("Guivant and Nebot", "left out of the passive part's diagonal", "stale by design"):
        assert piece in stable, piece
    L = ekf._lib()
    assert L.slamgpu_ekf_local_begin(None, None, 0, 0) == -1 and L.slamgpu_ekf_local_end(None) == -1
    assert L.slamgpu_ekf_local_info(None, None) == -1 and L.slamgpu_ekf_lookup(None, None, 0, None) == -1
    for m in ("local_begin", "local_end", "local_info", "lookup", "local"):
        assert callable(getattr(slam_amd.EkfGpu, m)), m


def test_backend_refuses_local_periods_it_cannot_run():
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    m = os.path.join(DATA, "example_loop1.mat")

    def run(*args):
        return subprocess.run([exe, "-m", m, *args], capture_output=True, text=True, timeout=60)
    for args in (("-method", "EKF1", "-EKF_LOCAL", "20"), ("-method", "EKF1", "-ekf", "host", "-EKF_LOCAL", "20"),
                 ("-method", "FASTSLAM2", "-EKF_LOCAL", "20")):
        r = run(*args)
        assert r.returncode != 0 and "-EKF_LOCAL margin: with -method EKF1 -ekf device" in r.stderr, args
    r = run("-method", "EKF1", "-ekf", "device", "-runs", "8", "-EKF_LOCAL", "20")
    assert r.returncode != 0 and "-EKF_LOCAL margin: not with -runs" in r.stderr
    for margin in ("0", "-3", "x"):
        r = run("-method", "EKF1", "-ekf", "device", "-EKF_LOCAL", margin)
        assert r.returncode != 0 and "-EKF_LOCAL margin: margin must be > 0" in r.stderr, margin
    r = run("-method", "EKF1", "-ekf", "device", "-EKF_LOCAL_NEW", "8")
    assert r.returncode != 0 and "-EKF_LOCAL_NEW n: with -EKF_LOCAL margin" in r.stderr
    r = run("-method", "EKF1", "-ekf", "device", "-EKF_LOCAL", "20", "-EKF_LOCAL_NEW", "0")
    assert r.returncode != 0 and "-EKF_LOCAL_NEW n: n must be >= 1" in r.stderr
    assert "-EKF_LOCAL margin" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout


def test_local_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """ekf_local.cpp cross-compiles with ekf.o's flags, is one of the library's units, and every kernel's private segment is 0 bytes"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "slam_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = {u: re.search(r"^\$\(BUILD\)/%s\.o:.*\n\t\$\(HIPCC\) \$\(COMMON\) (.*) -x hip -c" % u, mk, re.M).group(1).split() for u in ("ekf", "ekf_local")}
    assert flags["ekf_local"] == flags["ekf"]
    assert "$(BUILD)/ekf_local.o" in re.search(r"^HOSTOBJS := (.*)$", mk, re.M).group(1)
    out = str(tmp_path / "ekf_local.s")
    subprocess.run([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + src, "-I" + os.path.join(ROOT, "include"), *flags["ekf_local"],
                    "-x", "hip", "-S", "--cuda-device-only", "-o", out, os.path.join(src, "ekf_local.cpp")], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = open(out).read()
    sizes = dict(zip(re.findall(r"\.amdhsa_kernel\s+(\S+)", asm), map(int, re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm))))
    names = " ".join(sizes)
    for k in ("ekf_local_gather_kernel", "ekf_local_augment_kernel", "ekf_local_psi_chunk_kernel", "ekf_local_psi_heading_kernel", "ekf_local_t_kernel",
              "ekf_local_bb_kernel", "ekf_local_ab_kernel", "ekf_local_xb_kernel", "ekf_local_scatter_kernel"):
        assert k in names, k
    for kernel, size in sizes.items():
        assert size == 0, (kernel, size)
    # the commit's two products are on the matrix cores: P[B, B] in float64, P[A, B] in exact float32
    assert asm.count("v_mfma_f64_16x16x4_f64") >= 16 and asm.count("v_mfma_f32_32x32x2_f32") >= 64
