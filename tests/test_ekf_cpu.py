"""The device EKF (include/slamgpu.h: slamgpu_ekf_*), what can be checked without a GPU: the float64 model the GPU tests measure
against (tests/ekf_model.py) follows the host filter over a whole run; the host filter with explicit inputs (slamhost_ekf_sim)
is the host filter; the symbols, the backend's refusals, and ekf.cpp compiled for gfx950 with no kernel in scratch."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT, bits_equal

f32 = np.float32


def host_run(mapname, seed):
    from slam_amd import host
    sim = host.HostSim(["-m", os.path.join(DATA, mapname + ".mat"), "-method", "EKF1", "-SWITCH_SEED_RANDOM", seed])
    return sim, host.HostEkf(sim)


def model_for(sim, **kw):
    import ekf_model
    c = sim.conf
    return ekf_model.EkfModel(use_heading=c.SWITCH_HEADING_KNOWN == 1, batch_update=c.SWITCH_BATCH_UPDATE == 1,
                              association_known=c.SWITCH_ASSOCIATION_KNOWN != 0, wheel_base=c.WHEELBASE, sigma_phi=c.sigmaT,
                              gate_reject=c.GATE_REJECT, gate_augment=c.GATE_AUGMENT, **kw)


def test_model_follows_the_host_filter_over_a_whole_run():
    """example_loop1, seed 3 (heading observed): the float64 model, fed what the host filter was fed, has the host's dimension on every
    control step -- the same association decisions -- and its pose within the bound test_host_ekf_matches_reference holds the host to"""
    sim, ekf = host_run("example_loop1", 3)
    nz = sim.sim_noise()
    mdl = model_for(sim)
    k = 0
    while True:
        r = ekf.step()
        if r < 0:
            break
        V, G, phi, ob = ekf.last_inputs()
        assert ob == r
        z, vis = sim.last_z()
        mdl.sim(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], ob)
        x, _ = ekf.state(want_P=False)
        assert mdl.dim == x.shape[0], k
        assert np.abs(mdl.x[:3] - x[:3]).max() <= 1e-3, k
        k += 1
    assert k > 1000 and mdl.nf > 10
    x, P = ekf.state()
    assert np.abs(mdl.x - x).max() <= 2e-3 and np.abs(mdl.P - P).max() <= 1e-3 * np.abs(P).max()
    ekf.close()
    sim.close()


@pytest.mark.parametrize("mapname,seed", [("example_loop1", 3), ("example_webmap", 7)])
def test_host_filter_with_explicit_inputs_is_the_host_filter(mapname, seed):
    """slamhost_ekf_sim fed slamhost_ekf_last_inputs, slamhost_sim_last_z and slamhost_sim_noise reproduces slamhost_ekf_step bit for
    bit, 300 control steps"""
    from slam_amd import host
    sim, a = host_run(mapname, seed)
    b = host.HostEkf(sim)
    nz = sim.sim_noise()
    nobs = 0
    for k in range(300):
        r = a.step()
        assert r >= 0
        V, G, phi, ob = a.last_inputs()
        z, vis = sim.last_z()
        b.sim_step(V, G, nz["Qe"], nz["dt"], phi, z, vis, nz["Re"], nz["R"], ob)
        nobs += ob
        xa, Pa = a.state()
        xb, Pb = b.state()
        assert bits_equal(xa, xb) and bits_equal(Pa, Pb), k
    assert nobs > 20 and xa.shape[0] > 3
    # ... and an uploaded state is the state
    b.upload(xa[:5], Pa[:5, :5])
    xb, Pb = b.state()
    assert bits_equal(xb, xa[:5]) and bits_equal(Pb, Pa[:5, :5])
    for e in (a, b):
        e.close()
    sim.close()


@pytest.mark.parametrize("nf", [65, 257, 512, 600])
def test_scale_packet_is_decided_clearly_by_the_float64_model(nf):
    """The packet of 64 readings tests/test_gpu_ekf_scale.py sends through the gates of large maps, judged by the float64 model alone
    with EkfModel.associate's margin: at most 2 decisions within 1e-3 of a gate or of a rival, at least 40 matches and 6 new landmarks,
    and at 600 features at least 5 winners that are not the feature the reading came from (test_gpu_ekf_scale.caps).  The model's float32
    evaluation labels every clear decision alike, so a correct float32 kernel has room"""
    import ekf_model
    from test_gpu_ekf_scale import GATES, RE, caps, study
    s = study(nf)
    foreign = caps(s)
    lab, margin, clear = s["lab"], s["margin"], s["clear"]
    print("EKF scale packet nf %d: unclear %d, smallest margin %.1e, match / new / discard %d / %d / %d, foreign winners %d" %
          (nf, (~clear).sum(), margin.min(), (lab >= 0).sum(), (lab == -1).sum(), (lab == -2).sum(), foreign))
    assert lab.shape == (64,) and np.isfinite(margin).all() and (margin >= 0).all()
    m32 = ekf_model.EkfModel(dtype=f32, **GATES)
    m32.upload(s["x0"], s["P0"])
    assert np.array_equal(m32.associate(s["z"], RE)[clear], lab[clear])
    # the margin is what it says: each term recomputed for one reading, and the labels do not depend on asking for it
    mdl = ekf_model.EkfModel(**GATES)
    mdl.upload(s["x0"], s["P0"])
    assert np.array_equal(mdl.associate(s["z"], RE), lab)
    i = int(np.argmin(margin))
    zp, H, cols = mdl._model(np.arange(nf))
    S = H @ mdl.P[cols[:, :, None], cols[:, None, :]] @ H.transpose(0, 2, 1) + RE.astype(np.float64)
    v = s["z"][i].astype(np.float64) - zp
    v[:, 1] = (v[:, 1] + np.pi) % (2 * np.pi) - np.pi
    nis = np.array([v[j] @ np.linalg.solve(S[j], v[j]) for j in range(nf)])
    nd = np.sort((nis + np.log(np.linalg.det(S)))[nis < 4.0])
    want = min(np.abs(nis - 4.0).min(), np.abs(nis - 25.0).min(), nd[1] - nd[0] if nd.shape[0] > 1 else np.inf)
    assert abs(margin[i] - want) <= 1e-9 * max(1.0, want), (margin[i], want)
    # no features: everything is new and nothing was compared
    empty = ekf_model.EkfModel(**GATES)
    l0, m0 = empty.associate(s["z"][:3], RE, want_margin=True)
    assert (l0 == -1).all() and np.isinf(m0).all()


@pytest.mark.parametrize("which", ["odd", "tail"])
def test_scale_packet_inside_a_period_is_decided_clearly_by_the_float64_model(which):
    """The same packet through the gates of a local period of 600 landmarks' odd features (k 300) and of features 257 .. 599 (k 343),
    as tests/test_gpu_ekf_local_scale.py sends it, judged by the float64 local model: at most 2 unclear decisions, at least 40 / 30
    matches, at least 5 winners at a local index of 256 or more, at least 20 labels that differ from the full map's for the same
    reading, and in the odd-feature period, whose labels that file applies, room for every new landmark
    (test_gpu_ekf_local_scale.period_caps).  The float32 local model labels every clear decision
    alike, and a label is a feature of the period, by its global index"""
    import ekf_local_model as LM
    from test_gpu_ekf_local_scale import MAX_NEW, period_caps, period_study
    from test_gpu_ekf_scale import GATES, RE
    p = period_study(which)
    matches, past, differ = period_caps(p)
    lab, margin, clear, feats = p["lab"], p["margin"], p["clear"], p["feats"]
    print("EKF local scale packet, %s features (k %d): unclear %d, smallest margin %.1e, match / new / discard %d / %d / %d, local index >= 256: %d, "
          "differ from the full map's: %d" % (which, feats.shape[0], (~clear).sum(), margin.min(), matches, (lab == -1).sum(), (lab == -2).sum(), past, differ))
    assert lab.shape == (64,) and np.isfinite(margin).all() and (margin >= 0).all()
    assert np.isin(lab[lab >= 0], feats).all()
    m32 = LM.EkfLocalModel(dtype=f32, **GATES)
    m32.upload(p["x0"], p["P0"])
    m32.local_begin(feats, MAX_NEW)
    assert np.array_equal(m32.associate(p["z"], RE)[clear], lab[clear])


EKF_SYMBOLS = ["slamgpu_ekf_create", "slamgpu_ekf_destroy", "slamgpu_ekf_sim", "slamgpu_ekf_predict", "slamgpu_ekf_observe_heading",
               "slamgpu_ekf_associate", "slamgpu_ekf_update", "slamgpu_ekf_augment", "slamgpu_ekf_dim", "slamgpu_ekf_pose", "slamgpu_ekf_state",
               "slamgpu_ekf_block", "slamgpu_ekf_upload", "slamgpu_ekf_status", "slamgpu_ekf_sync"]


def test_library_exports_what_the_header_declares():
    import slam_amd
    from slam_amd import host
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    stable = hdr[:hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")]
    declared = sorted(set(re.findall(r"\b(slamgpu_ekf_[a-z_0-9]+)\s*\(", stable)))
    assert declared == sorted(EKF_SYMBOLS)
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr) and re.search(r"#define SLAMGPU_EKF_STATUS_NOT_PD 1\b", stable)
    out = subprocess.run(["nm", "-D", "--defined-only", slam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    for s in EKF_SYMBOLS:
        assert s in slam_amd.DECLARED_SYMBOLS and re.search(r"\bT %s$" % s, out, re.M), s
    # the header says what the device does differently from the reference
    doc = stable[stable.index("EKF-SLAM on the device"):stable.index("typedef struct slamgpu_ekf slamgpu_ekf;")]
    for piece in ("DEVIATION for m > 64", "SKIPPED", "the reference carries on with the broken factor"):
        assert piece in doc, piece
    assert callable(slam_amd.EkfGpu) and slam_amd.EKF_STATUS_NOT_PD == 1
    L = host.load_library()
    for s in ("slamhost_ekf_sim", "slamhost_ekf_upload", "slamhost_ekf_last_inputs", "slamhost_sim_noise"):
        assert s in host.DECLARED_SYMBOLS and hasattr(L, s), s


def test_null_handle_and_missing_gpu_are_refused():
    import ctypes as C
    import slam_amd
    from slam_amd import ekf
    L = ekf._lib()
    assert L.slamgpu_ekf_dim(None) == -1 and L.slamgpu_ekf_sync(None) == -1 and L.slamgpu_ekf_observe_heading(None, 0.0) == -1
    cfg = ekf.EkfConfig(C.sizeof(ekf.EkfConfig) - 4, 0, 8, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0)
    h = C.c_void_p()
    assert L.slamgpu_ekf_create(C.byref(cfg), C.byref(h)) == -1 and not h.value  # SLAMGPU_ERR_INVALID: struct_size
    if slam_amd.device_count() == 0:
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            slam_amd.EkfGpu(8)
        assert ei.value.code == -4 and "no CPU fallback" in str(ei.value)  # SLAMGPU_ERR_NO_DEVICE


def test_backend_refuses_what_the_device_filter_cannot_do():
    import slam_amd
    exe = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
    m = os.path.join(DATA, "example_loop1.mat")
    r = subprocess.run([exe, "-m", m, "-method", "FASTSLAM2", "-ekf", "device"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-ekf device: with -method EKF1 only" in r.stderr
    r = subprocess.run([exe, "-m", m, "-method", "EKF1", "-ekf", "somewhere"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-ekf host|device" in r.stderr
    assert "-ekf host|device" in subprocess.run([exe, "-h"], capture_output=True, text=True).stdout
    # -ekf host is the default path
    r = subprocess.run([exe, "-m", m, "-method", "EKF1", "-ekf", "host", "-SWITCH_SEED_RANDOM", "3", "-maxsteps", "300"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and "control steps 300" in r.stdout and "EKF on the device" not in r.stdout
    if slam_amd.device_count() == 0:
        r = subprocess.run([exe, "-m", m, "-method", "EKF1", "-ekf", "device"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_ekf_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """ekf.cpp cross-compiles with the Makefile's flags and every kernel's private segment is 0 bytes (read as
    test_no_kernel_spills_to_scratch reads it)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "slam_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    rule = re.search(r"^\$\(BUILD\)/ekf\.o:.*\n\t\$\(HIPCC\) \$\(COMMON\) (.*) -x hip -c", mk, re.M)
    assert rule and rule.group(1).split() == ["-ffp-contract=on", "-fno-slp-vectorize"]
    assert "$(BUILD)/ekf.o" in re.search(r"^HOSTOBJS := (.*)$", mk, re.M).group(1)
    out = str(tmp_path / "ekf.s")
    subprocess.run([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + src, "-I" + os.path.join(ROOT, "include"), *rule.group(1).split(),
                    "-x", "hip", "-S", "--cuda-device-only", "-o", out, os.path.join(src, "ekf.cpp")], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = open(out).read()
    sizes = dict(zip(re.findall(r"\.amdhsa_kernel\s+(\S+)", asm), map(int, re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm))))
    names = " ".join(sizes)
    for k in ("ekf_predict_kernel", "ekf_heading_kernel", "ekf_gate_kernel", "ekf_innov_kernel", "ekf_chol_kernel", "ekf_gain_kernel",
              "ekf_syrk_kernel", "ekf_augment_kernel"):
        assert k in names, k
    for kernel, size in sizes.items():
        assert size == 0, (kernel, size)
