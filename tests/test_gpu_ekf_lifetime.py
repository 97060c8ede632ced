"""Who allocates and frees what in the device EKF and the EKF ensemble (slamgpu_ekf_create / _destroy, slamgpu_ens_create / _destroy):
handles are made and closed repeatedly, on a stream of their own and on the caller's, which outlives them; every refused create says
why and leaves a null handle; an ensemble whose step buffers have grown and whose slot ring has been reset steps bit for bit as a
fresh one; the known-association table after an upload is reused and extended.  The smallest shapes: max_landmarks 0 and 4, B = 3.
Every sequence here is a legal one, and nothing here depends on how the two units are written."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
Q = np.array([[0.09, 0], [0, 0.0027]], f32)
R = np.array([[0.01, 0], [0, 0.0003]], f32)
DT = 0.025


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def state4():
    """two landmarks in front of a vehicle at the origin, a diagonal covariance"""
    x = np.array([0, 0, 0, 10, 2, 12, -3], f32)
    return x, np.diag(np.array([0.01, 0.01, 0.001, 0.2, 0.2, 0.3, 0.3], f32))


def observe(x, feats):
    """exact observations of the features `feats` of x"""
    f = 3 + 2 * np.asarray(feats)
    dx, dy = x[f] - x[0], x[f + 1] - x[1]
    return np.stack([np.hypot(dx, dy), np.arctan2(dy, dx) - x[2]], axis=1).astype(f32)


@pytest.mark.parametrize("max_landmarks", [0, 4])
def test_handles_are_made_and_closed_repeatedly(sg, max_landmarks):
    for k in range(6):
        d = sg.EkfGpu(max_landmarks, use_heading=True, sigma_phi=0.01)
        e = sg.EkfEnsemble(3, max_landmarks, use_heading=True, sigma_phi=0.01)
        if k % 2:  # (closed untouched, and closed with work in flight)
            d.sim(3.0, 0.01, Q, DT, 0.0)
            e.sim(np.tile(f32([3.0, 0.01]), (3, 1)), np.zeros(3, f32), Q, DT)
        assert d.dim == 3 and list(e.dims()) == [3, 3, 3]
        d.close()
        e.close()
    d = sg.EkfGpu(max_landmarks)
    d.predict(3.0, 0.01, Q, DT)
    xyt, Pvv = d.pose()
    assert xyt[0] > 0 and np.isfinite(Pvv).all() and Pvv[0, 0] > 0
    d.close()


def test_the_callers_stream_outlives_the_handles(sg):
    sg.load_library()
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))  # (the runtime libslamgpu.so runs on)
    vp = C.c_void_p
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    for fn in (hip.hipStreamSynchronize, hip.hipStreamDestroy, hip.hipFree):
        fn.argtypes = [vp]
    stream, buf = vp(), vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipMalloc(C.byref(buf), 64) == 0
    x, P = state4()
    own = sg.EkfGpu(4), sg.EkfEnsemble(3, 4)
    ext = sg.EkfGpu(4, external_stream=stream.value), sg.EkfEnsemble(3, 4, external_stream=stream.value)
    results = []
    for d, e in (own, ext):
        d.upload(x, P)
        d.sim(3.0, 0.01, Q, DT, 0.0, observe(x, [0, 1]), None, R, R, 1)
        for b in range(3):
            e.upload(b, x, P)
        e.sim(np.tile(f32([3.0, 0.01]), (3, 1)), np.zeros(3, f32), Q, DT, np.tile(observe(x, [0, 1]), (3, 1, 1)), None, R, R, 1)
        results.append(d.state() + e.state(2))
        d.close()
        e.close()
    for a, b in zip(*results):  # the stream a handle runs on changes nothing
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(results[0][1], P)
    # the stream still runs work
    out = np.zeros(16, np.int32)
    assert hip.hipMemsetAsync(buf, 0x5A, 64, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
    assert hip.hipMemcpy(out.ctypes.data_as(vp), buf, 64, 2) == 0 and (out == 0x5A5A5A5A).all()
    assert hip.hipStreamDestroy(stream) == 0 and hip.hipFree(buf) == 0


def refused(sg, make, piece):
    with pytest.raises(sg.SlamGpuError) as ei:
        make()
    assert ei.value.code == -1 and piece in str(ei.value), str(ei.value)  # SLAMGPU_ERR_INVALID


def test_every_refused_create_says_why_and_leaves_a_null_handle(sg):
    from slam_amd import ekf, ekf_ens
    ndev = sg.device_count()
    gates = "wheel_base must be positive, sigma_phi and the gates non-negative"
    refused(sg, lambda: sg.EkfGpu(32001), "max_landmarks 32001 outside [0, 32000]")
    refused(sg, lambda: sg.EkfEnsemble(3, 513), "max_landmarks 513 outside [0, 512]")
    refused(sg, lambda: sg.EkfEnsemble(0, 4), "members 0 outside [1, 65535]")
    refused(sg, lambda: sg.EkfGpu(4, wheel_base=0.0), gates)
    refused(sg, lambda: sg.EkfEnsemble(3, 4, wheel_base=0.0), gates)
    refused(sg, lambda: sg.EkfGpu(4, device=ndev), "device %d out of range (%d devices)" % (ndev, ndev))
    refused(sg, lambda: sg.EkfEnsemble(3, 4, device=-1), "device -1 out of range (%d devices)" % ndev)
    # the raw calls: a wrong struct_size, and the handle is null after every refusal
    L = ekf._lib()
    ekf_ens._lib()
    size = C.sizeof(ekf.EkfConfig)
    for cfg in (ekf.EkfConfig(size - 4, 0, 4, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0), ekf.EkfConfig(size, 0, 32001, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0),
                ekf.EkfConfig(size, 0, 4, 0, 1, 0, 0.0, 0.0, 4.0, 25.0, 0), ekf.EkfConfig(size, ndev, 4, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0)):
        h = C.c_void_p(1)
        assert L.slamgpu_ekf_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    h = C.c_void_p(1)
    assert L.slamgpu_ekf_create(C.byref(ekf.EkfConfig(size - 4, 0, 4, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0)), C.byref(h)) == -1 and not h.value
    assert "slamgpu_ekf_config.struct_size %d != %d (ABI mismatch)" % (size - 4, size) in L.slamgpu_last_error().decode()
    size = C.sizeof(ekf_ens.EkfEnsConfig)
    for cfg in (ekf_ens.EkfEnsConfig(size, 0, 0, 4, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0, 0), ekf_ens.EkfEnsConfig(size, 0, 3, 513, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0, 0),
                ekf_ens.EkfEnsConfig(size, 0, 3, 4, 0, 1, 0, 0.0, 0.0, 4.0, 25.0, 0, 0), ekf_ens.EkfEnsConfig(size, ndev, 3, 4, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0, 0),
                ekf_ens.EkfEnsConfig(size + 8, 0, 3, 4, 0, 1, 0, 4.0, 0.0, 4.0, 25.0, 0, 0)):
        h = C.c_void_p(1)
        assert L.slamgpu_ens_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    assert "slamgpu_ekf_ens_config.struct_size %d != %d (ABI mismatch)" % (size + 8, size) in L.slamgpu_last_error().decode()


def test_grown_buffers_and_a_reset_ring_step_as_a_fresh_handle(sg):
    """The gates, B = 3, nz = 3, then 70 (more than the 64 observations the label and input buffers start with, and a packet longer than
    a pinned slot: the buffers grow with the stream idle and the slot ring is reset), then 3 again: after each step the slabs equal,
    bit for bit, those of a fresh handle given the state before the step and the same step"""
    x, P = state4()
    rng = np.random.default_rng(5)
    kw = dict(use_heading=True, sigma_phi=0.01, gate_reject=4.0, gate_augment=25.0)
    VG, phi = np.tile(f32([3.0, 0.02]), (3, 1)), np.full(3, 0.001, f32)
    old = sg.EkfEnsemble(3, 4, **kw)
    for b in range(3):
        old.upload(b, x, P)
    for nz in (3, 70, 3):
        before = [old.state(b) for b in range(3)]
        z = np.stack([observe(before[b][0], rng.integers(0, 2, nz)) + rng.normal(0, 0.01, (nz, 2)).astype(f32) for b in range(3)])
        new = sg.EkfEnsemble(3, 4, **kw)
        for b in range(3):
            new.upload(b, *before[b])
        for e in (old, new):
            e.sim(VG, phi, Q, DT, z, None, R, R, 1)
        assert np.array_equal(old.dims(), new.dims()) and np.array_equal(old.status(), new.status()) and not old.status().any()
        for b in range(3):
            (xo, Po), (xn, Pn) = old.slab(b), new.slab(b)
            assert xo.tobytes() == xn.tobytes() and Po.tobytes() == Pn.tobytes(), (nz, b)
            assert not np.array_equal(old.state(b)[1], before[b][1])
        VGl, phil, zl = old.last_inputs()
        assert zl.shape == (3, nz, 2) and zl.tobytes() == z.tobytes() and VGl.tobytes() == VG.tobytes() and phil.tobytes() == phi.tobytes()
        new.close()
    old.close()


def test_known_association_table_after_an_upload_is_reused_and_extended(sg):
    """An upload of nf features makes the table the identity; later steps look ids up (0, 1: updates), learn new ones in observation order
    (7 then 5: features 2 and 3) and find them again.  The dimensions are the table's and the labels show in the state: an id that
    maps to feature f moves feature f"""
    x, P = state4()
    z01 = observe(x, [0, 1])
    znew = np.array([[20.0, 0.5], [25.0, -0.4]], f32)
    d = sg.EkfGpu(4, association_known=True)
    e = sg.EkfEnsemble(3, 4, association_known=True)
    d.upload(x, P)
    for b in range(3):
        e.upload(b, x, P)
    zero = np.zeros((3, 2), f32), np.zeros(3, f32)

    def step(z, ids):
        d.sim(0.0, 0.0, np.zeros((2, 2), f32), DT, 0.0, z, ids, R, R, 1)
        e.sim(*zero, np.zeros((2, 2), f32), DT, np.tile(z, (3, 1, 1)), ids, R, R, 1)
        return d.state(), e.state(1)

    for xs, Ps in step(z01, [0, 1]):  # reuse: no growth, both features tighten
        assert xs.shape[0] == 7 and (np.diag(Ps)[3:] < np.diag(P)[3:]).all()
    assert d.dim == 7 and list(e.dims()) == [7, 7, 7]
    for xs, Ps in step(np.concatenate([z01[:1], znew]), [0, 7, 5]):  # extend: id 7 -> feature 2, id 5 -> feature 3
        assert xs.shape[0] == 11
        assert np.allclose(xs[7:9], [20 * np.cos(0.5), 20 * np.sin(0.5)], atol=1e-3) and np.allclose(xs[9:11], [25 * np.cos(-0.4), 25 * np.sin(-0.4)], atol=1e-3)
    assert d.dim == 11 and list(e.dims()) == [11, 11, 11] and d.status() == 0 and not e.status().any()
    before = d.state(), e.state(1)
    z5 = observe(before[0][0], [3]) + f32([0.05, 0.0])
    for (xs, Ps), (xb, Pb) in zip(step(z5, [5]), before):  # found again: id 5 is feature 3, which moves and tightens; feature 2 keeps its variance order
        assert xs.shape[0] == 11 and Ps[9, 9] < Pb[9, 9] and Ps[10, 10] < Pb[10, 10] and xs[9:11].tobytes() != xb[9:11].tobytes()
        assert abs(np.hypot(xs[9], xs[10]) - np.hypot(xb[9], xb[10])) > 1e-3 > abs(np.hypot(xs[7], xs[8]) - np.hypot(xb[7], xb[8]))
    # the table is full (four features): one more new id is refused, by each handle in its own way, and nothing is learnt
    with pytest.raises(sg.SlamGpuError) as ei:
        d.sim(0.0, 0.0, np.zeros((2, 2), f32), DT, 0.0, znew[:1], [9], R, R, 1)
    assert ei.value.code == -3 and d.dim == 11  # SLAMGPU_ERR_CAPACITY, before anything ran
    e.sim(*zero, np.zeros((2, 2), f32), DT, np.tile(znew[:1], (3, 1, 1)), [9], R, R, 1)
    assert list(e.dims()) == [11, 11, 11] and (e.status() == sg.EKF_STATUS_CAPACITY).all()
    # a second upload makes the table the identity of ITS features: id 1 is feature 1 again, id 7 is new again
    d.upload(x, P)
    for b in range(3):
        e.upload(b, x, P)
    for xs, Ps in step(np.concatenate([z01[1:], znew[:1]]), [1, 7]):
        assert xs.shape[0] == 9 and Ps[5, 5] < P[5, 5] and Ps[3, 3] == P[3, 3]
    d.close()
    e.close()
