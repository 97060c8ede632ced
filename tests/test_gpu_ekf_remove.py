"""slamgpu_ekf_remove and slamgpu_ekf_feature_stats (include/slamgpu.h; slam_amd/csrc/ekf.cpp) on the GPU.  A removal is pure data
movement, so every check is bit for bit: against the numpy gather of tests/ekf_remove_model.py, and against a fresh handle uploaded
with the gathered state.
  1. the gather over shapes on both sides of the wave, workgroup, tile and ld edges, every removal set against every shape;
  2. continuation: the stages after a removal;  3. the known association's table;  4. the counters, through a local period too;
  5. the contract: refusals change nothing, nothing synchronises;  6. slam-backend -ekf device -EKF_PRUNE_*.
What no entry point can read is not checked: x beyond the new dim (slamgpu_ekf_state ends at dim; the continuation test would see a
non-zero there only through P, which slamgpu_ekf_block does read in full)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ekf_local_model as LM
import ekf_remove_model as RM
from conftest import DATA, bits_equal
from test_ekf_remove_cpu import removal_sets, report

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(777.25)
ROOT = os.path.dirname(DATA)
EXE = os.path.join(ROOT, "slam_amd", "bin", "slam-backend")
SHAPES = [1, 2, 31, 63, 64, 130, 512]  # dim 5, 7, 65, 129, 131, 263, 1027
SETS = ["first", "last", "all", "every_other", "run", "half", "none"]
EXTRA = 2  # features of capacity beyond the map: what lies there must stay as it was uploaded


def make_dev(max_landmarks, **kw):
    import slam_amd
    return slam_amd.EkfGpu(max_landmarks, **dict(LM.CONF, **kw))


def uploaded(nf, x0, P0, **kw):
    """a handle of capacity nf + EXTRA with the sentinel everywhere beyond the state"""
    cap = 3 + 2 * (nf + EXTRA)
    d = make_dev(nf + EXTRA, **kw)
    d.upload(np.full(cap, SENTINEL), np.full((cap, cap), SENTINEL))
    d.upload(x0, P0)
    return d, cap


def whole(d, cap):
    return d.block(np.arange(cap, dtype=np.int32))


def check_removed(d, cap, x0, P0, feats, tag):
    """the handle after remove(feats) from (x0, P0): the model's gather, the zero strip, the sentinel"""
    D, n = x0.shape[0], x0.shape[0] - 2 * len(feats)
    xm, Pm = RM.gather(x0, P0, feats)
    assert d.dim == n, tag
    x, P = d.state()
    full = whole(d, cap)
    assert bits_equal(x, xm) and bits_equal(P, Pm) and bits_equal(full[:n, :n], Pm), tag
    assert (full[n:D, :D] == 0).all() and (full[:D, n:D] == 0).all(), tag
    assert (full[D:, :] == SENTINEL).all() and (full[:, D:] == SENTINEL).all(), tag
    return P


# ---- 1. the gather ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("nf", SHAPES)
def test_remove_is_the_gather(nf, which):
    feats = removal_sets(nf)[which]
    x0, P0 = RM.distinct_state(nf)
    d, cap = uploaded(nf, x0, P0)
    before = whole(d, cap)
    d.remove(feats)
    P = check_removed(d, cap, x0, P0, feats, (nf, which))
    assert bits_equal(P, P.T.copy())
    if which == "none":
        assert bits_equal(whole(d, cap), before) and bits_equal(d.state()[0], x0)
    assert d.status() == 0
    d.close()


@pytest.mark.parametrize("which", ["first", "run", "half", "last"])
@pytest.mark.parametrize("nf", SHAPES)
def test_an_asymmetric_upload_comes_out_as_the_mirrored_lower_triangle(nf, which):
    """every ORDERED pair has a value of its own: wherever an index at or beyond the first removed entry is involved the result is
    the lower triangle's gather on both sides; the entries below it are not touched"""
    feats = removal_sets(nf)[which]
    x0, P0 = RM.distinct_state(nf, asymmetric=True)
    d, cap = uploaded(nf, x0, P0)
    d.remove(feats)
    P = check_removed(d, cap, x0, P0, feats, (nf, which))
    s0, src = 3 + 2 * int(feats[0]), RM.src_map(nf, feats)
    low = (np.tril(P0) + np.tril(P0, -1).T)[np.ix_(src, src)]
    moved = np.maximum.outer(np.arange(P.shape[0]), np.arange(P.shape[0])) >= s0
    assert np.array_equal(P[moved], low[moved]) and np.array_equal(P[moved], P.T[moved]) and bits_equal(P[:s0, :s0], P0[:s0, :s0])
    d.close()


def test_removals_in_a_row_reuse_the_staging():
    """three removals enqueued back to back on one handle: each index map has reached the device before the next one is written"""
    nf = 130
    x0, P0 = RM.distinct_state(nf)
    d, cap = uploaded(nf, x0, P0)
    x, P = x0, P0
    for feats in ([0, 64, 129], [1, 2, 3, 100], [60]):
        d.remove(feats)
        x, P = RM.gather(x, P, feats)
    xd, Pd = d.state()
    assert d.dim == 3 + 2 * (nf - 8) and bits_equal(xd, x) and bits_equal(Pd, P)
    d.close()


# ---- 2. continuation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,which", [(130, "half"), (130, "first"), (63, "every_other"), (200, "run")])
def test_the_filter_after_a_removal_is_the_filter_uploaded_with_the_gathered_state(nf, which):
    """predict, heading, associate, update (m on both sides of the chunk of 64) and augment on the handle that removed and on a fresh
    handle uploaded with the model's gather: labels, x, P (up to the capacity), dim and status, bit for bit.  Anything the removal
    leaves stale -- in the vacated strip, where augment appends, in the heading update's scratch vectors -- shows here"""
    feats = removal_sets(nf)[which]
    x0, P0 = LM.synthetic_state(nf, 3 * nf + 1)
    a, cap = uploaded(nf, x0, P0, use_heading=True)
    b = make_dev(nf + EXTRA, use_heading=True)
    xg, Pg = RM.gather(x0, P0, feats)
    D = x0.shape[0]
    far = np.full((cap, cap), SENTINEL)
    far[:D, :D] = 0  # (what the removal vacates is zero, as a fresh handle's memory is)
    b.upload(np.concatenate([np.zeros(D, f32), np.full(cap - D, SENTINEL)]), far)
    b.upload(xg, Pg)
    a.remove(feats)
    rng = np.random.default_rng(nf)
    left = nf - len(feats)
    for step, m in enumerate((min(10, left), min(65, left), min(63, left))):
        x, _ = a.state()
        now = (x.shape[0] - 3) // 2
        seen = np.sort(rng.permutation(now)[:m]).astype(np.int32)
        z = np.concatenate([LM.observations(x, seen, rng, noise=0.3), np.array([[9.0 + step, 2.0]], f32)])
        labels = []
        for d in (a, b):
            d.predict(3.0, float(f32(0.04 * (-1) ** step)), LM.Q, LM.DT)
            d.observe_heading(float(f32(x[2] + 0.002)))
            labels.append(d.associate(z, LM.R))
            d.update(z[:m], seen, LM.R)
            if step < EXTRA:
                d.augment(z[m:], LM.R)
        assert np.array_equal(labels[0], labels[1]), (step, labels)
        (xa, Pa), (xb, Pb) = a.state(), b.state()
        assert a.dim == b.dim == 3 + 2 * (left + min(step + 1, EXTRA)) and bits_equal(xa, xb) and bits_equal(Pa, Pb), step
        assert bits_equal(whole(a, cap), whole(b, cap)) and a.status() == b.status() == 0, step
    assert bits_equal(Pa, Pa.T.copy()) and not bits_equal(Pa[:3, :3], P0[:3, :3])
    a.close()
    b.close()


# ---- 3. the known association -----------------------------------------------------------------------------------------------------------------
def test_the_id_table_follows_a_removal():
    nf = 70
    x0, P0 = LM.synthetic_state(nf, 9)
    d, cap = uploaded(nf, x0, P0, association_known=True)  # id f is feature f
    feats = np.array([0, 5, 6, 40, 69], np.int32)
    d.remove(feats)
    ren = RM.renumber(nf, feats)
    assert np.array_equal(d.lookup(np.arange(nf + 3)), np.concatenate([ren, [-1, -1, -1]]))
    x, _ = d.state()
    z = np.concatenate([LM.observations(x, [int(ren[7]), int(ren[41])], np.random.default_rng(1), noise=0.1), np.array([[12.0, 0.5]], f32)])
    d.sim(3.0, float(f32(0.04)), LM.Q, LM.DT, 0.1, z, [7, 41, 40], LM.R, LM.R, 1)  # id 40 was removed: a new feature at the end
    assert d.dim == 3 + 2 * (nf - 5 + 1) and np.array_equal(d.lookup([7, 41, 40, 0]), [ren[7], ren[41], nf - 5, -1])
    st = d.feature_stats()
    hits = np.zeros(nf - 4, np.int32)
    hits[[ren[7], ren[41]]] = 1
    assert np.array_equal(st["hits"], hits) and st["epoch"] == 1 and st["born"][-1] == 1 and (st["born"][:-1] == 0).all()
    d.close()


# ---- 4. the counters --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_update", [True, False])
def test_the_counters_match_the_integer_model(batch_update):
    nf = 12
    x0, P0 = LM.synthetic_state(nf, 4)
    d = make_dev(nf + 6, association_known=True, batch_update=batch_update)
    c = RM.Counters(batch_update=batch_update)
    rng = np.random.default_rng(6)
    ctl = (3.0, float(f32(0.04)), LM.Q, LM.DT, 0.1)
    assert c.equals(d.feature_stats())
    d.upload(x0, P0)
    c.upload(nf)
    assert c.equals(d.feature_stats())

    def obs(feats):
        return LM.observations(d.state()[0], feats, rng, noise=0.1)

    d.update(obs([0, 2, 2]), [0, 2, 2], LM.R)  # a direct update counts whatever batch_update says: the caller ran the stage
    c.update([0, 2, 2])
    d.augment([[15.0, 0.3]], LM.R)  # feature 12, born at the epoch as it stands
    c.augment(1)
    d.predict(*ctl[:4])
    assert c.equals(d.feature_stats()) and c.epoch == 1 and c.born[-1] == 1
    z = np.concatenate([obs([3, 12]), np.array([[14.0, -0.7]], f32)])
    d.sim(*ctl, z, [3, 12, 50], LM.R, LM.R, 1)  # ids 12 and 50 have not been seen (feature 12 came from a direct augment): features 13 and 14
    c.sim([3], 2)
    assert c.equals(d.feature_stats()) and d.dim == 3 + 2 * 15
    d.sim(*ctl, None, None, None, None, 0)  # a control step
    assert c.equals(d.feature_stats())
    # ... through a local period: global indices, the features it creates included
    x = d.state()[0]
    z_in = LM.observations(x, [1, 13], rng, noise=0.1)
    d.local_begin([0, 1, 2, 13], 2)
    d.update(z_in, [1, 13], LM.R)
    c.update([1, 13])
    d.augment([[16.0, 1.3]], LM.R)
    c.augment(1)
    d.sim(*ctl, np.concatenate([z_in[:1], np.array([[13.0, 2.2]], f32)]), [1, 77], LM.R, LM.R, 1)
    c.sim([1], 1)
    assert c.equals(d.feature_stats())
    d.local_end()
    assert c.equals(d.feature_stats()) and d.dim == 3 + 2 * 17 and c.epoch == 4
    gone = [2, 13, 16]
    d.remove(gone)
    c.remove(gone)
    st = d.feature_stats()
    assert c.equals(st) and st["hits"].shape[0] == 14
    if batch_update:
        assert c.hits[1] == 2 and c.last[1] == 4 and c.hits[0] == 1 and c.hits[2] == 1
    else:
        assert c.hits[1] == 1 and c.last[1] == 3 and c.hits[0] == 1 and c.hits[2] == 0  # only the direct updates
    d.upload(x0, P0)
    c.upload(nf)
    assert c.equals(d.feature_stats()) and c.born == [4] * nf
    d.close()


# ---- 5. the contract --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_changes_nothing():
    import slam_amd
    nf = 20
    x0, P0 = LM.synthetic_state(nf, 2)
    d, cap = uploaded(nf, x0, P0, association_known=True)
    d.update(LM.observations(x0, [4, 9], np.random.default_rng(1)), [4, 9], LM.R)

    def snapshot():
        st = d.feature_stats()
        return (d.dim, whole(d, cap).tobytes(), d.state()[0].tobytes(), d.lookup(np.arange(nf + 2)).tobytes(), st["epoch"],
                st["hits"].tobytes(), st["born"].tobytes(), st["last"].tobytes(), d.status())

    def refused(call):
        with pytest.raises(slam_amd.SlamGpuError) as ei:
            call()
        assert ei.value.code == -1, ei.value

    before = snapshot()
    for bad in ([nf], [-1], [3, 3], [4, 1], [0, 1, nf], [0, 2, 2, 5]):
        refused(lambda: d.remove(bad))
    one = np.zeros(1, np.int32)
    assert d.L.slamgpu_ekf_remove(d.h, None, 1) == -1 and d.L.slamgpu_ekf_remove(d.h, one.ctypes.data_as(C.c_void_p), -1) == -1
    assert d.L.slamgpu_ekf_remove(d.h, None, 0) == 0  # k = 0: nothing to read
    assert snapshot() == before
    # a local period open: refused, and the period goes on as if nothing had been asked
    twin, _ = uploaded(nf, x0, P0, association_known=True)
    twin.update(LM.observations(x0, [4, 9], np.random.default_rng(1)), [4, 9], LM.R)
    z = LM.observations(x0, [1, 5], np.random.default_rng(2))
    for f in (d, twin):
        f.local_begin([1, 4, 5, 9], 1)
        f.predict(3.0, float(f32(0.05)), LM.Q, LM.DT)
    refused(lambda: d.remove([1]))
    refused(lambda: d.remove([12]))
    info = d.local_info()
    assert info["open"] == 1 and info["calls"] == 1 and d.dim == 3 + 2 * nf
    for f in (d, twin):
        f.update(z, [1, 5], LM.R)
        f.local_end()
    assert bits_equal(whole(d, cap), whole(twin, cap)) and bits_equal(d.state()[0], twin.state()[0])
    sd, st = d.feature_stats(), twin.feature_stats()
    assert sd["epoch"] == st["epoch"] == 2 and all(np.array_equal(sd[k], st[k]) for k in ("hits", "born", "last")) and sd["hits"][1] == 1
    d.remove([1])  # ... and after the commit it is an ordinary filter again
    assert d.dim == 3 + 2 * (nf - 1)
    d.close()
    twin.close()


def test_remove_does_not_wait_for_the_device():
    """the stream is the caller's and holds milliseconds of copies when remove is called: remove returns with the stream still busy,
    and after slamgpu_ekf_sync the result is the model's.  (A remove that waited would return with the stream idle.)"""
    import slam_amd
    slam_amd.load_library()
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    vp = C.c_void_p
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]
    for fn in (hip.hipStreamSynchronize, hip.hipStreamDestroy, hip.hipFree, hip.hipStreamQuery):
        fn.argtypes = [vp]
    stream, buf = vp(), vp()
    size = 1 << 30
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipMalloc(C.byref(buf), size) == 0
    nf = 130
    x0, P0 = RM.distinct_state(nf)
    d = make_dev(nf, external_stream=stream.value)
    d.upload(x0, P0)
    d.remove([5])  # (the staging buffers are made here, at their largest)
    d.sync()
    assert hip.hipStreamQuery(stream) == 0
    for _ in range(16):  # 16 GiB of device writes: milliseconds
        assert hip.hipMemsetAsync(buf, 0x5A, size, stream) == 0
    d.remove([0, 7, 128])
    busy = hip.hipStreamQuery(stream)
    assert d.dim == 3 + 2 * (nf - 4)  # the host side is done
    d.sync()
    assert busy == 600, busy  # hipErrorNotReady: remove returned before the stream had drained
    x, P = d.state()
    xm, Pm = RM.gather(*RM.gather(x0, P0, [5]), [0, 7, 128])
    assert bits_equal(x, xm) and bits_equal(P, Pm)
    d.close()
    assert hip.hipStreamDestroy(stream) == 0 and hip.hipFree(buf) == 0


# ---- 6. slam-backend --------------------------------------------------------------------------------------------------------------------------
def test_backend_prunes_on_the_device_as_on_the_host():
    """example_loop1, seed 3, -EKF_PRUNE_AGE 10 -EKF_PRUNE_HITS 1: the device path prints the host path's landmarks line and its final
    estimate to four decimals (all that is printed), with -EKF_LOCAL 20 too"""
    def run(*extra):
        r = subprocess.run([EXE, "-m", os.path.join(DATA, "example_loop1.mat"), "-method", "EKF1", "-SWITCH_SEED_RANDOM", "3", "-EKF_PRUNE_AGE", "10",
                            "-EKF_PRUNE_HITS", "1", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]
        return report(r.stdout)
    host = run()
    dev = run("-ekf", "device")
    loc = run("-ekf", "device", "-EKF_LOCAL", "20")
    print("slam-backend pruning: host %s | device %s | device, local periods %s" % (host, dev, loc))
    assert host[1] == "landmarks in map: 22 (0 removed by -EKF_PRUNE_AGE 10 -EKF_PRUNE_HITS 1)"
    assert dev == host and loc == host
