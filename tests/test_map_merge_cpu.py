"""From the posterior map's slot table to a landmark table, on the host (include/slamhost.h: slamhost_map_candidates, slamhost_map_merge,
through slam_amd/host.py), on hand-made summaries; and the declaration / binding of slamgpu_map_pairs, whose joint shares the merge reads.
No GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f64 = np.float64


def _slot(share, x, y, scatter=(0.01, 0.002, 0.02), pf=(0.003, 0.0005, 0.004)):
    return [share, x, y, *scatter, *pf]


def _joint(*shares):
    j = np.full((len(shares), 9), np.nan)
    j[:, 0] = shares
    return j


def test_map_pairs_is_declared_exported_and_bound():
    import slam_amd
    from slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    assert re.search(r"int slamgpu_map_pairs\(slamgpu_ctx \*ctx, const int32_t \*pairs, int32_t count, double \*out, int32_t \*both\);", hdr)
    assert hdr.index("int slamgpu_map_summary(") < hdr.index("int slamgpu_map_pairs(") < hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # an addition to the stable part: the version stays
    L = slam_amd.load_library()
    assert "slamgpu_map_pairs" in slam_amd.DECLARED_SYMBOLS and hasattr(L, "slamgpu_map_pairs")
    assert L.slamgpu_map_pairs.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert callable(getattr(capi.SlamGpu, "map_pairs", None))
    pairs, out, both = np.zeros((2, 2), np.int32), np.zeros((2, 9), f64), np.zeros(2, np.int32)
    assert L.slamgpu_map_pairs(None, pairs.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p), both.ctypes.data_as(C.c_void_p)) < 0


def test_merge_is_declared_and_exported():
    from slam_amd import host
    hdr = open(os.path.join(ROOT, "include", "slamhost.h")).read()
    assert re.search(r"int slamhost_map_merge\(const double \*summary, int32_t slots, const int32_t \*pairs, const double \*joint, int32_t npairs,\s+"
                     r"double radius,\s+double cohold, int32_t \*cluster /\*\[slots\]\*/, double \*merged /\*\[slots\]\[9\]\*/, int32_t \*nmerged\);", hdr)
    assert "exact for clusters of two" in hdr
    L = host.load_library()
    for name in ("slamhost_map_merge", "slamhost_map_candidates"):
        assert name in host.DECLARED_SYMBOLS and hasattr(L, name), name


def test_two_alternatives_become_one_landmark():
    from slam_amd import host
    t = np.array([_slot(0.6, 10.0, 5.0), _slot(0.4, 10.5, 5.0)])
    pairs = host.map_candidates(t, 1.0)
    assert pairs.tolist() == [[0, 1]]
    m = host.map_merge(t, pairs, _joint(0.0), radius=1.0, cohold=0.1)
    assert m["cluster"].tolist() == [0, 0] and len(m["merged"]) == 1
    assert m["share"][0] == 1.0
    np.testing.assert_allclose(m["mean"][0], [0.6 * 10.0 + 0.4 * 10.5, 5.0], rtol=0, atol=1e-14)
    # the spread includes the 0.5 m between the two records: 0.6 * 0.2^2 + 0.4 * 0.3^2 = 0.06 m^2 on top of the slots' own xx
    np.testing.assert_allclose(m["scatter"][0], [0.01 + 0.06, 0.002, 0.02], rtol=0, atol=1e-14)
    np.testing.assert_allclose(m["pf"][0], [0.003, 0.0005, 0.004], rtol=0, atol=1e-16)
    # dict input, as SlamGpu.map_summary / map_pairs return it
    d = dict(share=t[:, 0], mean=t[:, 1:3], scatter=t[:, 3:6], pf=t[:, 6:9])
    j = _joint(0.0)
    m2 = host.map_merge(d, pairs, dict(share=j[:, 0], mean=j[:, 1:3], scatter=j[:, 3:6], pf=j[:, 6:9]))
    assert m2["merged"].tobytes() == m["merged"].tobytes()


def test_held_together_or_far_apart_is_not_merged():
    from slam_amd import host
    t = np.array([_slot(0.6, 10.0, 5.0), _slot(0.4, 10.5, 5.0)])
    m = host.map_merge(t, [[0, 1]], _joint(0.4), radius=1.0, cohold=0.1)   # every holder of the second holds the first: neighbours
    assert m["cluster"].tolist() == [0, 1] and m["merged"].tobytes() == t.tobytes()
    # the threshold itself: s_ab <= cohold * min(s_a, s_b) merges, anything above does not
    assert host.map_merge(t, [[0, 1]], _joint(0.1 * 0.4), 1.0, 0.1)["cluster"].tolist() == [0, 0]
    assert host.map_merge(t, [[0, 1]], _joint(np.nextafter(0.1 * 0.4, 1.0)), 1.0, 0.1)["cluster"].tolist() == [0, 1]
    assert host.map_merge(t, [[0, 1]], _joint(np.nan), 1.0, 0.1)["cluster"].tolist() == [0, 1]
    far = np.array([_slot(0.6, 10.0, 5.0), _slot(0.4, 11.5, 5.0)])
    assert len(host.map_candidates(far, 1.0)) == 0
    m = host.map_merge(far, [[0, 1]], _joint(0.0), radius=1.0, cohold=0.1)   # (a pair the caller gives is still held to the radius)
    assert m["cluster"].tolist() == [0, 1] and m["merged"].tobytes() == far.tobytes()
    assert host.map_merge(far, [[0, 1]], _joint(0.0), radius=2.0, cohold=0.1)["cluster"].tolist() == [0, 0]


def test_chain_merges_by_single_linkage_and_the_share_is_clamped():
    from slam_amd import host
    # A - B - C, 0.8 m apart each: A and C are 1.6 m apart and still one cluster
    t = np.array([_slot(0.5, 0.0, 0.0), _slot(0.3, 0.8, 0.0), _slot(0.2, 1.6, 0.0)])
    pairs = host.map_candidates(t, 1.0)
    assert pairs.tolist() == [[0, 1], [1, 2]]
    m = host.map_merge(t, pairs, _joint(0.01, 0.02), 1.0, 0.1)
    assert m["cluster"].tolist() == [0, 0, 0] and len(m["merged"]) == 1
    np.testing.assert_allclose(m["share"][0], 1.0 - 0.03, rtol=0, atol=1e-15)
    S = 1.0
    mean = (0.5 * 0.0 + 0.3 * 0.8 + 0.2 * 1.6) / S
    np.testing.assert_allclose(m["mean"][0], [mean, 0.0], rtol=0, atol=1e-15)
    xx = (0.5 * (0.01 + mean ** 2) + 0.3 * (0.01 + (0.8 - mean) ** 2) + 0.2 * (0.01 + (1.6 - mean) ** 2)) / S
    np.testing.assert_allclose(m["scatter"][0], [xx, 0.002, 0.02], rtol=0, atol=1e-15)
    # a pair given twice (and the other way round) counts once; a pair across the cluster that does not link still counts inside it
    m = host.map_merge(t, [[0, 1], [1, 0], [1, 2], [0, 2]], _joint(0.01, 0.01, 0.02, 0.04), 1.0, 0.1)
    np.testing.assert_allclose(m["share"][0], 1.0 - 0.07, rtol=0, atol=1e-15)
    # the clamp from above: shares that add up to more than 1
    u = np.array([_slot(0.7, 0.0, 0.0), _slot(0.6, 0.5, 0.0)])
    assert host.map_merge(u, [[0, 1]], _joint(0.0), 1.0, 0.1)["share"][0] == 1.0
    # ... and from below: joint shares inside the cluster that would take it below its largest member (not a linking pair's: A - C)
    v = host.map_merge(t, [[0, 1], [1, 2], [0, 2]], _joint(0.0, 0.0, 0.9), 1.0, 0.1)
    assert v["cluster"].tolist() == [0, 0, 0] and v["share"][0] == 0.5


def test_share_zero_singletons_and_numbering():
    from slam_amd import host
    rng = np.random.default_rng(2)
    t = np.array([_slot(0.9, 50.0, 50.0, rng.random(3), rng.random(3)),      # 0: alone
                  _slot(0.0, np.nan, np.nan, [np.nan] * 3, [np.nan] * 3),    # 1: nobody holds it
                  _slot(0.55, 3.0, 3.0, rng.random(3), rng.random(3)),       # 2: merges with 5
                  _slot(1.0 / 3.0, -7.0, 2.0, rng.random(3), rng.random(3)),  # 3: alone
                  _slot(0.0, np.nan, np.nan, [np.nan] * 3, [np.nan] * 3),    # 4
                  _slot(0.45, 3.2, 3.1, rng.random(3), rng.random(3)),       # 5
                  _slot(0.125, 3.1, 3.0, rng.random(3), rng.random(3))])     # 6: near 2 and 5, held together with both: alone
    pairs = host.map_candidates(t, 1.0)
    assert pairs.tolist() == [[2, 5], [2, 6], [5, 6]]
    m = host.map_merge(t, pairs, _joint(0.0, 0.125, 0.1), 1.0, 0.1)
    assert m["cluster"].tolist() == [0, -1, 1, 2, -1, 1, 3]      # ascending by the cluster's lowest slot; share 0: -1 and no row
    assert len(m["merged"]) == 4
    for slot, c in ((0, 0), (3, 2), (6, 3)):                       # singletons: the slot's nine numbers, bit for bit
        assert m["merged"][c].tobytes() == t[slot].tobytes(), slot
    assert m["share"][1] == 1.0
    # no pairs at all: every held slot a landmark of its own
    m = host.map_merge(t, np.zeros((0, 2), np.int32), np.zeros((0, 9)), 1.0, 0.1)
    assert m["cluster"].tolist() == [0, -1, 1, 2, -1, 3, 4] and m["merged"].tobytes() == t[[0, 2, 3, 5, 6]].tobytes()
    # no slots at all
    m = host.map_merge(np.zeros((0, 9)), np.zeros((0, 2), np.int32), np.zeros((0, 9)), 1.0, 0.1)
    assert len(m["cluster"]) == 0 and len(m["merged"]) == 0
    # a pair outside the table is refused
    try:
        host.map_merge(t, [[0, 7]], _joint(0.0), 1.0, 0.1)
    except ValueError:
        pass
    else:
        raise AssertionError("slot 7 of 7 was accepted")


def test_candidates_equal_the_brute_force_list():
    from slam_amd import host
    rng = np.random.default_rng(11)
    n = 2000
    t = np.zeros((n, 9))
    t[:, 0] = rng.random(n)
    t[:, 1] = rng.uniform(-40.0, 40.0, n)
    t[:, 2] = rng.uniform(1e3 - 25.0, 1e3 + 25.0, n)
    dead = rng.choice(n, 150, replace=False)
    t[dead, 0] = 0.0
    t[dead, 1:] = np.nan
    for radius in (1.0, 0.37, 5.0):
        got = host.map_candidates(t, radius)
        dx, dy = t[:, None, 1] - t[None, :, 1], t[:, None, 2] - t[None, :, 2]
        with np.errstate(invalid="ignore"):
            ok = (dx * dx + dy * dy < radius * radius) & (t[:, None, 0] > 0) & (t[None, :, 0] > 0)
        a, b = np.nonzero(np.triu(ok, 1))
        exp = np.stack([a, b], axis=1).astype(np.int32)
        assert len(exp) > 50, "the case would pass vacuously"
        assert got.dtype == np.int32 and np.array_equal(got, exp), radius
    assert len(host.map_candidates(t, 0.0)) == 0 and len(host.map_candidates(np.zeros((0, 9)), 1.0)) == 0
