"""The counted instantiations of the update launch (kernels.hip: update_kernel_counted<SPEC, WPAR, M>; kernels.h: update_counted) against
the plain specialised kernels (SLAMGPU_NO_COUNTED=1) and the general one (SLAMGPU_NO_SPECIAL=1), both read when the context is created:
the same operations on the same values, so the whole state and the recorded history agree BIT FOR BIT.  A counted launch has the
packet's number of re-observed landmarks compiled in, keeps their records in registers from their loads through both passes and gets
no staging LDS from the launcher; both record paths are covered (every re-observed landmark fresh: the records are requested with the
pose; otherwise slot first, then record).  FastSLAM 2, Philox, both builds.  The helpers are those of tests/test_gpu_special.py."""
import numpy as np
import pytest

from conftest import sim_args
from test_gpu_special import assert_same, sg, tape_of  # noqa: F401  (sg: fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
K_COUNTED = 8  # kernels.h: kCountedMax
MODES = ("selected", "no_counted", "no_special")
NOBS = 200     # example_webmap: the first 200 observation steps hold every m from 1 to 7
FORCED = 4     # teacher-forced steps behind them and one more step of the tape (M = 8)


def m_of(st):
    return np.asarray(st["zf"]).reshape(-1, 2).shape[0]


def run(sg, monkeypatch, mode, steps, tape, N, every, forced=None, **kw):
    """the steps through slamgpu_step; peek() after every `every`-th step and at the end; then the history and the launch counters.
    forced: a dict that the first run fills with the teacher-forced packets (made from its own state) and the others replay."""
    for name in ("SLAMGPU_NO_COUNTED", "SLAMGPU_NO_SPECIAL"):
        monkeypatch.delenv(name, raising=False)
    if mode != "selected":
        monkeypatch.setenv("SLAMGPU_NO_COUNTED" if mode == "no_counted" else "SLAMGPU_NO_SPECIAL", "1")
    s = sg.SlamGpu(N, tape["nlm"], n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=7, **kw)
    for name in ("SLAMGPU_NO_COUNTED", "SLAMGPU_NO_SPECIAL"):  # (read at creation: the context keeps what it found)
        monkeypatch.delenv(name, raising=False)
    snaps = []
    for k, st in enumerate(steps):
        ctl = np.array(st["controls"], f32).reshape(-1, 3)
        s.step(ctl, tape["Q"], float(tape["dt"]), st["zf"], st["idf"], st["zn"], tape["R"])
        if (k + 1) % every == 0 or k + 1 == len(steps):
            snaps.append(s.peek())
    if forced is not None:
        # (no peek() between these: the launch behind one is a general launch.  The tape's next step as it is, then the forced ones)
        if "packets" not in forced:
            forced["packets"], forced["stale"] = forced_packets(tape["steps"][:len(steps) + 1], tape, snaps[-1])
        st = tape["steps"][len(steps)]
        s.step(np.array(st["controls"], f32).reshape(-1, 3), tape["Q"], float(tape["dt"]), st["zf"], st["idf"], st["zn"], tape["R"])
        for st, (zf, idf) in zip(tape["steps"][len(steps) + 1:], forced["packets"]):
            ctl = np.array(st["controls"], f32).reshape(-1, 3)
            s.step(ctl, tape["Q"], float(tape["dt"]), zf, idf, np.zeros((0, 2), f32), tape["R"])
        snaps.append(s.peek())
    hist = s.history_fetch()
    special, counted = s.special_launches(), s.counted_launches()
    s.close()
    return snaps, hist, special, counted


_map = {}


def webmap_landmarks():
    from slam_amd import host
    if "lm" not in _map:
        sim = host.HostSim(sim_args("example_webmap", "FASTSLAM2", 100, 7))
        _map["lm"] = np.asarray(sim.map()[0], np.float64).T.copy()  # [nlm, 2]
        sim.close()
    return _map["lm"]


def forced_packets(steps, tape, snap):
    """FORCED packets that re-observe eight KNOWN landmarks each: zf is the range and bearing from the tape's true pose to the map's
    landmarks.  Which map landmark a filter index is: the one nearest to the particles' mean of it.  A landmark is fresh in a step when
    the step before observed (or opened) it.  Packets 0 and 1: the same eight landmarks nearest to the vehicle (1: all of them
    fresh: the records come with the pose); 2 and 3: one of them replaced by the known landmark seen longest ago (slot first, then
    record).  Returns the packets and, per packet, whether it holds a landmark that is not fresh."""
    lm = webmap_landmarks()
    nf = snap["nf"]  # (known when the snapshot was taken, a step before the last of `steps`)
    assert nf >= 13, nf
    mean = snap["xf"].astype(np.float64).mean(axis=0)  # [nf, 2]
    d = np.linalg.norm(mean[:, None, :] - lm[None, :, :], axis=2)
    which = d.argmin(axis=1)
    assert len(set(which.tolist())) == nf, which
    last_seen = np.full(tape["nlm"], -1)
    for k, st in enumerate(steps):
        last_seen[np.asarray(st["idf"], np.int64)] = k
        nz = np.asarray(st["zn"]).reshape(-1, 2).shape[0]
        last_seen[st["nf_before"]:st["nf_before"] + nz] = k
    packets, stale = [], []
    now = len(steps)
    for q, st in enumerate(tape["steps"][len(steps):len(steps) + FORCED]):  # (the tape's controls and true poses)
        x, y, phi = (float(v) for v in st["true"])
        if q == 0:
            near = np.argsort(np.hypot(lm[which, 0] - x, lm[which, 1] - y), kind="stable")[:K_COUNTED]
        ids = near
        if q >= 2:  # one of the eight gives way to the known landmark seen longest ago
            old = [j for j in np.argsort(last_seen[:nf], kind="stable") if j not in ids]
            ids = np.concatenate([ids[:K_COUNTED - 1], [old[0]]])
        ids = np.sort(ids)
        dx, dy = lm[which[ids], 0] - x, lm[which[ids], 1] - y
        bearing = np.arctan2(dy, dx) - phi
        bearing = (bearing + np.pi) % (2 * np.pi) - np.pi
        packets.append((np.stack([np.hypot(dx, dy), bearing], axis=1).astype(f32), ids.astype(np.int32)))
        stale.append(bool((last_seen[ids] < now - 1).any()))
        last_seen[ids] = now
        now += 1
    return packets, stale


def three_ways(sg, monkeypatch, steps, tape, N, every, forced=None, **kw):
    runs = {mode: run(sg, monkeypatch, mode, steps, tape, N, every, forced=forced, **kw) for mode in MODES}
    assert_same(runs["selected"], runs["no_counted"])
    assert_same(runs["selected"], runs["no_special"])
    return runs


def check_counters(runs, ms):
    """ms: the packets' numbers of re-observed landmarks, launch by launch"""
    sel, noc, nos = (runs[mode] for mode in MODES)
    print("specialised launches %d / %d / %d, counted %s / %s / %s" % (sel[2], noc[2], nos[2], sel[3], noc[3], nos[3]))
    # neither switch lets a counted kernel run; SLAMGPU_NO_SPECIAL none at all
    assert nos[2] == 0 and not any(nos[3])
    assert not any(noc[3][1:]) and noc[3][0] == noc[2]
    # as selected: the same launches are specialised, and of those every one with 1 <= m <= 8 is counted, for its own m
    assert sel[2] == noc[2] and sum(sel[3]) == sel[2]
    in_range = [m for m in ms if 1 <= m <= K_COUNTED]
    assert sel[3][0] <= len(ms) - len(in_range), (sel[3], len(ms), len(in_range))
    assert sum(sel[3][1:]) == sel[2] - sel[3][0]
    for m in range(1, K_COUNTED + 1):
        assert sel[3][m] <= in_range.count(m), (m, sel[3], in_range.count(m))
    # (general launches: the first of the context and, at most, the one after each peek())
    assert sum(sel[3][1:]) >= len(in_range) - 1 - len(sel[0])


def check_resamples(hist):
    res = np.asarray(hist[2])[:-1]
    print("%d of %d steps resampled" % (int(res.sum()), len(res)))
    assert res.any() and not res.all(), res


@pytest.mark.parametrize("every", [3, 4])
@pytest.mark.parametrize("N", [300, 1024])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_webmap_counted_equals_special_equals_general(sg, monkeypatch, math_mode, N, every):
    """example_webmap, the first 200 observation steps: every m from 1 to 7 with births and resamples among them; 300 particles (two
    tiles, the last wave and tile partial) and 1 024; peek() every 3 and every 4 steps, so both parities see a general launch in between"""
    tape = tape_of("example_webmap", 2, NOBS + 1 + FORCED)
    steps = tape["steps"][:NOBS]
    ms = [m_of(st) for st in steps]
    assert set(range(1, 8)) <= set(ms) and max(ms) < K_COUNTED, sorted(set(ms))
    assert any(np.asarray(st["zn"]).reshape(-1, 2).shape[0] > 0 for st in steps[1:])
    runs = three_ways(sg, monkeypatch, steps, tape, N, every, method=2, math_mode=math_mode)
    check_resamples(runs["selected"][1])
    check_counters(runs, ms)
    assert all(c > 0 for c in runs["selected"][3][1:8]), runs["selected"][3]


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_loop902_counted_equals_special_equals_general(sg, monkeypatch, math_mode):
    """example_loop902, 512 particles, its first 120 observation steps: spec 2 (the heading is observed at every predict)"""
    tape = tape_of("example_loop902", 2, 120)
    conf = tape["conf"]
    assert bool(conf.SWITCH_HEADING_KNOWN)
    kw = dict(method=2, math_mode=math_mode, use_heading=True, wheel_base=float(conf.WHEELBASE), sigma_phi=float(conf.sigmaT))
    runs = three_ways(sg, monkeypatch, tape["steps"], tape, 512, 3, **kw)
    check_resamples(runs["selected"][1])
    check_counters(runs, [m_of(st) for st in tape["steps"]])
    assert sum(runs["selected"][3][1:]) > 0


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_eight_reobserved_landmarks_teacher_forced(sg, monkeypatch, math_mode):
    """M = 8, which no bundled tape reaches: behind the 200 steps and one more of the tape, four steps whose packets re-observe eight
    known landmarks, on both record paths, one of them with a landmark that is not fresh while a resample is pending"""
    tape = tape_of("example_webmap", 2, NOBS + 1 + FORCED)
    assert len(tape["steps"]) == NOBS + 1 + FORCED
    steps = tape["steps"][:NOBS]
    forced = {}
    runs = three_ways(sg, monkeypatch, steps, tape, 300, 4, forced=forced, method=2, math_mode=math_mode)
    assert all(len(idf) == K_COUNTED and len(set(idf.tolist())) == K_COUNTED for _, idf in forced["packets"])
    check_counters(runs, [m_of(st) for st in tape["steps"][:NOBS + 1]] + [K_COUNTED] * FORCED)
    assert runs["selected"][3][K_COUNTED] == FORCED, runs["selected"][3]
    # the resample decided in step k is applied by the launch of step k + 1
    res = np.asarray(runs["selected"][1][2])
    pending = [bool(res[NOBS + q]) for q in range(FORCED)]
    print("forced steps: not fresh %s, resample pending %s" % (forced["stale"], pending))
    assert not forced["stale"][1]  # (the same eight as the step before: the fresh path)
    assert any(s and p for s, p in zip(forced["stale"], pending)), (forced["stale"], pending)
