"""Innovation posterior with every particle's own match (slamgpu_innovation_summary_labels; the ring entries slamgpu_update_particle and
slamgpu_update_labels record by themselves): innovation_summary_kernel<true>, the per-particle-label form of the known-association kernel.

Yardsticks: (a) the known-association call itself -- with unanimous labels the new call must return its bits; (b) the float64 model
tests/innovation_labels_model.py (innovation_model with the slot taken per particle) on peek() of the same context taken immediately
before, within innovation_model.bounds -- the bounds of tests/test_gpu_innovation.py, computed from the model's own terms: the per-term
formula, the weights and the order of merging are the same, so no constant is added; holders exactly, NaN exactly where the model says
NaN; (c) for the ring, the synchronous call made with the step's final labels on a twin context at the same moment, bit for bit, and that
twin (ring off) for the filter's own state.  Every check prints its worst error / bound ratio before it asserts."""
import ctypes as C

import numpy as np
import pytest

import innovation_labels_model as ilm
import innovation_model as im
from test_gpu_innovation import KBLOCK, R0, TILE, _cloud, _compare
from test_gpu_particle_device import EXCL_ON, ERR_CAPACITY, ERR_INVALID, _course, _ctx, _host_step, _opt, _same_state

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NEW, DISCARD = ilm.NEW, ilm.DISCARD
STATE = ("xv", "Pv", "w", "xf", "Pf")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _same_bits(a, b, what):
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), what


# ---- 1. unanimous labels are the known path, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("N", [KBLOCK - 1, KBLOCK + 1, TILE + 1])
def test_unanimous_labels_are_the_known_call(sg, N, mm):
    """uploaded clouds (uneven weights with zeros), nz = 1, 8, 9 (less than a group of observations, one group, one more): the new call with
    labels[i][q] = idf[q] returns slamgpu_innovation_summary's bits; again under the pending gather of an update that resampled, and
    after download() has settled it"""
    xv, w, xf, Pf, zf = _cloud(N)
    s = sg.SlamGpu(N, 4, method=2, n_effective=N, rng_mode=sg.RNG_PHILOX, seed=2, math_mode=mm, particle_maps=True)
    d = s.download()
    d.update(nf=3, xv=xv, w=w, xf=xf, Pf=Pf, Pv=np.tile(np.diag([1e-3, 1e-3, 1e-4]).astype(f32), (N, 1, 1)))
    s.upload(d)

    def both(tag):
        for nz in (1, 8, 9):
            idf = (np.arange(nz) % 3).astype(np.int32)[::-1].copy()
            z = np.resize(zf, (nz, 2)).astype(f32)
            known = s.innovation_summary(z, idf, R0)
            mine = s.innovation_summary_labels(z, np.tile(idf, (N, 1)), R0)
            _same_bits(mine, known, "unanimous labels, N %d nz %d %s: not the known call's bits" % (N, nz, tag))
            assert np.all(known[1] == N) and np.isfinite(known[0]).all()
        return known
    a = both("as uploaded")
    s.update(zf, np.arange(3, dtype=np.int32), np.zeros((0, 2), f32), R0)
    s.estimate_async()
    assert s.stats()[1], ("the update did not resample: no gather is pending", s.stats(), s.status())
    b = both("under the pending gather")
    assert a[0].tobytes() != b[0].tobytes(), "the update changed nothing"
    s.download()
    c = both("after download")
    _same_bits(b, c, "pending and settled: different bits")
    s.close()


# ---- 2. / 3. mixed labels against the float64 model; chunks; position independence ------------------------------------------------------
def _mixed(sg, logw, mm):
    """TILE + 1 particles after 13 real per-particle steps of example_webmap, records punched out of three slots (each in another seventh
    of the particles), one more real step (the slots it touches move to a new genealogy row, and it resamples or not as it likes), the
    next step's predicts applied, and 9 observations with labels that differ from lane to lane: any slot, NEW, DISCARD, one observation
    nobody matched, the same slot under two observations of one particle, and a slot h named by the particles that hold it absent.
    Returns the context, the course, z, labels, who lacks h, h, the rows in use"""
    N, nz = TILE + 1, 9
    c = _course("FASTSLAM2", 16)
    s = _ctx(sg, c, N, 2, mm, logw=logw)
    opt = _opt(EXCL_ON, 1, 0.02)
    for k in range(13):
        _host_step(s, c, k, opt)
    d = s.download()
    assert d["nf"] >= 4
    for j, l in enumerate((0, d["nf"] // 2, d["nf"] - 1)):
        d["xf"][3 + j::7, l] = np.nan
        d["Pf"][3 + j::7, l] = np.nan
    s.upload(d)
    _host_step(s, c, 13, opt)
    for V, G, phi in c["ctl"][14]:
        s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
    o = s.observe(c["xt"][14], c["max_range"], c["R"], noise=2)
    assert len(o["z"]) >= 2
    z = np.resize(np.asarray(o["z"], f32), (nz, 2))
    nf = s.nf()
    absent = np.isnan(s.peek()["xf"][:, :, 0])      # (the step since has decided whose descendants lack what)
    count = absent.sum(axis=0)
    h = int(np.argmax(np.where(count < N, count, 0)))   # (what survives of the punched slots, or a slot the run itself left partial)
    assert 0 < count[h] < N, ("no slot is held by some particles and absent in others", count.tolist())
    holes = absent[:, h]
    rows = s.genealogy_rows()[0]
    assert rows >= 2, "every slot lies in one genealogy row"
    rng = np.random.default_rng(5)
    lab = rng.integers(0, nf, (N, nz)).astype(np.int32)
    u = rng.uniform(size=(N, nz))
    lab[u < 0.15] = NEW
    lab[(u >= 0.15) & (u < 0.3)] = DISCARD
    lab[:, 4] = np.where(np.arange(N) % 2 == 0, NEW, DISCARD)          # nobody matched observation 4
    lab[::3, 1] = lab[::3, 0]                                          # one slot under two observations of one particle
    lab[:, 2] = h                                                      # a slot some particles hold absent, named by everybody
    assert ((lab[:, 0] >= 0) & (lab[:, 1] == lab[:, 0])).sum() > 100 and (np.diff(lab[:, 0]) != 0).sum() > N // 2
    return s, c, z, lab, holes, h, rows


@pytest.mark.parametrize("logw,mm", [(False, 1), (True, 1), (False, 0)], ids=["linear_fast", "log_fast", "linear_strict"])
def test_mixed_labels_against_the_model(sg, monkeypatch, logw, mm):
    s, c, z, lab, holes, h, rows = _mixed(sg, logw, mm)
    N = s.N
    pk = s.peek()
    assert np.isnan(pk["xf"][holes, h]).all() and not np.isnan(pk["xf"][~holes, h]).any()
    monkeypatch.setenv("SLAMGPU_INNOV_CHUNK", "8")
    got, holders = s.innovation_summary_labels(z, lab, c["R"])
    monkeypatch.delenv("SLAMGPU_INNOV_CHUNK")
    whole = s.innovation_summary_labels(z, lab, c["R"])
    _same_bits((got, holders), whole, "the observations in chunks of 8: different bits")
    exp, eh, terms = ilm.summary_labels(pk["xv"], pk["w"], pk["xf"], pk["Pf"], z, lab, c["R"], logw)
    print("mixed labels: %d slots in %d genealogy rows; slot %d absent in %d particles; holders %s" % (s.nf(), rows, h, int(holes.sum()), eh.tolist()))
    _compare(got, holders, exp, eh, im.bounds(terms, N, exp), "labels, mixed, %s weights math%d N %d" % ("log" if logw else "linear", mm, N))
    assert eh[4] == 0 and got[4, 0] == 0.0 and np.isnan(got[4, 1:]).all()
    assert eh[2] == N - holes.sum() and np.all(eh[[0, 1, 3, 5, 6, 7, 8]] > N // 3)
    # the absent slot named by the particles that lack it adds nobody: the same entry with those labels DISCARD
    lab2 = lab.copy()
    lab2[holes, 2] = DISCARD
    again = s.innovation_summary_labels(z, lab2, c["R"])
    assert again[0][2].tobytes() == got[2].tobytes() and again[1][2] == holders[2]
    # read-only: the set peek shows is the one it showed
    pk1 = s.peek()
    for k in STATE:
        assert np.array_equal(pk[k], pk1[k], equal_nan=True), k
    s.close()


def test_position_independence(sg):
    """the observations permuted, the label columns alike: the entries permuted, bit for bit; a column's entry does not depend on the
    other columns either"""
    s, c, z, lab, holes, h, rows = _mixed(sg, False, 1)
    base = s.innovation_summary_labels(z, lab, c["R"])
    perm = np.random.default_rng(9).permutation(len(z))
    assert not np.array_equal(perm, np.arange(len(z)))
    moved = s.innovation_summary_labels(z[perm], np.ascontiguousarray(lab[:, perm]), c["R"])
    _same_bits(moved, (base[0][perm], base[1][perm]), "an observation's bits depend on its place")
    alone = s.innovation_summary_labels(z[5:6], np.ascontiguousarray(lab[:, 5:6]), c["R"])
    _same_bits(alone, (base[0][5:6], base[1][5:6]), "an observation's bits depend on what else is asked")
    s.close()


# ---- 4. the ring ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gates", "sampling", "labels"])
def test_ring_of_the_per_particle_step(sg, kind):
    """N = 512 on example_webmap, gates of the .ini (4 / 25), 12 observation steps.  gates: exclusion rule, spacing cap and mutual
    exclusion on, slamgpu_update_particle; sampling: data association sampling on; labels: slamgpu_update_labels with the labels a third
    context's slamgpu_update_particle made, every fifth particle's matches turned into DISCARD.  r has the ring on, t is its twin with the ring off.  Per step: peek of r before the step,
    the labels slamgpu_particle_labels returns after it, t's synchronous call with those labels BEFORE t's own step.  The ring's entries
    are t's synchronous entries bit for bit, match the model within its bounds, carry the tags (record, -3); t's poses, weights, records,
    labels, reports, history entry and ancestors are r's after every step, and so is the downloaded state at the end"""
    N, steps = 512, 12
    c = _course("FASTSLAM2", 16)
    opt = _opt(EXCL_ON, 1, 0.02)
    lopt = dict(new_share=opt["new_share"], p_new=opt["p_new"], census_every=opt["census_every"])

    def make():
        s = _ctx(sg, c, N, 2, 1)
        if kind == "gates":
            s.set_particle_excl_spacing(0.5)
            s.set_particle_mutex(1)
        if kind == "sampling":
            s.set_particle_assoc_sampling(True)
        return s
    r, t = make(), make()
    src = make() if kind == "labels" else None
    r.innovation_history_enable(4096)
    sync, holds, exps, ehs, bnds, tags = [], [], [], [], [], []
    seen_resample = False
    for k in range(steps):
        zs = []
        for s in (r, t) + ((src,) if src else ()):
            for V, G, phi in c["ctl"][k]:
                s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
            zs.append(np.asarray(s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)["z"], f32).reshape(-1, 2))
        z = zs[0]
        assert all(np.array_equal(z, y) for y in zs[1:])
        if len(z):
            pk = r.peek()
            if src:
                src.update_particle(z, c["R"], **opt)
                lab = src.particle_labels()
                lab[2::5][lab[2::5] >= 0] = DISCARD   # (every fifth particle gives its matches up: shares strictly between 0 and 1)
                rep_r = r.update_labels(z, c["R"], lab, **lopt)
            else:
                rep_r = r.update_particle(z, c["R"], **opt)
                lab = r.particle_labels()
            assert lab.shape == (N, len(z)) and np.array_equal(r.particle_labels(), lab)
            out, hold = t.innovation_summary_labels(z, lab, c["R"])
            rep_t = t.update_labels(z, c["R"], lab, **lopt) if src else t.update_particle(z, c["R"], **opt)
            assert rep_r == rep_t, (k, rep_r, rep_t)
            assert np.array_equal(t.particle_labels(), lab), "step %d: the twin's labels differ" % k
            exp, eh, terms = ilm.summary_labels(pk["xv"], pk["w"], pk["xf"], pk["Pf"], z, lab, c["R"], False)
            sync.append(out), holds.append(hold), exps.append(exp), ehs.append(eh), bnds.append(im.bounds(terms, N, exp))
            tags += [(len(sync) - 1, ilm.SLOT_PER_PARTICLE)] * len(z)
        for s in (r, t) + ((src,) if src else ()):
            s.estimate_async()
        a, b = r.peek(), t.peek()
        assert a["nf"] == b["nf"]
        for key in STATE:
            assert np.array_equal(a[key], b[key], equal_nan=True), "step %d: %s differs between ring on and off" % (k, key)
        assert np.array_equal(r.ancestors(), t.ancestors()), "step %d: ancestors differ" % k
        hr, ht = r.history_fetch(), t.history_fetch()   # (this step's entry: estimate, Neff, decision)
        assert len(hr[0]) == 1
        for x, y in zip(hr, ht):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), "step %d: history differs between ring on and off" % k
        seen_resample = seen_resample or bool(np.any(hr[2]))
    sync, holds, exps, ehs, bnds = (np.concatenate(x) for x in (sync, holds, exps, ehs, bnds))
    first, nxt, cap, rec = r.innovation_history_info()
    assert (first, nxt, cap, rec) == (0, len(sync), 4096, tags[-1][0] + 1) and t.innovation_history_info() == (0, 0, 0, 0)
    ring, record, slot = r.innovation_history_fetch()
    assert ring.shape == sync.shape and ring.tobytes() == sync.tobytes(), "ring entries differ from the synchronous call's"
    assert [(int(x), int(y)) for x, y in zip(record, slot)] == tags
    _compare(ring, holds, exps, ehs, bnds, "labels, ring (%s) N %d" % (kind, N))
    matched = ehs > 0
    print("ring (%s): %d entries, %d with holders, %d with every particle; mean share %.4f" %
          (kind, len(ehs), int(matched.sum()), int((ehs == N).sum()), float(np.nanmean(ring[:, 0]))))
    assert matched.sum() >= 10 and (~matched).sum() >= 1, "the run holds no matched observation, or no unmatched one"
    if kind == "labels":
        # (where the step before did not resample, those who gave their matches up weigh next to nothing: a share that rounds to 1)
        assert ((ehs > 0) & (ehs < N)).sum() >= 10 and (ring[matched, 0] < 1.0).sum() >= 10, "no entry with a share strictly between 0 and 1"
    assert np.all(ring[~matched, 0] == 0.0) and np.isnan(ring[~matched, 1:]).all()
    assert seen_resample, "no step of the run resampled"
    _same_state((r.history_fetch(), r.download()), (t.history_fetch(), t.download()), "ring on / off (%s)" % kind)
    for s in (r, t) + ((src,) if src else ()):
        s.close()


# ---- 5. refusals and launch counts --------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(sg):
    vp = C.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    N = 300
    out, hold = np.full((3, 10), -1.0), np.full(3, -1, np.int32)
    xv, w, xf, Pf, zf = _cloud(N)
    good = np.tile(np.array([0, 1, 2], np.int32), (N, 1))
    s = sg.SlamGpu(N, 4, method=2, rng_mode=sg.RNG_PHILOX, seed=2, particle_maps=True)
    d = s.download()
    d.update(nf=3, xv=xv, w=w, xf=xf, Pf=Pf)
    s.upload(d)
    L = s.L
    call = lambda ctx, z, nz, lab, R, o, h: ctx.L.slamgpu_innovation_summary_labels(ctx.h, p(z), nz, p(lab), p(R), p(o), p(h))
    for bad_label in (3, -3, 1 << 30, -(1 << 31)):   # nf, one below DISCARD, far outside either way
        bad = good.copy()
        bad[N - 1, 2] = bad_label
        assert call(s, zf, 3, bad, R0, out, hold) == ERR_INVALID, bad_label
        assert b"label" in L.slamgpu_last_error()
    assert call(s, zf, -1, good, R0, out, hold) == ERR_INVALID
    for a in ((None, good, R0, out), (zf, None, R0, out), (zf, good, None, out), (zf, good, R0, None)):
        assert call(s, a[0], 3, a[1], a[2], a[3], hold) == ERR_INVALID
    assert call(s, None, 0, None, None, None, None) == 0   # nz == 0 does nothing
    plain = sg.SlamGpu(N, 35, method=2, rng_mode=sg.RNG_PHILOX)
    assert call(plain, zf, 3, np.zeros((N, 3), np.int32), R0, out, hold) == ERR_INVALID and b"SLAMGPU_FLAG_PARTICLE_MAPS" in plain.L.slamgpu_last_error()
    plain.close()
    shard = sg.SlamGpu(256, 35, method=2, rng_mode=sg.RNG_PHILOX, n_particles_global=512, first_particle=0)
    assert call(shard, zf, 3, np.zeros((256, 3), np.int32), R0, out, hold) == ERR_INVALID and b"single contexts only" in shard.L.slamgpu_last_error()
    shard.close()
    assert np.all(out == -1.0) and np.all(hold == -1)
    # NEW and DISCARD are labels like any other, holders may be NULL
    lab = good.copy()
    lab[::2, 0] = NEW
    lab[1::2, 0] = DISCARD
    assert call(s, zf, 3, lab, R0, out, None) == 0 and out[0, 0] == 0.0 and np.isnan(out[0, 1:]).all() and np.isfinite(out[1:]).all()
    s.close()


def test_capacity_refusal_and_launch_counts(sg):
    """with the ring never enabled: no launch of the new kernel (nor of the finishing pass).  A step of more observations than the ring
    holds: SLAMGPU_ERR_CAPACITY, nothing recorded, and the context as it was -- the same step, made again once the ring is large
    enough, equals the twin's in report and state, and is the first launch of the new kernel"""
    N = 512
    c = _course("FASTSLAM2", 16)
    opt = _opt(EXCL_ON, 1, 0.02)
    a, b = _ctx(sg, c, N, 2, 1), _ctx(sg, c, N, 2, 1)
    for s in (a, b):
        s.profile(True)
    refused = False
    for k in range(16):
        zs = []
        for s in (a, b):
            for V, G, phi in c["ctl"][k]:
                s.predict(float(V), float(G), c["Q"], c["dt"], float(phi))
            zs.append(np.asarray(s.observe(c["xt"][k], c["max_range"], c["R"], noise=2)["z"], f32).reshape(-1, 2))
        z = zs[0]
        assert np.array_equal(z, zs[1])
        if k >= 6 and len(z) >= 2:
            for s in (a, b):
                for name in ("innovation_summary_labels", "innovation_summary", "innovation_finish"):
                    assert s.kernel_time(name)[1] == 0, name
                assert s.innovation_history_info() == (0, 0, 0, 0)
            a.innovation_history_enable(len(z) - 1)
            lab0 = a.particle_labels()
            with pytest.raises(sg.SlamGpuError) as e:
                a.update_particle(z, c["R"], **opt)
            assert e.value.code == ERR_CAPACITY and a.innovation_history_info() == (0, 0, len(z) - 1, 0)
            with pytest.raises(sg.SlamGpuError) as e:
                a.update_labels(z, c["R"], np.full((N, len(z)), DISCARD, np.int32), new_share=0.02, p_new=0.05, census_every=1)
            assert e.value.code == ERR_CAPACITY and a.innovation_history_info() == (0, 0, len(z) - 1, 0)
            assert np.array_equal(a.particle_labels(), lab0) and a.kernel_time("innovation_summary_labels")[1] == 0
            a.innovation_history_enable(len(z))
            ra, rb = a.update_particle(z, c["R"], **opt), b.update_particle(z, c["R"], **opt)
            assert ra == rb, (ra, rb)
            assert a.innovation_history_info() == (0, len(z), len(z), 1)
            assert a.kernel_time("innovation_summary_labels")[1] == 1 and a.kernel_time("innovation_finish")[1] == 1 and a.kernel_time("innovation_summary")[1] == 0
            assert b.kernel_time("innovation_summary_labels")[1] == 0 and b.kernel_time("innovation_finish")[1] == 0
            a.update_particle(np.zeros((0, 2), f32), c["R"], **opt)   # no observation: a record without entries
            assert a.innovation_history_info() == (0, len(z), len(z), 2)
            refused = True
        elif len(z):
            assert a.update_particle(z, c["R"], **opt) == b.update_particle(z, c["R"], **opt)
        for s in (a, b):
            s.estimate_async()
        if refused:
            break
    assert refused, "no step from the sixth on had two observations"
    assert np.array_equal(a.particle_labels(), b.particle_labels()) and np.array_equal(a.ancestors(), b.ancestors())
    _same_state((a.history_fetch(), a.download()), (b.history_fetch(), b.download()), "after the refused step")
    a.close()
    b.close()
