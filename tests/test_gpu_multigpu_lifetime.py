"""Who frees what in the multi-GPU layer (slamgpu_ctx::mg, multigpu_release): contexts that used the distributed or the sharded entry
points close cleanly in every state their buffers can be in, a later context is unaffected, and a caller's totals buffer stays the
caller's.  2 logical shards of 256 particles on one device, 10 observation steps; every sequence here is a legal one."""
import numpy as np
import pytest

from conftest import sim_args

pytestmark = pytest.mark.gpu
G, SHARD, NOBS = 2, 256, 10
N = G * SHARD


@pytest.fixture(scope="module")
def tape():
    from slam_amd import host
    tp = host.make_tape(sim_args("example_webmap", "FASTSLAM2", N, 7), max_obs=NOBS)
    tp["ctl"] = [np.array(st["controls"], np.float32).reshape(-1, 3) for st in tp["steps"]]
    return tp


def steps(tp):
    return ((tp["ctl"][k], tp["Q"], float(tp["dt"]), st["zf"], st["idf"], st["zn"], tp["R"]) for k, st in enumerate(tp["steps"]))


def usable_context(sg, tp):
    """a fresh single context takes the whole tape and hands out a finite set with weight in it"""
    s = sg.SlamGpu(SHARD, tp["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * SHARD), rng_mode=sg.RNG_PHILOX, seed=3, math_mode=1)
    for a in steps(tp):
        s.step(*a)
    est = s.history_fetch()[0]
    d = s.download()
    s.close()
    assert len(est) == len(tp["steps"]) and np.isfinite(est).all()
    assert all(np.isfinite(d[k]).all() for k in ("xv", "Pv", "w", "xf", "Pf"))
    assert d["nf"] > 0 and float(d["w"].sum(dtype=np.float64)) > 0.0


def dist_run(sg, tp):
    from slam_amd.dist import DistFilter
    f = DistFilter.local(G, SHARD, tp["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * N), seed=9, math_mode=1)
    for a in steps(tp):
        f.step(*a)
    hist = f.history_fetch()
    parts = f.download()
    f.close()
    return hist, {k: np.concatenate([p[k] for p in parts]) for k in ("xv", "Pv", "w", "xf", "Pf")}


def test_distributed_run_closed_and_built_again_is_the_same_run(tape):
    import slam_amd as sg
    h1, d1 = dist_run(sg, tape)
    h2, d2 = dist_run(sg, tape)
    assert len(h1[0]) == len(tape["steps"])
    for a, b in zip(h1, h2):
        assert a.tobytes() == b.tobytes()
    for k in d1:
        assert d1[k].shape == d2[k].shape and d1[k].tobytes() == d2[k].tobytes(), k


def test_exported_never_connected_context_closes(tape):
    import slam_amd as sg
    s = sg.SlamGpu(SHARD, tape["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=9, math_mode=1,
                   first_particle=0, n_particles_global=N)
    assert len(s.dist_export()) > 0  # (allocates the totals tables and the flag words, which the peers would map)
    s.close()
    usable_context(sg, tape)


@pytest.mark.parametrize("resample", [True, False])
def test_sharded_run_with_and_without_the_arrival_pool_closes(tape, resample):
    """resample=True with n_effective = N: every update with observations resamples, offspring cross the shard boundary and the
    first unpack that receives some allocates the arrival pool; resample=False: no plan resamples, nothing is ever unpacked."""
    import slam_amd as sg
    from slam_amd.sharded import GpuEngine, LocalComm, ShardedFilter
    eng = [GpuEngine(g, G, SHARD, tape["nlm"], method=sg.FASTSLAM2, n_effective=N, resample=resample, rng_mode=sg.RNG_PHILOX, seed=9,
                     math_mode=1) for g in range(G)]
    flt = ShardedFilter(eng, LocalComm(eng), G)
    resampled = [bool(flt.step(*a).resampled) for a in steps(tape)]
    est = flt.estimate_fetch()
    moved = flt.exchanged_records
    flt.close()
    assert len(est) == len(tape["steps"]) and np.isfinite(est).all()
    assert (any(resampled) and moved > 0) if resample else (not any(resampled) and moved == 0)
    usable_context(sg, tape)


def test_callers_totals_buffer_outlives_the_context(tape):
    import slam_amd as sg
    owner = sg.SlamGpu(SHARD, tape["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * SHARD), rng_mode=sg.RNG_PHILOX, seed=3, math_mode=1)
    s = sg.SlamGpu(SHARD, tape["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=9, math_mode=1,
                   first_particle=0, n_particles_global=N)
    _, nb = s.shard_block_totals()
    buf = owner.dev_alloc(4 * 3 * nb)  # [w | w2 (| max log-weight)] per block of 256
    s.shard_set_totals_buffer(buf)
    assert s.shard_block_totals()[0] == buf
    a = next(steps(tape))
    s.shard_step(*a)  # (the update launch writes this shard's totals into the caller's buffer)
    s.sync()
    s.close()  # not restored: the context must free its own buffer and leave that one alone
    assert owner.L.slamgpu_dev_free(owner.h, buf) == 0, owner.L.slamgpu_last_error()
    owner.close()
    usable_context(sg, tape)


def test_callers_totals_buffer_handed_back_before_the_context_closes(tape):
    """a caller's buffer, then null: the context's own buffer is the one in use again, and the caller's still takes a copy and a free"""
    import slam_amd as sg
    owner = sg.SlamGpu(SHARD, tape["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * SHARD), rng_mode=sg.RNG_PHILOX, seed=3, math_mode=1)
    s = sg.SlamGpu(SHARD, tape["nlm"], method=sg.FASTSLAM2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=9, math_mode=1,
                   first_particle=0, n_particles_global=N)
    own, nb = s.shard_block_totals()
    buf, other = owner.dev_alloc(4 * 3 * nb), owner.dev_alloc(4 * 3 * nb)
    assert own not in (buf, other)
    s.shard_set_totals_buffer(buf)
    assert s.shard_block_totals()[0] == buf
    s.shard_step(*next(steps(tape)))
    s.sync()
    s.shard_set_totals_buffer(None)
    assert s.shard_block_totals()[0] == own
    s.close()
    owner.dev_copy(other, buf, 4 * 3 * nb)
    for p in (buf, other):
        assert owner.L.slamgpu_dev_free(owner.h, p) == 0, owner.L.slamgpu_last_error()
    owner.close()
    usable_context(sg, tape)
