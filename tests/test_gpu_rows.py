"""The genealogy row book (slam_amd/csrc/rows.h) through every writer it has, one after the other, in ONE context: host-made packets
(slamgpu_step), the device front end (slamgpu_step_observe), the per-particle update driven by the host (slamgpu_update_particle) and by
the device (slamgpu_run_particle, K = 3), a download (flatten), an upload, host-made packets again.  Between two writers the tables
change hands (book_push / book_pull, pp_push / pp_pull, sync_tables).  A twin context takes the same steps through the host-driven
entry points only (slamgpu_observe + slamgpu_step, slamgpu_observe + slamgpu_update_particle); after every segment rows in use,
landmark count, history and state are the same, bit for bit.  tests/test_gpu_observe.py and tests/test_gpu_particle_device.py hold
such twins pairwise; this one chains the hand-overs.  Plain rows held near 6 by consolidation (SLAMGPU_PLAIN_ROWS_TARGET=6), one
block of 256 particles."""
import numpy as np
import pytest

from conftest import bits_equal, sim_args

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 256
SEG = dict(packets=600, front=10, particle=1, device=3, again=10)
OPT = dict(gate_reject=4.0, gate_augment=25.0, mode=0, new_share=0.02, p_new=0.05, census_every=1)


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


def _course(steps):
    from slam_amd import host
    args = sim_args("example_webmap", "FASTSLAM2", 100, 7)
    tape = host.make_tape(args, max_obs=steps)
    sim = host.HostSim(args)
    lm, _ = sim.map()
    max_range = float(sim.conf.MAX_RANGE)
    sim.close()
    return dict(ctl=[np.array(st["controls"], f32).reshape(-1, 3) for st in tape["steps"]], xt=[np.asarray(st["true"], f32) for st in tape["steps"]],
                lm=lm, max_range=max_range, Q=tape["Q"], R=tape["R"], dt=float(tape["dt"]), nlm=tape["nlm"])


def _same(a, b, what):
    """rows in use, landmark count, history, state (NaN = absent): the same bits; the download flattens both"""
    ra, rb = a.genealogy_rows(), b.genealogy_rows()
    assert ra[0] <= ra[1] and rb[0] <= rb[1], (what, ra, rb)
    assert a.live_rows() == b.live_rows(), (what, a.live_rows(), b.live_rows())
    assert a.nf() == b.nf(), (what, a.nf(), b.nf())
    for x, y in zip(a.history_fetch(), b.history_fetch()):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), what
    da, db = a.download(), b.download()
    assert da["nf"] == db["nf"], (what, da["nf"], db["nf"])
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        assert bits_equal(da[k], db[k]), (what, k)
    return ra[0], da


def test_row_book_through_every_writer(sg, monkeypatch):
    monkeypatch.setenv("SLAMGPU_PLAIN_ROWS_TARGET", "6")
    c = _course(sum(SEG.values()))
    Q, R, dt, mr = c["Q"], c["R"], c["dt"], c["max_range"]
    a, b = (sg.SlamGpu(N, c["nlm"] * 4, method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=5, math_mode=1, device_observe=True,
                       particle_maps=True) for _ in range(2))
    for s in (a, b):
        s.set_map(c["lm"])
        assert s.genealogy_rows()[1] == c["nlm"] * 4 + 1, "not a plain-row context"

    def packet_step(s, k, keep_below=None):
        """slamgpu_observe + slamgpu_step; keep_below: only the re-observed landmarks whose feature index the front end's table is sure of"""
        o = s.observe(c["xt"][k], mr, R, noise=2)
        if keep_below is not None:
            sel = o["idf"] < keep_below
            o = dict(zf=o["zf"][sel], idf=o["idf"][sel], zn=np.zeros((0, 2), f32))
        return o

    def particle_step(s, k):
        for V, G, phi in c["ctl"][k]:
            s.predict(float(V), float(G), Q, dt, float(phi))
        o = s.observe(c["xt"][k], mr, R, noise=2)
        if len(o["z"]):
            s.update_particle(o["z"], R, **OPT)
        s.estimate_async()

    k = 0
    # host-made packets
    rows_max = 0
    for _ in range(SEG["packets"]):
        for s in (a, b):
            o = packet_step(s, k)
            s.step(c["ctl"][k], Q, dt, o["zf"], o["idf"], o["zn"], R)
        rows_max = max(rows_max, a.live_rows())
        k += 1
    rows, _ = _same(a, b, "host-made packets")
    assert rows_max > 6 and rows <= rows_max, "the consolidation of plain rows never had anything to do"
    # the device front end: packet and book made on the device
    for _ in range(SEG["front"]):
        a.step_observe(c["ctl"][k], Q, dt, c["xt"][k], mr, R, noise=2)
        o = packet_step(b, k)
        b.step(c["ctl"][k], Q, dt, o["zf"], o["idf"], o["zn"], R)
        k += 1
    _same(a, b, "step_observe")
    nf_known = a.nf()  # (from here on new landmarks get their slots from the per-particle association, not from the front end's table)
    assert nf_known >= 6
    # the per-particle update, its bookkeeping on the host
    for _ in range(SEG["particle"]):
        particle_step(a, k)
        particle_step(b, k)
        k += 1
    _same(a, b, "update_particle")
    # ... and on the device, three iterations in one call
    n = SEG["device"]
    a.run_particle(c["ctl"][k:k + n], Q, dt, c["xt"][k:k + n], mr, R, noise=2, **OPT)
    for q in range(n):
        particle_step(b, k + q)
    k += n
    rep = a.particle_report_fetch()
    assert rep.shape[0] == n
    # a download (flatten) and an upload of it
    _, da = _same(a, b, "run_particle / download")
    a.upload(da)
    b.upload(da)
    _same(a, b, "upload")
    # host-made packets again (the same packet to both: the twin's, cut down to the landmarks known before the per-particle steps)
    for _ in range(SEG["again"]):
        a.observe(c["xt"][k], mr, R, noise=2)
        o = packet_step(b, k, keep_below=nf_known)
        for s in (a, b):
            s.step(c["ctl"][k], Q, dt, o["zf"], o["idf"], o["zn"], R)
        k += 1
    _same(a, b, "host-made packets again")
    a.close()
    b.close()
