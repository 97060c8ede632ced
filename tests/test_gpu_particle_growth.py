"""The per-particle association's device buffers while they grow (association.cpp: DevBuf::reserve at the sizes pp_reserve, pp_grow_tab,
pp_reserve_particles, associate_impl, mx_reserve and das_reserve ask for): steps of 3, 70, 150 and 20 observations -- 70 is past the first
capacity of 64 observations, 150 past twice 70, 20 a step after everything has grown -- with the mutual-exclusion table and the sampling
ratios released and reserved again in between.  A step whose buffers were just replaced must be the step it would have been: the labels
slamgpu_update_particle made, replayed into a twin through slamgpu_update_labels, leave the twin's state, weights and reports equal bit
for bit after every step, and the cumulative counters count on across a release."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 300                    # not a multiple of 256: the padding up to ncap is live
COUNTS = (3, 70, 150, 20)  # observations per step
R = np.array([0.1 ** 2, 0.0, 0.0, np.radians(1.0) ** 2], f32)
Q = np.array([0.3 ** 2, 0.0, 0.0, np.radians(3.0) ** 2], f32)


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1
    return slam_amd


@pytest.fixture(scope="module")
def steps():
    """150 landmarks on five rings around the origin, where every particle starts (1.5 m apart or more); step k observes the first
    COUNTS[k] of them, range and bearing with the sensor's noise."""
    i = np.arange(max(COUNTS))
    z = np.stack([8.0 + 4.0 * (i // 30), -2.8 + 0.19 * (i % 30)], 1)
    rng = np.random.default_rng(5)
    return [(z[:n] + rng.normal(size=(n, 2)) * np.sqrt(R[[0, 3]])).astype(f32) for n in COUNTS]


def _context(sg, math_mode):
    return sg.SlamGpu(N, 512, method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=9, math_mode=math_mode, particle_maps=True,
                      log_weights=True)  # (150 likelihoods in one step: their product is below float32 in linear weights)


def _predict(s):
    """2.5 cm ahead before every step: FastSLAM 2's proposal needs the pose covariance a predict leaves"""
    s.predict(1.0, 0.0, Q, 0.025)


def _same(a, b, what):
    for k in ("xv", "Pv", "w", "xf", "Pf"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(x, y, equal_nan=True), (what, k, int((x != y).sum()))
    assert a["nf"] == b["nf"], (what, a["nf"], b["nf"])


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("mode", [0, 3], ids=["auto", "lists"])  # SLAMGPU_ASSOC_AUTO, SLAMGPU_ASSOC_LISTS
def test_steps_that_grow_the_buffers_replay_bit_for_bit(sg, steps, mode, math_mode):
    """Context A associates (mutual exclusion on, off, on, on: its table is released and reserved again while the other buffers grow);
    twin B takes A's labels.  _AUTO: the exhaustive scan while the map has fewer than 64 slots, the prefilter with the census riding in
    its launch after; _LISTS: associate_lists in every step."""
    a, b = _context(sg, math_mode), _context(sg, math_mode)
    opt = dict(new_share=0.02, p_new=0.05, census_every=1)
    on_steps = 0
    for k, (z, mx) in enumerate(zip(steps, (True, False, True, True))):
        a.set_particle_mutex(mx)
        _predict(a)
        _predict(b)
        ra = a.update_particle(z, R, mode=mode, **opt)
        lab = a.particle_labels()
        assert lab.shape == (N, len(z))
        rb = b.update_labels(z, R, lab, **opt)
        a.estimate_async()
        b.estimate_async()
        assert ra == rb, (k, ra, rb)
        assert ra["dropped"] == 0, (k, ra)
        _same(a.download(), b.download(), "step %d (%d observations)" % (k, len(z)))
        on_steps += mx
        st = a.particle_mutex_stats()
        assert st["steps"] == on_steps, (k, st)  # (the counters outlive the table: they count on after a release)
    assert a.download()["nf"] >= 100  # (the map grew past both capacities: most of the 150 landmarks have a slot)
    ea, eb = a.history_fetch(), b.history_fetch()
    a.close()
    b.close()
    assert len(ea[0]) == len(COUNTS) and np.isfinite(ea[0]).all()
    for x, y in zip(ea, eb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_sampling_toggled_while_the_buffers_grow(sg, steps, math_mode):
    """Data association sampling on for the steps of 3 and 70 observations, off for the step of 150 (the ratios are released), on again
    for the step of 20 (reserved again, behind buffers that have grown since): the counters count the three steps, the step without
    sampling leaves them as they were, and every step is a valid one."""
    s = _context(sg, math_mode)
    seen, on_steps = None, 0
    for k, (z, on) in enumerate(zip(steps, (True, True, False, True))):
        s.set_particle_assoc_sampling(on)
        _predict(s)
        rep = s.update_particle(z, R, mode=0, new_share=0.02, p_new=0.05, census_every=1)
        assert rep["dropped"] == 0, (k, rep)
        assert s.particle_labels().shape == (N, len(z))
        st = s.particle_sample_stats()
        on_steps += on
        assert st["steps"] == on_steps, (k, st)
        if not on:
            assert st == seen, (k, st, seen)
        seen = st
        d = s.download()
        assert np.isfinite(d["w"]).all() and np.isfinite(d["xv"]).all(), k
    s.close()
