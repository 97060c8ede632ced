"""The inline plan at the head of the specialised update launch (update_step.inl; kernels.hip: scan_totals / scan_prefix, find_ancestor_win)
at the sizes and weights where its pieces can go wrong: partial last waves and tiles and a one-lane tile (the lanes in use are a
prefix of the wave, and the window's bounds are taken over them alone), the ancestor window read as LDS with the per-lane arm beside it
(an output wave that draws from more source tiles than the window holds), the block prefix written only by launches that resample (and
a launch that does not), plateaus of the prefix under the galloping search.

Three ways to the ancestors of one uploaded weight vector, which must agree BIT FOR BIT:
  special   the inline plan of update_kernel_special<2, p> (FastSLAM 2, Philox, the heading observed),
  general   the same context created under SLAMGPU_NO_SPECIAL=1: the general instantiation's text,
  stage     resample_kernel as launches of its own (stats() / ancestors(): find_ancestor, per lane).
Every particle carries its index in its pose, as in tests/test_gpu_resample_kat.py's inline path, so the ancestors of the inline ways
are read off the particles.

How a launch gets specialised here: the launcher compares the launch's own values with kernels.h: kUpdateSpecs, and the heading flag is
a value of the QUEUED PREDICTS (PredictArgs::use_heading), so a launch without any has none of it and is a general launch.  The second
step therefore queues ONE predict, with V = 0: x += V dt cos(..) leaves the index in x exactly as it was.  That the launch was a
specialised one (and, with a re-observed landmark, a counted one) is asserted from the context's counters."""
import numpy as np
import pytest

from test_gpu_special import assert_same, bits, run, sg, tape_of  # noqa: F401  (sg: fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
K_BLOCK = 256     # kernels.h: kBlock
K_WIN = 4         # kernels.hip: kWinBlocks
NS = [1, 63, 64, 65, 255, 256, 257, 300, 1024, 1279]
Q = np.array([[0.09, 0], [0, 0.0027]], f32)
R = np.array([[0.01, 0], [0, 3e-4]], f32)
DT = 0.025
NONE2, NONEI = np.zeros((0, 2), f32), np.zeros(0, np.int32)
STILL = np.zeros((1, 3), f32)  # one queued predict: V = 0, G = 0, observed heading 0


def n_eff_of(N):
    """fires for every weight vector below (their Neff is at most N / 2) and not for the uniform set the resample leaves (Neff = N);
    one particle: Neff = 1 whatever the weight, so the second stage fires too, and maps particle 0 to particle 0"""
    return max(2, int(0.9 * N))


def neff64(w):
    w = w.astype(np.float64)
    return w.sum() ** 2 / (w * w).sum()


def patterns(N):
    """name -> weights.  Smooth random ones; all the weight on one particle (every lane of every wave has the same source block: the
    window's first and last block are the same); a last particle of weight zero"""
    rng = np.random.default_rng(1000 + N)
    smooth = np.exp(2.0 * rng.standard_normal(N)).astype(f32)
    out = {"smooth": smooth}
    for name, at in (("first", 0), ("last", N - 1), ("middle", N // 2)):
        w = np.zeros(N, f32)
        w[at] = 0.75
        out["one_" + name] = w
    if N > 1:
        w = smooth.copy()
        w[-1] = 0.0
        out["last_zero"] = w
    return out


def plateau(N):
    """whole tiles of zero weight between live ones: plateaus in the block prefix"""
    rng = np.random.default_rng(2000 + N)
    w = np.exp(2.0 * rng.standard_normal(N)).astype(f32)
    nb = (N + K_BLOCK - 1) // K_BLOCK
    for b in range(1, nb - 1, 2):
        w[b * K_BLOCK:(b + 1) * K_BLOCK] = 0.0
    if nb == 4:
        w[K_BLOCK:3 * K_BLOCK] = 0.0  # (two dead tiles side by side)
    return w


def crossing():
    """2 048 particles: particle 0 holds 0.5, one particle in each of tiles 1 .. 6 holds 1e-3, one particle of tile 7 the rest: the strata
    just above 0.5 cross six tiles inside one output wave -- more than the window's kWinBlocks: the per-lane arm runs"""
    w = np.zeros(2048, f32)
    w[0] = 0.5
    for b in range(1, 7):
        w[b * K_BLOCK + 37 * b] = 1e-3
    w[7 * K_BLOCK + 100] = 1.0 - 0.5 - 6e-3
    return w


def state(N, w, landmark=False):
    xv = np.zeros((N, 3), f32)
    xv[:, 0] = np.arange(N)  # every particle carries its own index
    st = dict(nf=0, xv=xv, Pv=np.zeros((N, 3, 3), f32), w=w, xf=None, Pf=None)
    if landmark:
        # (a pose covariance the proposal can invert, and one landmark 10 m ahead of every particle)
        st["Pv"] = np.tile(np.diag([1e-2, 1e-2, 1e-4]).astype(f32), (N, 1, 1))
        st["nf"] = 1
        st["xf"] = np.stack([xv[:, 0] + 10.0, np.zeros(N, f32)], axis=1).reshape(N, 1, 2).astype(f32)
        st["Pf"] = np.tile(np.diag([0.05, 0.05]).astype(f32), (N, 1, 1, 1))
    return st


def context(sg, monkeypatch, general, N, n_eff, math_mode):
    if general:
        monkeypatch.setenv("SLAMGPU_NO_SPECIAL", "1")
    else:
        monkeypatch.delenv("SLAMGPU_NO_SPECIAL", raising=False)
    s = sg.SlamGpu(N, 1, method=2, n_effective=n_eff, use_heading=True, rng_mode=sg.RNG_PHILOX, seed=7, math_mode=math_mode)
    monkeypatch.delenv("SLAMGPU_NO_SPECIAL", raising=False)  # (read at creation: the context keeps what it found)
    return s


def inline(sg, monkeypatch, general, N, w, n_eff, math_mode, zf=NONE2, idf=NONEI):
    """first update: the weights' prefix and block totals (a general launch: nothing to plan); second step: its launch plans the first
    one's resampling stage at its head and applies it.  Returns the state after it, (Neff, resampled) of the first stage as the launch
    worked them out, and the launch counters"""
    s = context(sg, monkeypatch, general, N, n_eff, math_mode)
    s.upload(state(N, w, landmark=len(idf) > 0))
    s.update(NONE2, NONEI, NONE2, R)
    s.estimate_async()  # (history entry 0: filled by the launch that plans this update's stage)
    s.step(STILL, Q, DT, zf, idf, NONE2, R)
    got = s.peek()
    _, neff, res = s.history_fetch()
    special, counted = s.special_launches(), s.counted_launches()
    s.close()
    return got, f32(neff[0]), bool(res[0]), special, counted


def stage(sg, monkeypatch, N, w, n_eff, math_mode, zf=NONE2, idf=NONEI):
    """the first update's resampling stage as launches of its own, then the same second step (its launch has nothing left to plan)"""
    s = context(sg, monkeypatch, False, N, n_eff, math_mode)
    s.upload(state(N, w, landmark=len(idf) > 0))
    s.update(NONE2, NONEI, NONE2, R)
    neff, did, _ = s.stats()
    keep = s.ancestors()
    s.step(STILL, Q, DT, zf, idf, NONE2, R)
    got = s.peek()
    s.close()
    return got, f32(neff), did, keep


def check_weights_after(w, N):
    """what a resampled set reads back as: the launch gives every particle 1/N as the host rounds it (slamgpu.cpp: Ctrl::inv_n); peek()
    then runs the second step's own stage, which does not resample a uniform set but divides by the float of its sum.  That sum is 1
    to the rounding of 1/N and of a tile's float32 prefix (at most 256 additions of 2^-24 each; the sums across tiles are double),
    and the quotient rounds once more: every weight the same float, within 258 * 2^-24 of 1/N"""
    assert np.all(bits(w) == bits(w)[0]), w[:4]
    assert abs(float(w[0]) * N - 1.0) <= 258 * 2.0 ** -24, (w[0], N)


def three_ways(sg, monkeypatch, N, w, math_mode, fires=True, n_eff=None):
    n_eff = n_eff_of(N) if n_eff is None else n_eff
    n64 = neff64(w)
    assert (n64 < 0.8 * n_eff) if fires else (n64 >= n_eff + 0.5), (n64, n_eff)  # (the test's own weights: well on one side)
    a = inline(sg, monkeypatch, False, N, w, n_eff, math_mode)
    b = inline(sg, monkeypatch, True, N, w, n_eff, math_mode)
    c = stage(sg, monkeypatch, N, w, n_eff, math_mode)
    # the launch that planned was update_kernel_special<2, p> (no re-observed landmark: not a counted one); never under the switch
    assert a[3] == 1 and a[4][0] == 1 and not any(a[4][1:]), (a[3], a[4])
    assert b[3] == 0 and not any(b[4]), (b[3], b[4])
    # Neff and the decision: the same float, the same bit
    nbits = bits(np.asarray([a[1], b[1], c[1]], f32))
    assert nbits[0] == nbits[1] == nbits[2], (a[1], b[1], c[1])
    # (against float64: a tile's total is the last entry of a float32 prefix of at most 256 terms, each addition within 2^-24; the
    # sums across tiles are double.  W enters squared; Q once, with a tile's float32 sum of squares on top: 4 * 256 * 2^-24)
    np.testing.assert_allclose(a[1], n64, rtol=4 * 256 * 2.0 ** -24)
    assert a[2] == b[2] == c[2] == fires, (a[2], b[2], c[2])
    for key in ("xv", "Pv", "w"):
        assert np.array_equal(bits(a[0][key]), bits(b[0][key])), key
        assert np.array_equal(bits(a[0][key]), bits(c[0][key])), key
    if not fires:
        # nobody moved; the weights normalised twice (by the launch or the first stage, then by the second step's stage), the same bits
        assert np.array_equal(a[0]["xv"][:, 0], np.arange(N, dtype=f32))
        return None
    keep = np.rint(a[0]["xv"][:, 0]).astype(np.int32)
    assert np.array_equal(a[0]["xv"][:, 0], keep.astype(f32))
    assert np.array_equal(keep, c[3]), np.nonzero(keep != c[3])[0][:8]
    assert np.all(np.diff(keep) >= 0) and keep.min() >= 0 and keep.max() < N
    assert np.all(w[keep] > 0)  # (nobody descends from a particle without weight)
    check_weights_after(a[0]["w"], N)
    return keep


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_ancestors_three_ways(sg, monkeypatch, math_mode, N):
    """partial last waves and tiles (63, 65, 255, 257, 300, 1 279), a one-lane second tile (257), one lane in all (1), four totals or
    fewer against several; per size: smooth weights, all the weight on the first / the last / the middle particle, a last particle of
    weight zero"""
    for name, w in patterns(N).items():
        keep = three_ways(sg, monkeypatch, N, w, math_mode)
        if name.startswith("one_"):
            assert np.all(keep == int(np.nonzero(w)[0][0])), name


@pytest.mark.parametrize("N", [300, 1024, 1279])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_no_resample_leaves_the_prefix_unwritten(sg, monkeypatch, math_mode, N):
    """uniform weights: Neff = N, the launch does not resample and so does not write the block prefix; it normalises exactly as the
    general kernel and the stage do"""
    three_ways(sg, monkeypatch, N, np.full(N, 0.25, f32), math_mode, fires=False, n_eff=n_eff_of(N))


@pytest.mark.parametrize("N", [1024, 1279])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_dead_tiles_between_live_ones(sg, monkeypatch, math_mode, N):
    w = plateau(N)
    keep = three_ways(sg, monkeypatch, N, w, math_mode)
    tiles = set((keep // K_BLOCK).tolist())
    dead = {b for b in range((N + K_BLOCK - 1) // K_BLOCK) if not w[b * K_BLOCK:(b + 1) * K_BLOCK].any()}
    assert dead and not (tiles & dead) and len(tiles) >= 2, (tiles, dead)


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_a_wave_that_draws_from_more_tiles_than_the_window_holds(sg, monkeypatch, math_mode):
    w = crossing()
    keep = three_ways(sg, monkeypatch, 2048, w, math_mode)
    # the construction does what it claims: the wave that holds the outputs around index 1 024 has ancestors in at least five tiles
    wave = keep[1024:1024 + 64] // K_BLOCK
    print("source tiles of outputs 1024 .. 1087:", sorted(set(wave.tolist())))
    assert len(set(wave.tolist())) >= 5 and int(wave.max()) - int(wave.min()) >= K_WIN, wave


@pytest.mark.parametrize("N", [300, 1279])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_one_reobserved_landmark_goes_through_the_counted_kernel(sg, monkeypatch, math_mode, N):
    """a single uploaded landmark re-observed once: update_kernel_counted<2, p, 1> plans.  The proposal moves the pose, so the index
    cannot be read off it: the whole state, bit for bit, between the three ways (a particle's pose after the step depends on the
    ancestor it was sampled around), and the stage's own ancestors for the properties"""
    w = patterns(N)["smooth"]
    n_eff = n_eff_of(N)
    zf, idf = np.array([[10.2, 0.03]], f32), np.array([0], np.int32)
    a = inline(sg, monkeypatch, False, N, w, n_eff, math_mode, zf, idf)
    b = inline(sg, monkeypatch, True, N, w, n_eff, math_mode, zf, idf)
    c = stage(sg, monkeypatch, N, w, n_eff, math_mode, zf, idf)
    assert a[3] == 1 and a[4][1] == 1 and sum(a[4]) == 1, (a[3], a[4])
    assert b[3] == 0 and not any(b[4]), (b[3], b[4])
    assert bits(np.asarray([a[1]], f32))[0] == bits(np.asarray([b[1]], f32))[0] == bits(np.asarray([c[1]], f32))[0]
    assert a[2] and b[2] and c[2]
    for key in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(bits(a[0][key]), bits(b[0][key])), key
        assert np.array_equal(bits(a[0][key]), bits(c[0][key])), key
    keep = c[3]
    assert np.all(np.diff(keep) >= 0) and keep.min() >= 0 and keep.max() < N
    # the particles are where their ancestors were, to what one observation moves a pose of this covariance
    assert np.all(np.abs(a[0]["xv"][:, 0] - keep) < 2.0)


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_webmap_whole_run_special_equals_general(sg, monkeypatch, math_mode):
    """example_webmap's first 120 observation steps at 300 particles (two tiles, the last wave and tile partial): state and history of
    the specialised and counted launches bit for bit those of the general instantiation"""
    tape = tape_of("example_webmap", 2, 120)
    a = run(sg, monkeypatch, False, tape, 300, every=7, method=2, math_mode=math_mode)
    b = run(sg, monkeypatch, True, tape, 300, every=7, method=2, math_mode=math_mode)
    assert_same(a, b)
    res = np.asarray(a[1][2])[:-1]
    assert res.any() and not res.all(), res
    assert a[2] >= a[3] - 1 - len(a[0]) and b[2] == 0, (a[2], b[2])
