"""Single contexts above 131 072 particles: every code path the step takes on the way to the size limit of 8 192 tiles.

With nb tiles of 256 particles and per = ceil(nb / 256) block totals per thread of the scan:
  nb > 512   scan_finish's batched loop (per >= 3) inside every update launch and inside resample_kernel
  nb > 768   FastSLAM 1: update_kernel_wide (kernels.h: update_is_wide); the context counts its launches
  nb > 1024  scan_kernel after every update (scan_segments<8 / 16 / 32>; log-weights: scan_block_totals) and the
             h_scan_global branch of update_step.inl
  nb = 8192  the limit: resample_kernel with 8 * (nb + 1) bytes of dynamic LDS
SIZES holds the first particle count of every regime (the last tile then holds ONE particle) and the limit itself.

The resampling plan is checked EXACTLY.  The in-tile prefix and the tile totals are float32 sums of the raw weights, the tile
prefix is a double sum of the totals, the target is (double) stratum * W.  When every weight is a small integer times 2^-20
(at most 2^15 units: a tile's sum stays below 2^24 units, the whole set's below 2^36) every one of those sums is exact in any
association, and the product stratum * W is one IEEE double multiplication on both sides.  A flat float64 model
    ancestor = searchsorted(cumsum(w), float64(stratum) * W, side="right"), clamped to N - 1
then IS the device's answer: any differing index is a bug, at any size.

Neff bound (NEFF_ROUNDINGS).  float32 roundings between a weight and neff_of's result, update_step.inl's tail onwards:
w / tw (a division: counted as a reciprocal, 2, and a product, 1); rw * rw (1); the wave's sum of 64 squares (6 levels of
the DPP scan); f = sh_w[k] / T (3, as above); f * f (1); sh_w2[k] * (f * f) (1); the four waves' terms added (4); the
conversion of W * W / Q to float32 in neff_of (1): 20.  The sums of the weights themselves are exact here.  Everything in
between is double (the products qk * tk^2, their sums over at most 8 192 tiles, v_rcp_f64 refined by one Newton step, the
rescaling exp(M_b - M) of log-weight contexts): a few 2^-53 each, and one more unit of 2^-24 covers all of them together with
the second-order terms of the twenty.  Every term of Q is positive, so the relative error of Q is at most that of its worst
term: |neff / model - 1| <= 21 * 2^-24 = 1.25e-6.  (Measured worst ratio: profiles/large_contexts.txt.)

Log-weights, generic case (LOGW_K).  Relative error of a cumulative position, in units of 2^-24: the argument l - M_b is a
float32 difference of magnitude below 4 (half an ulp: 2^-23 absolute = 2 units of the exponential); expf to one ulp (2, either
build: neither passes a fast-math flag to the compiler, both call the same expf); the in-tile prefix, a DPP scan of 64 lanes
and the waves' bases (8 additions; a tile total is the prefix's last entry): 12.  The target carries the same 12 through W.
K = 24.  A quarter of a stratum at the far end allows K * 2^-24 < 1 / (4 N), that is N < 174 762: the derived K breaks the
condition at 262 145 particles already, so the generic case runs at 131 073 only, both builds.  The structured case, which
needs no tolerance, runs at all three sizes."""
import functools
import os

import numpy as np
import pytest

from conftest import DATA
from test_gpu_parity import philox_steps_vs_oracle

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TILE = 256
SIZES = [131_073, 196_609, 262_145, 524_289, 1_048_577, 2_097_152]
LIMIT = 2_097_152
UNIT = 2.0 ** -20
SHAPES = "ABCDEF"
NEFF_ROUNDINGS = 21
LOGW_K = 24.0
R0 = np.array([[0.01, 0], [0, 3e-4]], f32)
NONE2, NONEI = np.zeros((0, 2), f32), np.zeros(0, np.int32)
BUILD = ("strict", "fast")


@pytest.fixture(scope="module")
def sg():
    import slam_amd
    assert slam_amd.device_count() >= 1, "GPU tests need a HIP device"
    return slam_amd


def tiles_of(N):
    nb = (N + TILE - 1) // TILE
    return nb, (nb + TILE - 1) // TILE


@functools.lru_cache(maxsize=2)
def strata_of(N):
    u = np.random.default_rng(77 + N).random(N)
    return ((np.arange(N) + u) / N).astype(f32)


def shape_units(shape, N):
    """the weight of every particle in units of 2^-20 (integers, at most 2^15)"""
    nb, per = tiles_of(N)
    u = np.random.default_rng(1000 * SHAPES.index(shape) + N).random(N)
    tile = np.arange(N) // TILE
    if shape == "A":    # heavy-tailed: Neff ~ 0.36 N
        m = np.floor(2.0 ** 15 * u ** 4)
    elif shape == "B":  # every ancestor at the far end
        m = np.zeros(N)
        m[-3:] = (5, 1, 7)
    elif shape == "C":  # the first tile only
        m = np.where(tile == 0, 1 + np.floor(2.0 ** 10 * u), 0.0)
    elif shape == "D":  # whole thread segments of the scan are zero, and the tile prefix has ties
        m = 1 + np.floor(2.0 ** 10 * u)
        m[tile % 2 == 1] = 0
        m[(tile // per) % 2 == 1] = 0
    elif shape == "E":  # one particle holds everything
        m = np.zeros(N)
        m[N // 2 + 1] = 3
    else:               # ancestors drift many tiles to one side
        m = 1 + np.floor((tile / nb) ** 3 * 2.0 ** 14 * u)
    assert m.min() >= 0 and m.max() <= 2 ** 15
    return m


@functools.lru_cache(maxsize=6)
def plan_case(N, shape):
    """weights, and the float64 model of the plan for the strata of this N: computed once, shared by every context of this N"""
    w = (shape_units(shape, N) * UNIT).astype(f32)
    return (w,) + flat_model(w, strata_of(N))


def flat_model(w, sel):
    N = w.shape[0]
    wd = w.astype(f64)
    c = np.cumsum(wd)
    W = float(c[-1])
    keep = np.minimum(np.searchsorted(c, sel.astype(f64) * W, side="right"), N - 1).astype(np.int32)
    return keep, W, W * W / float(np.sum(wd * wd))


def upload(s, w, xv):
    """pose x = the particle's own index, the given weights; covariances stay as they are"""
    from slam_amd.capi import _chk, _ptr
    _chk(s.L.slamgpu_upload(s.h, 0, _ptr(xv), None, _ptr(np.ascontiguousarray(w, f32)), None, None))


@functools.lru_cache(maxsize=1)
def index_pose(N):
    xv = np.zeros((N, 3), f32)
    xv[:, 0] = np.arange(N)   # (exact in float32 below 2^24)
    return xv


def ancestors_off_the_poses(s):
    got = s.download(landmarks=False)
    keep = np.rint(got["xv"][:, 0]).astype(np.int32)
    assert np.array_equal(got["xv"][:, 0], keep.astype(f32))
    return keep, got["w"]


def check_keep(keep, model, N, tag):
    assert keep.min() >= 0 and keep.max() < N and np.all(np.diff(keep) >= 0), tag
    bad = np.nonzero(keep != model)[0]
    print("LARGE %s: %d of %d ancestors differ from the float64 model" % (tag, bad.size, N))
    assert bad.size == 0, (tag, bad.size, bad[:8], keep[bad[:8]], model[bad[:8]])


def check_neff(neff, model, tag):
    ratio = abs(float(neff) / model - 1.0)
    print("LARGE %s: |Neff / model - 1| = %.3g = %.2f x 2^-24" % (tag, ratio, ratio * 2.0 ** 24))
    assert ratio <= NEFF_ROUNDINGS * 2.0 ** -24, (tag, float(neff), model, ratio)


# (a) FastSLAM 2 at every size, FastSLAM 1 where update_kernel_wide runs; both builds at 131 073, 262 145 and the limit
PLAN_CASES = ([(N, 2, 1) for N in SIZES] + [(N, 2, 0) for N in (131_073, 262_145, LIMIT)] +
              [(N, 1, 1) for N in SIZES[1:]] + [(N, 1, 0) for N in (262_145, LIMIT)])
PLAN_CASES.sort(key=lambda c: c[0])   # (one N after another: the models are computed once per N and shape)


@pytest.mark.parametrize("N,method,math_mode", PLAN_CASES, ids=["N%d-fs%d-%s" % (c[0], c[1], BUILD[c[2]]) for c in PLAN_CASES])
def test_resampling_plan_is_exact(sg, N, method, math_mode):
    """Six weight shapes through one context, both ways the resampling stage is reached: every ancestor, the sum of the weights
    and the decision equal the float64 model's; Neff within NEFF_ROUNDINGS * 2^-24 (module docstring)."""
    nb, per = tiles_of(N)
    s = sg.SlamGpu(N, 1, method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_TAPE, math_mode=math_mode)
    sel, xv = strata_of(N), index_pose(N)
    for shape in SHAPES:
        w, model, W, neff_m = plan_case(N, shape)
        assert neff_m < 0.5 * N   # (the resample fires at 0.75 N with room to spare)
        for path in ("stage", "inline"):
            tag = "N=%d nb=%d per=%d fs%d %s %s %s" % (N, nb, per, method, BUILD[math_mode], shape, path)
            upload(s, w, xv)
            s.update(NONE2, NONEI, NONE2, R0, None, sel)
            if path == "stage":   # resample_kernel / finish_kernel as launches of their own
                neff, did, wsum = s.stats()
                assert did, tag
                assert wsum == W, (tag, wsum, W)
                check_neff(neff, neff_m, tag)
                keep = s.ancestors()
            else:                 # the plan at the head of the next update launch; the ancestors are read off the particles
                s.update(NONE2, NONEI, NONE2, R0, None, sel)
                keep, wgot = ancestors_off_the_poses(s)
                assert np.all(wgot == f32(1.0) / f32(N)), tag
            check_keep(keep, model, N, tag)
    wide = s.wide_launches()
    s.close()
    if method == 1:
        assert wide > 0
    else:
        assert wide == 0


def test_philox_plan_at_the_size_limit(sg, oracle):
    """2 097 152 particles, the device's own strata (Philox stream 1, float32 values of (i + u) / N) against the oracle's
    restatement of the generator: exact ancestors, both paths; one particle more is refused."""
    N, seed = LIMIT, 11
    s = sg.SlamGpu(N, 1, method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=seed, math_mode=1)
    w = (shape_units("A", N) * UNIT).astype(f32)
    xv = index_pose(N)
    step = 0
    for path in ("stage", "inline"):
        tag = "N=%d philox fast A %s" % (N, path)
        upload(s, w, xv)
        s.update(NONE2, NONEI, NONE2, R0)
        step += 1
        _, sel = oracle.philox_update_tape(seed, step, 0, N, N, want_normals=False)   # the strata of THIS update
        model, W, neff_m = flat_model(w, sel)
        if path == "stage":
            neff, did, wsum = s.stats()
            assert did and wsum == W, (tag, wsum, W)
            check_neff(neff, neff_m, tag)
            keep = s.ancestors()
        else:
            s.update(NONE2, NONEI, NONE2, R0)
            step += 1
            keep, wgot = ancestors_off_the_poses(s)
            assert np.all(wgot == f32(1.0) / f32(N)), tag
        check_keep(keep, model, N, tag)
    s.close()
    with pytest.raises(sg.SlamGpuError) as e:
        sg.SlamGpu(N + 1, 1, method=2, rng_mode=sg.RNG_PHILOX, seed=seed, math_mode=1)
    assert e.value.code == -1   # SLAMGPU_ERR_INVALID


# ---- (c) log-weight contexts past two totals per thread ----------------------------------------------------------------

LOGW_SEED = {131_073: 1, 262_145: 1, 1_048_577: 1}   # (seeds at which no stratum lies within 8 * 2^-52 of a boundary of the model)


@functools.lru_cache(maxsize=2)
def structured_case(N):
    """l = c_b + {0, -inf}: expf(l - M_b) is exactly 0 or 1, a tile's total an exact count; only exp(M_b - M) (double) rounds.
    Model: count * exp(float64(c_b) - M), the tile prefix in extended precision so that the model's own sums do not count."""
    nb, _ = tiles_of(N)
    rng = np.random.default_rng(LOGW_SEED[N])
    tile = np.arange(N) // TILE
    cb = (-60.0 * rng.random(nb)).astype(f32)
    on = rng.random(N) < 0.5
    on[(rng.random(nb) < 0.1)[tile]] = False   # some tiles are all -inf
    logw = np.where(on, cb[tile], -np.inf).astype(f32)
    u = rng.random(N)
    sel = ((np.arange(N) + u) / N).astype(f32)
    first = np.arange(0, N, TILE)
    cnt = np.add.reduceat(on.astype(np.int64), first)
    M = float(cb[cnt > 0].max())
    sb = np.where(cnt > 0, np.exp(cb.astype(f64) - M), 0.0)
    T = cnt * sb
    P = np.concatenate([[0.0], np.cumsum(T.astype(np.longdouble))])
    cs = np.cumsum(on.astype(np.int64))
    incl = cs - np.concatenate([[0], cs[first[1:] - 1]])[tile]   # inclusive count inside the tile
    cum = np.maximum.accumulate(P[tile] + incl * sb[tile].astype(np.longdouble))
    W = float(P[-1])
    t = sel.astype(f64) * W
    a = np.searchsorted(cum, t.astype(np.longdouble), side="right")
    below = np.where(a > 0, cum[np.maximum(a - 1, 0)], 0.0)
    above = cum[np.minimum(a, N - 1)]
    eps = 8.0 * 2.0 ** -52 * t
    near = (t - below <= eps) | (above - t <= eps) | (a >= N)
    neff = W * W / float(np.sum(cnt * sb * sb))
    return logw, sel, np.minimum(a, N - 1).astype(np.int32), int(near.sum()), float(M + np.log(W)), neff


@pytest.mark.parametrize("N,math_mode", [(131_073, 0), (131_073, 1), (262_145, 1), (1_048_577, 1)],
                         ids=lambda v: str(v))
def test_log_weights_structured_plan(sg, N, math_mode):
    """per = 3, 5 and 17 with log-weights: the fmaxf sweep and block_scale per entry in scan_finish (inside the update launch
    up to 1 024 tiles, inside scan_kernel above, inside resample_kernel always)."""
    logw, sel, model, near, lsum_m, neff_m = structured_case(N)
    assert near == 0   # on the model alone: no stratum close enough to a boundary for exp()'s last bits to decide
    assert neff_m < 0.5 * N
    s = sg.SlamGpu(N, 1, method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_TAPE, math_mode=math_mode, log_weights=True)
    xv = index_pose(N)
    for path in ("stage", "inline"):
        tag = "N=%d logw structured %s %s" % (N, BUILD[math_mode], path)
        upload(s, logw, xv)
        s.update(NONE2, NONEI, NONE2, R0, None, sel)
        if path == "stage":
            neff, did, lsum = s.stats()
            assert did, tag
            assert abs(lsum - lsum_m) <= 1e-12 * max(1.0, abs(lsum_m)), (tag, lsum, lsum_m)
            check_neff(neff, neff_m, tag)
            keep = s.ancestors()
        else:
            s.update(NONE2, NONEI, NONE2, R0, None, sel)
            keep, wgot = ancestors_off_the_poses(s)
            assert np.all(wgot == wgot[0]) and abs(float(wgot[0]) - np.log(1.0 / N)) < 1e-5, tag
        check_keep(keep, model, N, tag)
    s.close()


@pytest.mark.parametrize("math_mode", [0, 1], ids=BUILD)
def test_log_weights_generic_plan(sg, math_mode):
    """l = -4 u^2 (a spread of e^4) at 131 073 particles: every ancestor bracketed by the float64 cumulative sum of exp(l) with
    LOGW_K * 2^-24 of slack (module docstring: why this size only)."""
    N = 131_073
    assert LOGW_K * 2.0 ** -24 < 1.0 / (4 * N)
    rng = np.random.default_rng(31)
    logw = (-4.0 * rng.random(N) ** 2).astype(f32)
    sel = ((np.arange(N) + rng.random(N)) / N).astype(f32)
    C = np.cumsum(np.exp(logw.astype(f64)))
    W = float(C[-1])
    neff_m = W * W / float(np.sum(np.exp(2.0 * logw.astype(f64))))
    assert neff_m < 0.7 * N
    t = sel.astype(f64) * W
    s = sg.SlamGpu(N, 1, method=2, n_effective=int(0.75 * N), rng_mode=sg.RNG_TAPE, math_mode=math_mode, log_weights=True)
    xv = index_pose(N)
    for path in ("stage", "inline"):
        tag = "N=%d logw generic %s %s" % (N, BUILD[math_mode], path)
        upload(s, logw, xv)
        s.update(NONE2, NONEI, NONE2, R0, None, sel)
        if path == "stage":
            neff, did, lsum = s.stats()
            assert did, tag
            assert abs(lsum - np.log(W)) <= 12 * 2.0 ** -24, (tag, lsum, np.log(W))   # (the 12 units of a cumulative position)
            # (here a weight carries 4 units itself, the argument and expf: W^2 and Q 8 each; and the float32 sums of the weights are
            # no longer exact: 8 additions under W, squared, 16 -- in Q the totals cancel against the ratios w / T.  32 on top.)
            ratio = abs(float(neff) / neff_m - 1.0)
            print("LARGE %s: |Neff / model - 1| = %.3g = %.2f x 2^-24" % (tag, ratio, ratio * 2.0 ** 24))
            assert ratio <= (NEFF_ROUNDINGS + 32) * 2.0 ** -24, (tag, float(neff), neff_m)
            keep = s.ancestors()
        else:
            s.update(NONE2, NONEI, NONE2, R0, None, sel)
            keep, wgot = ancestors_off_the_poses(s)
            assert np.all(wgot == wgot[0]) and abs(float(wgot[0]) - np.log(1.0 / N)) < 1e-5, tag
        assert keep.min() >= 0 and keep.max() < N and np.all(np.diff(keep) >= 0), tag
        lo = np.where(keep > 0, C[np.maximum(keep - 1, 0)], 0.0)
        hi = C[keep]
        unit = 2.0 ** -24 * hi
        last = keep == N - 1   # (a stratum beyond the last cumulative weight is clamped to the last particle)
        used = max(float(((lo - t) / unit).max()), float(((t - hi) / unit)[~last].max()), 0.0)
        print("LARGE %s: largest slack used %.2f x 2^-24 x C[a] (allowed %.0f)" % (tag, used, LOGW_K))
        assert np.all(t >= lo - LOGW_K * unit), (tag, used)
        assert np.all((t < hi + LOGW_K * unit) | last), (tag, used)
    s.close()


# ---- (d) the wide step against the oracle -------------------------------------------------------------------------------

@pytest.mark.parametrize("math_mode", [0, 1], ids=BUILD)
def test_wide_step_vs_oracle(sg, oracle, math_mode):
    """FastSLAM 1 at 196 609 particles (769 tiles: update_kernel_wide), teacher-forced against the oracle with the bounds of
    tests/test_gpu_parity.py.  Seed 7, Philox particle noise: the oracle resamples at observation steps 5 and 6 and not before."""
    resamples, plain, wide, wide_shadow = philox_steps_vs_oracle(sg, oracle, 1, 196_609, 6, math_mode)
    assert resamples >= 1 and plain >= 1, (resamples, plain)
    assert wide > 0 and wide_shadow > 0, (wide, wide_shadow)


# ---- (e) the alternatives at real size: bit-identical ------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def webmap_tape(method):
    from slam_amd import host
    return host.make_tape(["-m", os.path.join(DATA, "example_webmap.mat"), "-method", method, "-NPARTICLES", 1000, "-NEFFECTIVE", 750,
                           "-SWITCH_SEED_RANDOM", 4], max_obs=12)


def run_tape(sg, method, N, log_weights=False):
    tape = webmap_tape("FASTSLAM%d" % method)
    s = sg.SlamGpu(N, tape["nlm"], method=method, n_effective=int(0.75 * N), rng_mode=sg.RNG_PHILOX, seed=6, math_mode=1,
                   log_weights=log_weights)
    for st in tape["steps"]:
        s.step(np.array(st["controls"], f32).reshape(-1, 3), tape["Q"], float(tape["dt"]), st["zf"], st["idf"], st["zn"], tape["R"])
    hist = s.history_fetch()
    state = s.download()
    wide = s.wide_launches()
    s.close()
    return hist, state, wide


def assert_same_bits(a, b, tag):
    (ha, sa, _), (hb, sb, _) = a, b
    assert len(ha[0]) == 12, tag
    print("LARGE %s: %d resamples in 12 observation steps" % (tag, int(ha[2].sum())))
    assert ha[2].sum() >= 3, (tag, ha[2])
    for x, y in zip(ha, hb):
        assert np.array_equal(x, y), tag
    assert sa["nf"] == sb["nf"] and sa["nf"] > 0, tag
    for key in ("xv", "Pv", "w", "xf", "Pf"):
        assert np.array_equal(sa[key].view(np.uint32), sb[key].view(np.uint32)), (tag, key)


@pytest.mark.parametrize("N", [196_609, 1_048_577])
def test_wide_kernel_changes_no_bit(sg, monkeypatch, N):
    """FastSLAM 1 above 768 tiles: update_kernel_wide against update_kernel (SLAMGPU_NO_WIDE=1, read when the context is made)."""
    monkeypatch.delenv("SLAMGPU_NO_WIDE", raising=False)
    a = run_tape(sg, 1, N)
    monkeypatch.setenv("SLAMGPU_NO_WIDE", "1")
    b = run_tape(sg, 1, N)
    assert a[2] > 0 and b[2] == 0, (a[2], b[2])
    assert_same_bits(a, b, "N=%d fs1 wide against plain" % N)


@pytest.mark.parametrize("N,log_weights", [(262_145, False), (524_289, False), (1_048_577, False), (262_145, True)],
                         ids=["N262145", "N524289", "N1048577", "N262145-logw"])
def test_scan_kernel_changes_no_bit(sg, monkeypatch, N, log_weights):
    """FastSLAM 2 above 1 024 tiles (per = 5, 9, 17): the prefix from scan_kernel (register segments; log-weights:
    scan_block_totals) against every tile's own scan (SLAMGPU_SCAN_MIN_BLOCKS=8192)."""
    monkeypatch.delenv("SLAMGPU_SCAN_MIN_BLOCKS", raising=False)
    a = run_tape(sg, 2, N, log_weights)
    monkeypatch.setenv("SLAMGPU_SCAN_MIN_BLOCKS", "8192")
    b = run_tape(sg, 2, N, log_weights)
    assert a[2] == 0 and b[2] == 0
    assert_same_bits(a, b, "N=%d fs2%s scan kernel against inline scan" % (N, " logw" if log_weights else ""))
