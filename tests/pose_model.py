"""float64 / math.fsum model of the pose posterior (include/slamgpu.h: slamgpu_pose_summary) and of its NEES (include/slamhost.h:
slamhost_pose_nees), written from the headers' definitions only; the yardstick of tests/test_pose_cpu.py and tests/test_gpu_pose.py.

The set is what slamgpu_peek shows: present_set() applies a pending gather (pose through keep[], weight 1 / N).  The weights are
slamgpu_map_summary's: w / sum w, or exp(l - max l) normalised for log-weight contexts.  Headings enter as
u_i = IEEE remainder(theta_i - theta_p, 2 pi) about the heading theta_p of particle 0 of the set (math.remainder: exact), so the model
makes the same one pass the contract describes.  Sums are math.fsum's: exactly rounded.

bounds() gives the rounding bounds the GPU tests hold the device to (their derivation: tests/test_gpu_pose.py's docstring).
self_check() runs the model on sets with known answers."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
STRIDE = 18
TWO_PI = 2.0 * math.pi  # the double nearest to 2 pi (doubling is exact)
U = 2.0 ** -53
CHI2_3_95 = 7.8147
NAN18 = np.full(STRIDE, np.nan)


def present_set(xv, Pv, w, keep=None):
    """the set slamgpu_peek shows: under a pending gather (keep: the ancestors) particle k is ancestor keep[k] with weight float32(1 / N)"""
    xv, Pv, w = np.asarray(xv, f32), np.asarray(Pv, f32), np.asarray(w, f32)
    if keep is None:
        return xv, Pv, w
    keep = np.asarray(keep)
    return xv[keep], Pv[keep], np.full(len(keep), f32(1.0) / f32(len(keep)), f32)


def weights(w, logw=False):
    """normalised float64 weights, or None where they sum to zero or to nothing finite"""
    w = np.asarray(w, f32).astype(f64)
    if logw:
        m = w.max() if len(w) else -math.inf
        if math.isnan(m) or m == math.inf:
            return None
        with np.errstate(all="ignore"):
            w = np.exp(w - m) if m != -math.inf else np.zeros_like(w)
    if not np.isfinite(w).all():
        return None
    tot = math.fsum(w)
    if not (tot > 0.0) or not math.isfinite(tot):
        return None
    return w / tot


def deviations(theta):
    """u_i = remainder(theta_i - theta_p, 2 pi) in double, theta_p = theta_0 (float32 promoted)"""
    th = np.asarray(theta, f32).astype(f64)
    return np.array([math.remainder(t - th[0], TWO_PI) for t in th], f64)


def summary(xv, Pv, w, logw=False):
    """out[18] of slamgpu_pose_summary for the set (xv[N, 3], Pv[N, 3, 3], w[N]: float32 as peek returns them)"""
    xv, Pv = np.asarray(xv, f32).astype(f64), np.asarray(Pv, f32).astype(f64)
    wh = weights(w, logw)
    if wh is None:
        return NAN18.copy()
    x, y, th = xv[:, 0], xv[:, 1], xv[:, 2]
    u = deviations(xv[:, 2])
    out = np.zeros(STRIDE, f64)
    out[0] = math.fsum(wh * wh)
    mx, my, mu = math.fsum(wh * x), math.fsum(wh * y), math.fsum(wh * u)
    out[1], out[2], out[3] = mx, my, th[0] + mu
    out[4], out[5] = math.fsum(wh * np.cos(th)), math.fsum(wh * np.sin(th))
    dx, dy, du = x - mx, y - my, u - mu
    for q, (a, b) in enumerate(((dx, dx), (dx, dy), (dy, dy), (dx, du), (dy, du), (du, du))):
        out[6 + q] = math.fsum(wh * a * b)
    for q, (a, b) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        out[12 + q] = math.fsum(wh * Pv[:, a, b])
    return out


def bounds(xv, Pv, out, N=None):
    """rounding bounds of the 18 entries for a set of N particles (tests/test_gpu_pose.py's docstring): k = 8 N u;
    [0] k out[0] | [1..2] k (D + |mu|) | [3] k (pi + |out[3]|) | [4..5] k + 4 u | xx, xy, yy k D (D + |mu|) | xu, yu k pi (2 D + |mu|) |
    uu 2 k pi^2 | [12..17] k max |Pv entry|"""
    xv, Pv = np.asarray(xv, f32).astype(f64), np.asarray(Pv, f32).astype(f64)
    N = len(xv) if N is None else N
    k = 8.0 * N * U
    D = max(np.ptp(xv[:, 0]), np.ptp(xv[:, 1]))
    mu = max(abs(out[1]), abs(out[2]))
    b = np.zeros(STRIDE, f64)
    b[0] = k * out[0]
    b[1:3] = k * (D + mu)
    b[3] = k * (math.pi + abs(out[3]))
    b[4:6] = k + 4.0 * U
    b[6:9] = k * D * (D + mu)
    b[9:11] = k * math.pi * (2.0 * D + mu)
    b[11] = 2.0 * k * math.pi ** 2
    b[12:18] = k * np.abs(Pv).max()
    return b


def covariance(out):
    """P = scatter + mean Pv as a 3 x 3 symmetric matrix"""
    s = np.asarray(out, f64)
    p = s[6:12] + s[12:18]
    return np.array([[p[0], p[1], p[3]], [p[1], p[2], p[4]], [p[3], p[4], p[5]]], f64)


def nees(summaries, xtrue):
    """(nees[count], err[count, 3], bad) of slamhost_pose_nees: e = (x- - x_t, y- - y_t, remainder(out[3] - theta_t, 2 pi)),
    NEES = e^T P^-1 e; NaN (and counted) where P is not positive definite or the summary holds a NaN"""
    S = np.asarray(summaries, f64).reshape(-1, STRIDE)
    T = np.asarray(xtrue, f32).astype(f64).reshape(-1, 3)
    val, err, bad = np.full(len(S), np.nan), np.full((len(S), 3), np.nan), 0
    for k, (s, t) in enumerate(zip(S, T)):
        e = np.array([s[1] - t[0], s[2] - t[1], math.remainder(s[3] - t[2], TWO_PI) if math.isfinite(s[3]) else np.nan])
        err[k] = e
        P = covariance(s)
        ok = np.isfinite(P).all() and np.isfinite(e).all()
        if ok:
            try:
                L = np.linalg.cholesky(P)
                yv = np.linalg.solve(L, e)
                val[k] = float(yv @ yv)
            except np.linalg.LinAlgError:
                ok = False
        if not ok or not math.isfinite(val[k]):
            val[k] = np.nan
            bad += 1
    return val, err, bad


def self_check():
    """sets with known answers"""
    # four particles placed symmetrically about (3, -2), equal weights, headings +-0.1 about 0.5, a common Pv
    d = 0.25
    xv = np.array([[3 + d, -2 + d, 0.6], [3 - d, -2 + d, 0.4], [3 - d, -2 - d, 0.6], [3 + d, -2 - d, 0.4]], f32)
    Pv = np.tile(np.array([[0.5, 0.125, 0.0], [0.125, 0.25, 0.0], [0.0, 0.0, 0.0625]], f32), (4, 1, 1))
    o = summary(xv, Pv, np.full(4, 0.25, f32))
    assert o[0] == 0.25 and abs(o[1] - 3.0) < 1e-15 and abs(o[2] + 2.0) < 1e-15 and abs(o[3] - 0.5) < 1e-7
    assert np.allclose(o[6:12], [d * d, 0.0, d * d, 0.0, 0.0, 0.01], atol=1e-8)  # xx, xy, yy, xu, yu, uu
    assert np.allclose(o[12:18], [0.5, 0.125, 0.25, 0.0, 0.0, 0.0625], atol=0)
    assert abs(math.atan2(o[5], o[4]) - 0.5) < 1e-7
    # weights in any scale, and as log-weights
    assert np.allclose(summary(xv, Pv, np.full(4, 7.0, f32)), o, rtol=1e-15, atol=1e-15)
    assert np.allclose(summary(xv, Pv, np.full(4, -800.0, f32), logw=True), o, rtol=1e-15, atol=1e-15)
    # headings straddling +-pi: uu is the small spread squared, not pi^2, and the mean heading wraps to +-pi
    s = 0.01
    xv2 = xv.copy()
    xv2[:, 2] = [math.pi - s, -math.pi + s, math.pi - s, -math.pi + s]
    o2 = summary(xv2, Pv, np.full(4, 0.25, f32))
    assert abs(o2[11] - s * s) < 1e-6 and o2[11] < 1e-3, o2[11]
    assert abs(abs(math.remainder(o2[3], TWO_PI)) - math.pi) < 1e-6
    assert math.hypot(o2[4], o2[5]) > 0.999 and abs(abs(math.atan2(o2[5], o2[4])) - math.pi) < 1e-6
    # ... and the same cloud half a turn away gives the same scatter (the pivot rule does not care where the cloud sits)
    xv3 = xv2.copy()
    xv3[:, 2] = [0.0 - s, 0.0 + s, 0.0 - s, 0.0 + s]
    assert np.allclose(summary(xv3, Pv, np.full(4, 0.25, f32))[6:12], o2[6:12], atol=1e-6)
    # a pending gather: pose through keep[], weight 1 / N
    keep = np.array([2, 2, 0, 1])
    a, b, c = present_set(xv, Pv, np.array([0.7, 0.1, 0.1, 0.1], f32), keep)
    assert np.array_equal(a, xv[keep]) and np.all(c == f32(0.25))
    og = summary(a, b, c)
    assert abs(og[1] - (3 - d + 3 - d + 3 + d + 3 - d) / 4) < 1e-15
    # uneven weights with a zero: the zero-weight particle does not move anything
    w = np.array([0.5, 0.0, 0.25, 0.25], f32)
    ow = summary(xv, Pv, w)
    far = xv.copy()
    far[1] = [1e6, -1e6, 2.0]
    assert np.allclose(summary(far, Pv, w), ow, rtol=0, atol=1e-12)
    assert abs(ow[0] - (0.25 + 0.0625 + 0.0625)) < 1e-15
    # N = 1: no scatter at all; degenerate weights: NaN everywhere
    o1 = summary(xv[:1], Pv[:1], np.ones(1, f32))
    assert o1[0] == 1.0 and np.all(o1[6:12] == 0.0) and o1[3] == float(xv[0, 2])
    for bad in (np.zeros(4, f32), np.array([1, np.inf, 1, 1], f32), np.array([1, np.nan, 1, 1], f32)):
        assert np.isnan(summary(xv, Pv, bad)).all()
    assert np.isnan(summary(xv, Pv, np.full(4, -np.inf, f32), logw=True)).all()
    # NEES: a diagonal P and a known e
    sm = np.zeros(STRIDE)
    sm[1:4] = [1.0, 2.0, 0.5]
    sm[[6, 8, 11]] = [0.04, 0.09, 0.01]       # scatter xx, yy, uu
    sm[[12, 14, 17]] = [0.0, 0.07, 0.0]       # mean Pv: P = diag(0.04, 0.16, 0.01)
    v, e, bad = nees(sm, [0.8, 2.4, 0.4])
    assert bad == 0 and np.allclose(e[0], [0.2, -0.4, 0.1], atol=1e-7) and abs(v[0] - (1.0 + 1.0 + 1.0)) < 1e-5
    # a heading error across +-pi
    sm2 = sm.copy()
    sm2[3] = math.pi - 0.05
    v, e, bad = nees(sm2, [1.0, 2.0, -math.pi + 0.05])
    assert bad == 0 and abs(e[0, 2] + 0.1) < 1e-6 and abs(v[0] - 1.0) < 1e-4
    # N = 1 (P = 0: not positive definite) and a NaN summary: NaN, counted
    o1 = summary(xv[:1], np.zeros((1, 3, 3), f32), np.ones(1, f32))
    v, e, bad = nees(np.stack([o1, NAN18]), np.zeros((2, 3), f32))
    assert bad == 2 and np.isnan(v).all()
    return True


if __name__ == "__main__":
    self_check()
    print("pose_model: ok")
