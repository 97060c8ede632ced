"""float64 model of slamgpu_innovation_summary and slamhost_innovation_nis, written from include/slamgpu.h and include/slamhost.h alone:
plain Python floats, math.sqrt / math.atan2 / math.remainder per particle, math.fsum (exactly rounded) for every sum over the particles.

summary(xv, w, xf, Pf, zf, idf, R, logw) takes what peek() returns (xv [N, 3], w [N], xf [N, nf, 2], Pf [N, nf, 2, 2], float32) and the
packet, and returns (out [m, 10], holders [m], terms): `terms` holds, per observation, what bounds() needs of the per-particle doubles.

bounds(terms, N) gives the rounding bounds of tests/test_gpu_innovation.py (derived in that file's docstring), nis(entries) mirrors
slamhost_innovation_nis, self_check() runs sets whose answers are known by hand."""
import math

import numpy as np

STRIDE = 10
TWO_PI = 6.283185307179586476925286766559   # the double nearest to 2 pi
U = 2.0 ** -53
NAN = float("nan")


def weights(w, logw):
    """w^_i; None where the weights sum to zero or to nothing finite"""
    w = [float(x) for x in np.asarray(w, np.float32)]
    if logw:
        M = max(w) if w else NAN
        if not M > -math.inf:     # (all -inf, or a NaN that max() let through below)
            return None
        w = [math.exp(x - M) if x == x else NAN for x in w]
    if any(x != x for x in w):
        return None
    tot = math.fsum(w) if all(math.isfinite(x) for x in w) else math.inf
    if not (tot > 0.0) or not (tot < math.inf):
        return None
    return [x / tot for x in w]


def term(pose, rec, P, zr, zb, R):
    """one particle's (v0, v1, s00, s10, s11, nis) and |H| |Pf| |H|^T + |R| entrywise (the size of the terms S is summed from), in the
    header's order; None for a particle outside H_q (record absent, or d2 == 0)"""
    x, y, th = (float(v) for v in pose)
    fx, fy = float(rec[0]), float(rec[1])
    if fx != fx:
        return None
    p00, p10, p11 = float(P[0][0]), float(P[1][0]), float(P[1][1])
    r00, r10, r11 = float(R[0]), float(R[2]), float(R[3])
    dx = fx - x
    dy = fy - y
    d2 = dx * dx + dy * dy
    if not d2 > 0.0:
        return None
    d = math.sqrt(d2)
    v0 = zr - d
    ang = math.atan2(dy, dx)
    v1 = math.remainder(zb - (ang - th), TWO_PI)
    h00, h01, h10, h11 = dx / d, dy / d, -dy / d2, dx / d2
    t0, t1 = h00 * p00 + h01 * p10, h00 * p10 + h01 * p11
    u0, u1 = h10 * p00 + h11 * p10, h10 * p10 + h11 * p11
    s00 = t0 * h00 + t1 * h01 + r00
    s10 = u0 * h00 + u1 * h01 + r10
    s11 = u0 * h10 + u1 * h11 + r11
    det = s00 * s11 - s10 * s10
    num = s11 * v0 * v0 - 2.0 * s10 * v0 * v1 + s00 * v1 * v1
    nis = num / det if det != 0.0 else (math.copysign(math.inf, num) if num != 0.0 else NAN)
    a00, a01, a10, a11 = abs(h00), abs(h01), abs(h10), abs(h11)
    q00, q10, q11 = abs(p00), abs(p10), abs(p11)
    m00 = (a00 * q00 + a01 * q10) * a00 + (a00 * q10 + a01 * q11) * a01 + abs(r00)
    m10 = (a10 * q00 + a11 * q10) * a00 + (a10 * q10 + a11 * q11) * a01 + abs(r10)
    m11 = (a10 * q00 + a11 * q10) * a10 + (a10 * q10 + a11 * q11) * a11 + abs(r11)
    return dict(v=(v0, v1), S=(s00, s10, s11), nis=nis, det=det, mag=(m00, m10, m11), d=d, ang=abs(ang) + abs(th) + abs(zb))


def summary(xv, w, xf, Pf, zf, idf, R, logw=False):
    xv, xf, Pf = np.asarray(xv, np.float32), np.asarray(xf, np.float32), np.asarray(Pf, np.float32)
    zf = np.asarray(zf, np.float32).reshape(-1, 2)
    idf = np.asarray(idf, np.int32).reshape(-1)
    R = np.asarray(R, np.float32).reshape(-1)
    N, m = len(xv), len(idf)
    wh = weights(w, logw)
    out = np.full((m, STRIDE), NAN)
    holders = np.zeros(m, np.int32)
    terms = []
    for q in range(m):
        l, zr, zb = int(idf[q]), float(zf[q, 0]), float(zf[q, 1])
        T = [(i, term(xv[i], xf[i, l], Pf[i, l], zr, zb, R)) for i in range(N)]
        T = [(i, t) for i, t in T if t is not None]
        holders[q] = len(T)
        terms.append(dict(T=[t for _, t in T], w=[wh[i] for i, _ in T] if wh is not None else None))
        if wh is None:
            continue
        s = math.fsum(wh[i] for i, _ in T)
        out[q, 0] = s
        if not T or not s > 0.0:
            continue
        m0 = math.fsum(wh[i] * t["v"][0] for i, t in T) / s
        m1 = math.fsum(wh[i] * t["v"][1] for i, t in T) / s
        out[q, 1], out[q, 2] = m0, m1
        out[q, 3] = math.fsum(wh[i] * (t["v"][0] - m0) * (t["v"][0] - m0) for i, t in T) / s
        out[q, 4] = math.fsum(wh[i] * (t["v"][0] - m0) * (t["v"][1] - m1) for i, t in T) / s
        out[q, 5] = math.fsum(wh[i] * (t["v"][1] - m1) * (t["v"][1] - m1) for i, t in T) / s
        for k in range(3):
            out[q, 6 + k] = math.fsum(wh[i] * t["S"][k] for i, t in T) / s
        ns = [wh[i] * t["nis"] for i, t in T]
        out[q, 9] = math.fsum(ns) / s if all(math.isfinite(x) for x in ns) else float(np.sum(ns)) / s
    return out, holders, terms


def bounds(terms, N, out):
    """[m, 10] rounding bounds of a correct double implementation against summary() (tests/test_gpu_innovation.py's docstring)"""
    m = len(terms)
    b = np.zeros((m, STRIDE))
    k = 8.0 * N * U
    for q in range(m):
        T, w = terms[q]["T"], terms[q]["w"]
        if not T or w is None or not math.fsum(w) > 0.0:
            continue
        T = [t for t, x in zip(T, w) if x > 0.0]   # (what carries weight: the rest adds exact zeros)
        v0 = [t["v"][0] for t in T]
        v1 = [t["v"][1] for t in T]
        D0, D1 = max(v0) - min(v0), max(v1) - min(v1)
        mu0, mu1 = abs(out[q, 1]), abs(out[q, 2])
        # per-term: sqrt within 2 ulps of d, then one subtraction; atan2 within 4 ulps, two subtractions at the size of their operands
        e0 = max(4.0 * U * t["d"] for t in T) + 2.0 * U * max(abs(x) for x in v0)
        e1 = max(8.0 * U * t["ang"] for t in T)
        b[q, 0] = k
        b[q, 1] = k * (D0 + mu0) + e0
        b[q, 2] = k * (D1 + mu1) + e1
        b[q, 3] = k * D0 * (D0 + mu0) + 2.0 * D0 * e0 + e0 * e0
        b[q, 4] = k * (D0 * (D1 + mu1) + D1 * (D0 + mu0)) + D0 * e1 + D1 * e0 + e0 * e1
        b[q, 5] = k * D1 * (D1 + mu1) + 2.0 * D1 * e1 + e1 * e1
        # S: 4 divisions (each carrying sqrt's ulps), 12 products and 9 sums from float32 inputs: 16 u at the size of the terms it is summed from
        dS = [max(16.0 * U * t["mag"][j] for t in T) for j in range(3)]
        for j in range(3):
            b[q, 6 + j] = k * max(abs(t["S"][j]) for t in T) + dS[j]
        # nis = num / det: the errors of v and S through num, and through det at 1 / det -- the conditioning of S_i, from the model's S_i
        dn = 0.0
        for t in T:
            a0, a1 = abs(t["v"][0]), abs(t["v"][1])
            s00, s10, s11 = t["S"]
            m00, m10, m11 = (16.0 * U * x for x in t["mag"])
            num_abs = abs(s11) * a0 * a0 + 2.0 * abs(s10) * a0 * a1 + abs(s00) * a1 * a1
            dnum = a0 * a0 * m11 + 2.0 * a0 * a1 * m10 + a1 * a1 * m00 + (2.0 * abs(s11) * a0 + 2.0 * abs(s10) * a1) * e0 + \
                (2.0 * abs(s10) * a0 + 2.0 * abs(s00) * a1) * e1 + 8.0 * U * num_abs
            ddet = abs(s00) * m11 + abs(s11) * m00 + 2.0 * abs(s10) * m10 + 4.0 * U * (abs(s00 * s11) + s10 * s10)
            det = abs(t["det"])
            dn = max(dn, (dnum + abs(t["nis"]) * ddet) / det + 2.0 * U * abs(t["nis"])) if det > 0.0 else math.inf
        b[q, 9] = k * max(abs(t["nis"]) for t in T) + dn
    return b


def nis(entries):
    """slamhost_innovation_nis: (nis [count], bad)"""
    e = np.asarray(entries, np.float64).reshape(-1, STRIDE)
    out, bad = np.full(len(e), NAN), 0
    for k, s in enumerate(e):
        v = NAN
        if s[0] > 0.0 and not np.isnan(s).any():
            p00, p10, p11 = float(s[3] + s[6]), float(s[4] + s[7]), float(s[5] + s[8])
            if p00 > 0.0 and math.isfinite(p00):
                l00 = math.sqrt(p00)
                l10 = p10 / l00
                d1 = p11 - l10 * l10
                if d1 > 0.0 and math.isfinite(d1):
                    l11 = math.sqrt(d1)
                    y0 = float(s[1]) / l00
                    y1 = (float(s[2]) - l10 * y0) / l11
                    v = y0 * y0 + y1 * y1
        if not math.isfinite(v):
            v, bad = NAN, bad + 1
        out[k] = v
    return out, bad


# ---- sets whose answers are known -----------------------------------------------------------------------------------------------------
def known_sets():
    """name -> (xv, w, xf, Pf, zf, idf, R, logw); the answers are in self_check().  Every number is a float32, so that an upload of the set
    holds exactly these values"""
    f = np.float32
    R = np.array([0.01, 0.0, 0.0, 0.0004], f)
    th = float(f(0.1))
    P1 = np.array([[0.04, 0.0], [0.0, 0.09]], f)
    sets = {}
    # four particles placed symmetrically about the origin on the line to the landmark at (10, 0), headings +-0.1
    xv = np.array([[1, 0, th], [1, 0, -th], [-1, 0, th], [-1, 0, -th]], f)
    sets["symmetric"] = (xv, np.full(4, 0.25, f), np.tile(np.array([10.0, 0.0], f), (4, 1, 1)), np.tile(P1, (4, 1, 1, 1)), np.array([[10.0, 0.0]], f), [0], R, False)
    # a landmark dead ahead (slot 0) and one behind the vehicle, a hair to the right (slot 1: its bearing is just above -pi, measured as just below +pi)
    xv = np.array([[0.0, 0.0, 0.0]], f)
    xf = np.array([[[5.0, 0.0], [-5.0, -0.001]]], f)
    sets["ahead_behind"] = (xv, np.ones(1, f), xf, np.tile(P1, (1, 2, 1, 1)), np.array([[5.5, 0.01], [5.0, float(f(math.pi)) - 0.01]], f), [0, 1], R, False)
    # a slot held by half the weight (the weights are not normalised)
    xv = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], f)
    xf = np.array([[[4.0, 3.0]], [[np.nan, np.nan]]], f)
    Pf = np.array([[P1], [np.full((2, 2), np.nan)]], f)
    sets["half"] = (xv, np.array([0.25, 0.25], f), xf, Pf, np.array([[5.0, float(f(math.atan2(3.0, 4.0)))]], f), [0], R, False)
    # N = 1
    sets["one"] = (np.array([[1.0, 2.0, 0.5]], f), np.array([0.3], f), np.array([[[4.0, 6.0]]], f), np.array([[P1]], f), np.array([[5.25, 0.4]], f), [0], R, False)
    # degenerate weights: all zero, one infinite
    sets["zero_weights"] = (sets["symmetric"][0], np.zeros(4, f)) + sets["symmetric"][2:]
    sets["inf_weight"] = (sets["symmetric"][0], np.array([0.25, np.inf, 0.25, 0.25], f)) + sets["symmetric"][2:]
    return sets


def check_known(name, out, holders, tol=1e-13):
    """the hand answers of known_sets()[name] against a summary (the model's, or the device's): relative to each answer's own size"""
    f = np.float32
    th = float(f(0.1))
    r00, r11 = float(f(0.01)), float(f(0.0004))
    p00, p11 = float(f(0.04)), float(f(0.09))

    def near(got, exp, what):
        assert abs(got - exp) <= tol * max(1.0, abs(exp)), (name, what, got, exp)
    if name == "symmetric":
        assert holders[0] == 4
        near(out[0, 0], 1.0, "share")
        near(out[0, 1], 0.0, "mean v0")          # v0 = +1, +1, -1, -1
        near(out[0, 2], 0.0, "mean v1")          # v1 = theta: +-0.1
        near(out[0, 3], 1.0, "rr")
        near(out[0, 4], 0.0, "rb")
        near(out[0, 5], th * th, "bb")
        near(out[0, 6], p00 + r00, "s00")        # dy = 0: H = diag(1, 1 / d)
        near(out[0, 7], 0.0, "s10")
        s11 = (p11 / 81.0 + r11, p11 / 121.0 + r11)
        near(out[0, 8], 0.5 * (s11[0] + s11[1]), "s11")
        near(out[0, 9], 1.0 / (p00 + r00) + 0.5 * (th * th / s11[0] + th * th / s11[1]), "mean nis")
    elif name == "ahead_behind":
        assert list(holders) == [1, 1]
        near(out[0, 1], 0.5, "ahead v0")
        near(out[0, 2], float(f(0.01)), "ahead v1")
        assert np.all(out[:, 3:6] == 0.0) and np.all(out[:, 0] == 1.0)
        assert abs(out[1, 2]) < 0.02 and abs(out[1, 1]) < 1e-6, (name, "behind: v1 wrapped the wrong way", out[1])
        near(out[1, 2], (float(f(float(f(math.pi)) - 0.01)) - 2.0 * math.pi) - (math.atan2(-float(f(0.001)), -5.0)), "behind v1")
    elif name == "half":
        assert holders[0] == 1
        near(out[0, 0], 0.5, "share")
        near(out[0, 1], 0.0, "v0")
        assert abs(out[0, 2]) < 1e-7 and np.all(out[0, 3:6] == 0.0)
    elif name == "one":
        assert holders[0] == 1 and out[0, 0] == 1.0 and np.all(out[0, 3:6] == 0.0), (name, out[0])
        near(out[0, 1], 0.25, "v0")
        near(out[0, 2], float(f(0.4)) - (math.atan2(4.0, 3.0) - 0.5), "v1")
    else:
        assert holders[0] == 4 and np.isnan(out).all(), (name, out, holders)


def self_check():
    for name, (xv, w, xf, Pf, zf, idf, R, logw) in known_sets().items():
        out, holders, _ = summary(xv, w, xf, Pf, zf, idf, R, logw)
        check_known(name, out, holders)
    # nis(): a diagonal P by hand, a share of 0, a P that is not positive definite, a NaN
    e = np.array([[1.0, 0.3, -0.2, 0.01, 0.0, 0.02, 0.09, 0.0, 0.03, 2.0],
                  [0.0] + [NAN] * 9,
                  [1.0, 0.3, -0.2, 0.01, 0.5, 0.02, 0.09, 0.0, 0.03, 2.0],
                  [1.0, 0.3, -0.2, 0.01, 0.0, NAN, 0.09, 0.0, 0.03, 2.0]])
    v, bad = nis(e)
    assert abs(v[0] - (0.09 / 0.1 + 0.04 / 0.05)) < 1e-14 and np.isnan(v[1:]).all() and bad == 3, (v, bad)
    return True
