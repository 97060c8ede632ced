"""float64 model of slamgpu_innovation_summary_labels, written from include/slamgpu.h alone: tests/innovation_model.py with the slot of
an observation taken per particle.  Its weights, per-particle term, bounds and NIS are innovation_model's own (one copy); only the choice
of the record differs, so unanimous labels give innovation_model.summary's floats exactly.

summary_labels(xv, w, xf, Pf, z, labels, R, logw) takes what peek() returns (xv [N, 3], w [N], xf [N, nf, 2], Pf [N, nf, 2, 2], float32),
the observations z [nz, 2] and labels [N, nz] (a slot, NEW = -1, DISCARD = -2; anything outside [0, nf) is "no slot"), and returns
(out [nz, 10], holders [nz], terms) exactly as innovation_model.summary does, `terms` being what bounds() needs."""
import math

import numpy as np

from innovation_model import NAN, STRIDE, bounds, nis, term, weights  # noqa: F401  (bounds, nis: re-exported for the tests)

NEW, DISCARD = -1, -2
SLOT_PER_PARTICLE = -3   # SLAMGPU_INNOV_SLOT_PER_PARTICLE


def summary_labels(xv, w, xf, Pf, z, labels, R, logw=False):
    xv, xf, Pf = np.asarray(xv, np.float32), np.asarray(xf, np.float32), np.asarray(Pf, np.float32)
    z = np.asarray(z, np.float32).reshape(-1, 2)
    N, nz = len(xv), len(z)
    labels = np.asarray(labels, np.int32).reshape(N, nz)
    R = np.asarray(R, np.float32).reshape(-1)
    nf = xf.shape[1] if xf.ndim == 3 else 0
    wh = weights(w, logw)
    out = np.full((nz, STRIDE), NAN)
    holders = np.zeros(nz, np.int32)
    terms = []
    for q in range(nz):
        zr, zb = float(z[q, 0]), float(z[q, 1])
        T = []
        for i in range(N):
            l = int(labels[i, q])
            if not 0 <= l < nf:     # NEW, DISCARD, anything else: outside H_q, never an index
                continue
            t = term(xv[i], xf[i, l], Pf[i, l], zr, zb, R)
            if t is not None:
                T.append((i, t))
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


def hand_set():
    """4 particles, 3 slots, 2 observations, every number a float32 and simple enough to work by hand (hand_answers()).
    All poses at the origin heading 0; Pf = diag(0.04, 0.09), R = diag(0.01, 0.0004); weights 1, 2, 3, 2 (not normalised).
      slot 0 at (10, 0), slot 1 at (0, 5) -- absent in particle 2 -- slot 2 at (-4, 0).
      observation 0 = (range 10.5, bearing 0):  particle 0 -> slot 0, particle 1 -> NEW, particle 2 -> slot 1 (which it holds absent),
                                                 particle 3 -> slot 2
      observation 1 = (range 5, bearing 0.25):  DISCARD, NEW, DISCARD, NEW: nobody matched"""
    f = np.float32
    N = 4
    xv = np.zeros((N, 3), f)
    xf = np.tile(np.array([[10.0, 0.0], [0.0, 5.0], [-4.0, 0.0]], f), (N, 1, 1))
    Pf = np.tile(np.array([[0.04, 0.0], [0.0, 0.09]], f), (N, 3, 1, 1))
    xf[2, 1] = np.nan
    Pf[2, 1] = np.nan
    w = np.array([1.0, 2.0, 3.0, 2.0], f)
    z = np.array([[10.5, 0.0], [5.0, 0.25]], f)
    labels = np.array([[0, DISCARD], [NEW, NEW], [1, DISCARD], [2, NEW]], np.int32)
    R = np.array([0.01, 0.0, 0.0, 0.0004], f)
    return xv, w, xf, Pf, z, labels, R


def hand_answers():
    """(out [2, 10], holders [2]) of hand_set(), worked from the header's formula.
    Observation 0: H_0 = {particle 0 (w^ = 1/8, slot 0), particle 3 (w^ = 2/8, slot 2)}; share 3/8; inside H_0 the weights are 1/3, 2/3.
      particle 0: dx = 10, dy = 0: d = 10, v = (0.5, 0); H = diag(1, 1/10): S = (p00 + r00, 0, p11 / 100 + r11)
      particle 3: dx = -4, dy = 0: d = 4, atan2 = pi (the double): v0 = 6.5, v1 = remainder(-pi, 2 pi) = -pi (the quotient -1/2 is a
                  tie and rounds to the even 0); H = diag(-1, -1/4): S = (p00 + r00, 0, p11 / 16 + r11)
      p10 = 0 and s10 = 0 make nis_i = v0^2 / s00 + v1^2 / s11.
    Observation 1: nobody: share 0, the rest NaN."""
    f = np.float32
    p00, p11, r00, r11 = float(f(0.04)), float(f(0.09)), float(f(0.01)), float(f(0.0004))
    v1_3 = math.remainder(0.0 - (math.pi - 0.0), 6.283185307179586476925286766559)
    a, b = 1.0 / 3.0, 2.0 / 3.0
    va, vb = (0.5, 0.0), (6.5, v1_3)
    m0, m1 = a * va[0] + b * vb[0], a * va[1] + b * vb[1]
    out = np.full((2, STRIDE), NAN)
    out[0, 0] = 3.0 / 8.0
    out[0, 1], out[0, 2] = m0, m1
    out[0, 3] = a * (va[0] - m0) ** 2 + b * (vb[0] - m0) ** 2
    out[0, 4] = a * (va[0] - m0) * (va[1] - m1) + b * (vb[0] - m0) * (vb[1] - m1)
    out[0, 5] = a * (va[1] - m1) ** 2 + b * (vb[1] - m1) ** 2
    s11a, s11b = p11 / 100.0 + r11, p11 / 16.0 + r11
    out[0, 6] = p00 + r00
    out[0, 7] = 0.0
    out[0, 8] = a * s11a + b * s11b
    out[0, 9] = a * (0.25 / (p00 + r00)) + b * (6.5 * 6.5 / (p00 + r00) + v1_3 * v1_3 / s11b)
    out[1, 0] = 0.0
    return out, np.array([2, 0], np.int32)
