"""A float64 model of slamgpu_ens_moments (include/slamgpu.h), in the header's order of sums: tiles of 256 consecutive members, every
sum over members in ascending member order within a tile, the tiles in ascending order.  (The device puts four members through one
matrix instruction, whose inner order is the hardware's: on data whose sums are exact the two agree bit for bit, on generic data within
the bounds `bounds` gives.)"""
import math

import numpy as np

TILE = 256
TWO_PI = 2.0 * math.pi
U = 2.0 ** -53
FACTOR = 8.0


def select(x, P, dims, status, D, exclude=0):
    """the set J as a boolean array: dim >= D, no excluded status bit, x[0:D] finite, the diagonal of P over [0, D) finite"""
    x, P = np.asarray(x), np.asarray(P)
    diag = P[:, np.arange(D), np.arange(D)]
    return (np.asarray(dims) >= D) & ((np.asarray(status).astype(np.int64) & int(exclude)) == 0) & np.isfinite(x[:, :D]).all(axis=1) & np.isfinite(diag).all(axis=1)


def deviations(x, J, D):
    """(pivot member, pivot vector [D], v [B, D]): v_b = x_b - x_pivot in double, the heading through the IEEE remainder; rows outside J
    are zero"""
    members = np.flatnonzero(J)
    piv = int(members[0])
    xp = np.asarray(x[piv, :D], np.float64)
    v = np.zeros((x.shape[0], D))
    for b in members:
        xb = np.asarray(x[b, :D], np.float64)
        v[b] = xb - xp
        v[b, 2] = math.remainder(xb[2] - xp[2], TWO_PI)
    return piv, xp, v


def wrap(th):
    """into (-pi, pi], as slamhost_joint_dense wraps"""
    th = math.remainder(th, TWO_PI)
    return th + TWO_PI if th <= -TWO_PI / 2 else th


def mirror(A):
    """the lower triangle copied over the upper one (no arithmetic: the bits of the lower entries)"""
    out = A.copy()
    iu = np.triu_indices(A.shape[0], 1)
    out[iu] = A.T[iu]
    return out


def moments(x, P, dims, status, D, exclude=0):
    """x [B, >= D] and P [B, >= D, >= D] in float32 (what lies beyond a member's own dimension is never read for a member of J beyond
    D).  Returns a dict of mean, C, Pbar, counted, left_out, pivot and, for the bounds, v [n, D] (the deviations of J's members)"""
    x, P = np.asarray(x), np.asarray(P)
    B = x.shape[0]
    J = select(x, P, dims, status, D, exclude)
    n = int(J.sum())
    if n == 0:
        nan = np.full((D, D), np.nan)
        return dict(mean=np.full(D, np.nan), C=nan, Pbar=nan.copy(), counted=0, left_out=B, pivot=-1, v=np.zeros((0, D)))
    piv, xp, v = deviations(x, J, D)
    S, s1, SP = np.zeros((D, D)), np.zeros(D), np.zeros((D, D))
    for t0 in range(0, B, TILE):
        St, s1t, SPt = np.zeros((D, D)), np.zeros(D), np.zeros((D, D))
        for b in range(t0, min(B, t0 + TILE)):
            if J[b]:
                St += np.outer(v[b], v[b])
                s1t += v[b]
                SPt += P[b, :D, :D].astype(np.float64)
        S += St
        s1 += s1t
        SP += SPt
    delta = s1 / n
    mean = xp + delta
    mean[2] = wrap(mean[2])
    C = mirror(S / n - np.outer(delta, delta))
    Pbar = mirror(SP / n)
    return dict(mean=mean, C=C, Pbar=Pbar, counted=n, left_out=B - n, pivot=piv, v=v[J])


def bounds(m, P_max):
    """The error bounds of the generic-data tests, u = 2^-53, factor 8 (the form of tests/test_gpu_joint.py's): a sum of n terms in
    double, in whatever order, is within n u sum |terms| of the exact one to first order; the terms of the mean are at most R_a, the
    component's range over J (|v| <= R: v is taken from a member of J), those of the scatter R_a R_b, those of Pbar max |P_ab|; dividing
    by n leaves n u R.  The mean also carries the pivot's own value: R_a + |mu_a|.  Returns (mean [D], C [D, D], Pbar scalar)"""
    n, v = m["counted"], m["v"]
    R = v.max(axis=0) - v.min(axis=0)
    return FACTOR * n * U * (R + np.abs(m["mean"])), FACTOR * n * U * np.outer(R, R), FACTOR * n * U * P_max
