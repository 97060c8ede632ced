"""A float64 numpy model of slamgpu_joint_summary on peek(first=0, stride=1, count=N) of the same context taken immediately before
the call: the definitions of include/slamgpu.h evaluated directly (float32 poses, records and weights promoted to float64, numpy's
pairwise sums), and the rounding bounds of tests/test_gpu_joint.py.  The weight handling and the particle sums are those of
tests/test_gpu_map_summary.py (exp(l - max l) for log-weights, normalised over ALL particles; _psum)."""
import math

import numpy as np

from test_gpu_map_summary import _psum

f64 = np.float64
U = 2.0 ** -53
TWO_PI = 2.0 * np.pi


def joint_size(k):
    D = 3 + 2 * k
    return 1 + D + D * (D + 1) // 2 + 6 + 3 * k


def vectors(pk, slots):
    """v[N, D] in the EKF's ordering and J[N]: the particles that hold every listed slot"""
    slots = np.asarray(slots, np.int64).reshape(-1)
    xv = pk["xv"].astype(f64)
    N = len(xv)
    u = np.array([math.remainder(t, TWO_PI) for t in xv[:, 2] - xv[0, 2]], f64)   # (the IEEE remainder, as the header has it)
    cols = [xv[:, 0], xv[:, 1], u]
    J = np.ones(N, bool)
    if len(slots):
        xf = pk["xf"].astype(f64)[:, slots, :]
        J = ~np.isnan(xf[:, :, 0]).any(axis=1)
        for s in range(len(slots)):
            cols += [xf[:, s, 0], xf[:, s, 1]]
    return np.stack(cols, axis=1), J


def weights(pk, logw):
    w = pk["w"].astype(f64)
    if logw:
        w = np.exp(w - w.max())
    with np.errstate(all="ignore"):
        return w / w.sum()


def model(pk, logw, slots):
    """the call's outputs (share, mean[D], scatter[D, D], pv[6], pf[k, 3], both) and what the bounds need (range[D], mu[D], Pv_max,
    Pf_max[k])"""
    slots = np.asarray(slots, np.int64).reshape(-1)
    k, D = len(slots), 3 + 2 * len(slots)
    v, J = vectors(pk, slots)
    wh = weights(pk, logw)
    nan = np.full(D, np.nan)
    with np.errstate(all="ignore"):
        W = np.where(J, wh, 0.0)
        share = float(_psum(W[:, None])[0])
        both = int(J.sum())
        if not np.isfinite(wh).all():   # the weights sum to zero or to nothing finite
            return dict(share=np.nan, mean=nan, scatter=np.full((D, D), np.nan), pv=np.full(6, np.nan), pf=np.full((k, 3), np.nan), both=both,
                        range=np.zeros(D), mu=np.zeros(D), Pv_max=0.0, Pf_max=np.zeros(k))
        if both == 0 or share == 0.0:
            return dict(share=share, mean=nan, scatter=np.full((D, D), np.nan), pv=np.full(6, np.nan), pf=np.full((k, 3), np.nan), both=both,
                        range=np.zeros(D), mu=np.zeros(D), Pv_max=0.0, Pf_max=np.zeros(k))
        vj = np.where(J[:, None], v, 0.0)
        mean = _psum(W[:, None] * vj) / share
        d = np.where(J[:, None], v - mean[None, :], 0.0)
        scatter = np.empty((D, D))
        for a in range(D):
            scatter[a] = _psum(W[:, None] * d[:, a:a + 1] * d) / share
        Pv = pk["Pv"].astype(f64)
        pvs = np.stack([Pv[:, 0, 0], Pv[:, 1, 0], Pv[:, 1, 1], Pv[:, 2, 0], Pv[:, 2, 1], Pv[:, 2, 2]], axis=1)
        pvs = np.where(J[:, None], pvs, 0.0)
        pv = _psum(W[:, None] * pvs) / share
        pf, Pf_max = np.zeros((k, 3)), np.zeros(k)
        if k:
            Pf = pk["Pf"].astype(f64)[:, slots]
            pfs = np.where(J[:, None, None], np.stack([Pf[:, :, 0, 0], Pf[:, :, 1, 0], Pf[:, :, 1, 1]], axis=2), 0.0)
            pf = np.stack([_psum(W[:, None] * pfs[:, :, q]) / share for q in range(3)], axis=1)
            Pf_max = np.abs(np.where(J[:, None, None, None], Pf, 0.0)).max(axis=(0, 2, 3))
        rng = v[J].max(axis=0) - v[J].min(axis=0)
        mean_out = mean.copy()
        mean_out[2] += float(pk["xv"][0, 2])
    return dict(share=share, mean=mean_out, scatter=scatter, pv=pv, pf=pf, both=both, range=rng, mu=np.abs(mean_out), Pv_max=float(np.abs(pvs).max()),
                Pf_max=Pf_max)


def brute(pk, logw, slots):
    """the same definitions as plain Python loops over particles and coordinates (tests/test_joint_cpu.py holds the model to it)"""
    slots = [int(s) for s in slots]
    k, D = len(slots), 3 + 2 * len(slots)
    w = [float(x) for x in pk["w"]]
    if logw:
        top = max(w)
        w = [float(np.exp(x - top)) for x in w]
    tot = sum(w)
    th0 = float(pk["xv"][0, 2])
    rows, ws, pvs, pfs = [], [], [], []
    for i in range(len(w)):
        if any(np.isnan(pk["xf"][i, s, 0]) for s in slots):
            continue
        u = float(np.float64(pk["xv"][i, 2]) - th0)
        u = u - TWO_PI * round(u / TWO_PI)
        row = [float(pk["xv"][i, 0]), float(pk["xv"][i, 1]), u]
        for s in slots:
            row += [float(pk["xf"][i, s, 0]), float(pk["xf"][i, s, 1])]
        rows.append(row)
        ws.append(w[i] / tot)
        P = pk["Pv"][i]
        pvs.append([float(P[0, 0]), float(P[1, 0]), float(P[1, 1]), float(P[2, 0]), float(P[2, 1]), float(P[2, 2])])
        pfs.append([[float(pk["Pf"][i, s, 0, 0]), float(pk["Pf"][i, s, 1, 0]), float(pk["Pf"][i, s, 1, 1])] for s in slots])
    share = sum(ws)
    mean = [sum(wi * r[a] for wi, r in zip(ws, rows)) / share for a in range(D)]
    scatter = [[sum(wi * (r[a] - mean[a]) * (r[b] - mean[b]) for wi, r in zip(ws, rows)) / share for b in range(D)] for a in range(D)]
    pv = [sum(wi * p[q] for wi, p in zip(ws, pvs)) / share for q in range(6)]
    pf = [[sum(wi * p[s][q] for wi, p in zip(ws, pfs)) / share for q in range(3)] for s in range(k)]
    mean[2] += th0
    return dict(share=share, mean=np.array(mean), scatter=np.array(scatter).reshape(D, D), pv=np.array(pv), pf=np.array(pf).reshape(k, 3), both=len(rows))


def bounds(m, N):
    """the rounding bounds of tests/test_gpu_joint.py's docstring"""
    c = 8.0 * N * U
    r = m["range"]
    return dict(share=c, mean=c * (r + m["mu"]), scatter=c * np.outer(r, r), pv=c * m["Pv_max"], pf=c * m["Pf_max"][:, None] * np.ones((1, 3)))


def compare(got, m, N, tag):
    """the call's answer against the model within the bounds; prints the worst error / bound of each quantity first; returns the ratios"""
    b = bounds(m, N)
    report, bad, ratios = [], [], {}
    for q in ("share", "mean", "scatter", "pv", "pf"):
        g, e = np.asarray(got[q], f64), np.asarray(m[q], f64)
        assert g.shape == e.shape, (tag, q, g.shape, e.shape)
        with np.errstate(all="ignore"):
            err = np.abs(g - e)
        bound = np.broadcast_to(np.asarray(b[q], f64), err.shape)
        some = ~np.isnan(e)
        ratio = np.where(some & (err > 0), err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
        ratios[q] = float(ratio.max()) if ratio.size else 0.0
        report.append("%s %.3g (err %.3g)" % (q, ratios[q], float(np.nanmax(err)) if some.any() and err.size else 0.0))
        if not np.array_equal(np.isnan(g), np.isnan(e)):
            bad.append(q + ": NaN pattern")
        elif not np.all(err[some] <= bound[some]):
            bad.append(q + ": outside its bound")
    print("joint_summary %s: N %d, D %d, |J| %d; worst error / bound: %s" % (tag, N, len(m["mean"]), m["both"], ", ".join(report)))
    assert got["both"] == m["both"], (tag, got["both"], m["both"])
    assert not bad, (tag, bad)
    return ratios
