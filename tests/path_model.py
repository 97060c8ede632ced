"""Float64 numpy model of the path posterior (include/slamgpu.h: slamgpu_path_*): from the records (pose, parent), the origin array and
the present weights it returns lineages, traces, the seven sums of slamgpu_path_summary and the distinct-ancestor counts.

Lineage by index composition: a(R - 1, i) = origin[i], a(r - 1, i) = parent_r[a(r, i)].  Sums per record through the descendants'
weight W_r[k] = sum of w^_i over the present particles i with a(r, i) = k (np.bincount) and numpy's pairwise sums over k.  No GPU, no
library: tests/test_path_cpu.py checks it against a brute-force enumeration of descendants."""
import numpy as np

f64 = np.float64


def lineages(records, origin):
    """a[r, i] for the records given (oldest first); records: sequence of (pose[N, 3], parent[N])"""
    R = len(records)
    a = np.zeros((R, len(origin)), np.int64)
    if R == 0:
        return a
    a[R - 1] = np.asarray(origin, np.int64)
    for r in range(R - 1, 0, -1):
        a[r - 1] = np.asarray(records[r][1], np.int64)[a[r]]
    return a


def trace(records, origin, particle):
    """(xyt[R, 3] in the records' own dtype, index[R]) of the path present particle `particle` descends from"""
    a = lineages(records, origin)[:, particle]
    xyt = np.stack([np.asarray(records[r][0])[a[r]] for r in range(len(records))]) if len(records) else np.zeros((0, 3), np.float32)
    return xyt, a.astype(np.int32)


def normalised(w, logw=False):
    """w^_i of the header: linear weights over their sum; log-weights: exp(l - max l) over its sum"""
    w = np.asarray(w).astype(f64)
    with np.errstate(all="ignore"):
        if logw:
            w = np.exp(w - w.max())
        return w / w.sum()


def summary(records, origin, w, logw=False):
    """mean[R, 2], scatter[R, 3] (xx, xy, yy about the mean), cs[R, 2] (sum w^ cos, sum w^ sin), distinct[R]; and for the tests' bounds
    D[R] (the larger coordinate range of the ancestors' poses) and mu[R] (the larger coordinate of the mean).  Weights that sum to zero or
    to nothing finite: every float NaN, distinct still exact"""
    R, N = len(records), len(origin)
    a = lineages(records, origin)
    wh = normalised(w, logw)
    ok = bool(np.isfinite(wh).all())
    mean, scatter, cs = np.full((R, 2), np.nan), np.full((R, 3), np.nan), np.full((R, 2), np.nan)
    distinct, D, mu = np.zeros(R, np.int32), np.zeros(R), np.zeros(R)
    for r in range(R):
        pose = np.asarray(records[r][0]).astype(f64)
        cnt = np.bincount(a[r], minlength=N)
        distinct[r] = np.count_nonzero(cnt)
        anc = cnt > 0
        D[r] = max(np.ptp(pose[anc, 0]), np.ptp(pose[anc, 1]))
        if not ok:
            continue
        W = np.bincount(a[r], weights=wh, minlength=N)
        # about a pivot inside the ancestors' cloud (float32 coordinates: the differences are exact in float64), so that the model's own
        # rounding is at the size of the cloud, not of its distance from the origin: one ancestor gives its pose and a scatter of exactly 0
        px, py = pose[np.argmax(anc)][:2]
        Ws = np.sum(W)
        mx, my = px + np.sum(W * (pose[:, 0] - px)) / Ws, py + np.sum(W * (pose[:, 1] - py)) / Ws
        dx, dy = np.where(anc, pose[:, 0] - mx, 0.0), np.where(anc, pose[:, 1] - my, 0.0)
        mean[r] = mx, my
        scatter[r] = np.sum(W * dx * dx), np.sum(W * dx * dy), np.sum(W * dy * dy)
        cs[r] = np.sum(W * np.cos(pose[:, 2])), np.sum(W * np.sin(pose[:, 2]))
        mu[r] = max(abs(mx), abs(my))
    return dict(mean=mean, scatter=scatter, cs=cs, distinct=distinct, D=D, mu=mu)
