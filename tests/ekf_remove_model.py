"""Model of slamgpu_ekf_remove / slamhost_ekf_remove and of the per-feature counts (include/slamgpu.h), in numpy and plain integers.

Removal: src is the ascending list of the surviving state indices (0, 1, 2, then the two entries of every kept feature), s0 = 3 + 2 x
the first removed feature, and

    x'[i]    = x[src[i]]
    P'[i][j] = P[src[max(i, j)]][src[min(i, j)]]   wherever max(i, j) >= s0; entries with both indices below s0 stay as they are

that is P[np.ix_(src, src)] of the LOWER triangle mirrored: for a symmetric P simply P[np.ix_(src, src)].

Counts: epoch advances with every successful sim that observes and every successful direct update; the call in progress counts at
epoch + 1.  hits[f]: observations handed to the update stage; born[f]: the epoch of the append; last[f]: of the latest hit, else born."""
import numpy as np


def valid(nf, features):
    """ascending, distinct, each in [0, nf)"""
    f = np.asarray(features, np.int64).reshape(-1)
    return bool(((f >= 0) & (f < nf)).all() and (np.diff(f) > 0).all())


def src_map(nf, features):
    keep = np.setdiff1d(np.arange(nf), np.asarray(features, np.int64))
    return np.concatenate([np.arange(3), np.stack([3 + 2 * keep, 4 + 2 * keep], axis=1).reshape(-1)]).astype(np.int64)


def renumber(nf, features):
    """[nf]: the new index of every feature, -1 removed"""
    out = np.full(nf, -1, np.int64)
    keep = np.setdiff1d(np.arange(nf), np.asarray(features, np.int64))
    out[keep] = np.arange(keep.shape[0])
    return out


def gather(x, P, features):
    """(x', P') of a removal from the state x[D], P[D][D]; nothing is changed in place"""
    x, P = np.asarray(x), np.asarray(P)
    nf = (x.shape[0] - 3) // 2
    features = np.asarray(features, np.int64).reshape(-1)
    assert valid(nf, features)
    if features.shape[0] == 0:
        return x.copy(), P.copy()
    src, s0 = src_map(nf, features), 3 + 2 * int(features[0])
    low = np.tril(P) + np.tril(P, -1).T
    out = low[np.ix_(src, src)]
    out[:s0, :s0] = P[:s0, :s0]
    return x[src].copy(), out


def distinct_state(nf, asymmetric=False):
    """x and P (float32) with a value of its own in every entry of x and for every unordered pair (i, j) of P -- every ORDERED pair with
    asymmetric -- all exactly representable, so that a misplaced element shows"""
    D = 3 + 2 * nf
    i, j = np.meshgrid(np.arange(D), np.arange(D), indexing="ij")
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    P = (1 + hi * (hi + 1) // 2 + lo).astype(np.float64)
    assert P.max() < 2 ** 23
    if asymmetric:
        P = np.where(i < j, -P, P)
    return (-(1.0 + np.arange(D)) / 4).astype(np.float32), P.astype(np.float32)


class Counters:
    """the integer model of slamgpu_ekf_feature_stats"""

    def __init__(self, batch_update=True):
        self.batch_update = batch_update
        self.epoch = 0
        self.hits, self.born, self.last = [], [], []

    def upload(self, nf):
        self.hits, self.born, self.last = [0] * nf, [self.epoch] * nf, [self.epoch] * nf

    def _seen(self, idf, at):
        for f in idf:
            self.hits[int(f)] += 1
            self.last[int(f)] = at

    def _append(self, n, at):
        self.hits += [0] * n
        self.born += [at] * n
        self.last += [at] * n

    def update(self, idf):
        """a successful direct update"""
        self.epoch += 1
        self._seen(idf, self.epoch)

    def augment(self, n):
        """a successful direct augment"""
        self._append(n, self.epoch)

    def sim(self, idf, n_new):
        """a successful sim with observe != 0 that matched idf and created n_new features"""
        self.epoch += 1
        if self.batch_update:
            self._seen(idf, self.epoch)
        self._append(n_new, self.epoch)

    def remove(self, features):
        gone = set(int(f) for f in features)
        for name in ("hits", "born", "last"):
            setattr(self, name, [v for f, v in enumerate(getattr(self, name)) if f not in gone])

    def equals(self, stats):
        return (stats["epoch"] == self.epoch and list(stats["hits"]) == self.hits and list(stats["born"]) == self.born and
                list(stats["last"]) == self.last)
