"""Model of the device EKF's local periods (include/slamgpu.h: slamgpu_ekf_local_*): the compressed EKF of Guivant and Nebot on top of
ekf_model.EkfModel.  Between local_begin and local_end the stages of EkfModel run on the extended symmetric matrix and state

    M = [ P_AA   phi ]      s = [ x_A   ]      at begin: phi = I (na0 x na0), psi = 0, theta = 0
        [ phi^T -psi ]          [ theta ]

(A: the pose, the chosen features and the features the period creates; the na0 = 3 + 2 k carried entries are state that no observation
refers to, that the gates skip and behind which augment does not append), and local_end commits with Y = P[A0, B] as it stood at begin:

    P[A, B] = phi Y (and its mirror)      P[B, B] -= Y^T psi Y      x_B += Y^T theta      P[A, A], x_A scattered back.

Feature indices in idf and in labels are global throughout.  The model keeps the carried entries directly behind the active state (the
device leaves room for max_new features between them: a layout, not arithmetic).  Also here: the scripts of stage calls that the CPU
and the GPU tests drive every filter with, and their synthetic states."""
import numpy as np

from ekf_model import ASSOC_NEW, EkfModel

# (every input of a script is a float32 value: the float64 models and the device are handed the same numbers)
Q = np.array([[0.3 ** 2, 0], [0, (3.0 * np.pi / 180) ** 2]], np.float32)
R = np.array([[0.1 ** 2, 0], [0, (1.0 * np.pi / 180) ** 2]], np.float32)
DT = float(np.float32(0.025))
CONF = dict(wheel_base=4.0, sigma_phi=0.0087, gate_reject=4.0, gate_augment=25.0)
CHUNK = 64  # the device's chunk of a batch update (ekf_helpers.h: kChunk)


class Invalid(Exception):
    pass


class Capacity(Exception):
    pass


class _Ext(EkfModel):
    """EkfModel on the extended state: only the first nreal features are features"""
    nreal = 0

    @property
    def nf(self):
        return self.nreal


class EkfLocalModel:
    def __init__(self, **kw):
        """kw: EkfModel's, chunk and dtype among them: the full filter and every period's extended one are built from the same"""
        self.kw = kw
        self.full = EkfModel(**kw)
        self.ext = None
        self.commits = 0

    # ---- what EkfModel offers, on whichever filter is current ------------------------------------------------------------------
    @property
    def x(self):
        assert self.ext is None
        return self.full.x

    @property
    def P(self):
        assert self.ext is None
        return self.full.P

    @property
    def dim(self):
        return self.full.dim + (2 * self.n_new if self.ext is not None else 0)

    @property
    def nf(self):
        return (self.dim - 3) // 2

    def upload(self, x, P):
        if self.ext is not None:
            raise Invalid("upload while a period is open")
        self.full.upload(x, P)

    def pose(self):
        m = self.ext if self.ext is not None else self.full
        return m.x[:3].copy(), m.P[:3, :3].copy()

    # ---- the period -------------------------------------------------------------------------------------------------------------------
    def local_begin(self, features, max_new=0):
        if self.ext is not None:
            raise Invalid("a period is open")
        f = np.asarray(features, np.int64).reshape(-1)
        nf0, dim0 = self.full.nf, self.full.dim
        if max_new < 0 or (f.size and (f.min() < 0 or f.max() >= nf0 or (np.diff(f) <= 0).any())):
            raise Invalid("features: ascending, distinct, in [0, nf)")
        t = self.full.t
        A0 = np.concatenate([np.arange(3), np.stack([3 + 2 * f, 4 + 2 * f], axis=1).reshape(-1)]).astype(np.int64)
        B = np.setdiff1d(np.arange(dim0), A0)
        na0 = A0.shape[0]
        ext = _Ext(**self.kw)
        ext.x = np.concatenate([self.full.x[A0], np.zeros(na0, t)]).astype(t)
        M = np.zeros((2 * na0, 2 * na0), t)
        M[:na0, :na0] = self.full.P[np.ix_(A0, A0)]
        M[:na0, na0:] = np.eye(na0, dtype=t)
        M[na0:, :na0] = np.eye(na0, dtype=t)
        ext.P = M
        ext.nreal = f.shape[0]
        self.ext, self.A0, self.B, self.Y = ext, A0, B, self.full.P[np.ix_(A0, B)].copy()
        self.feat, self.nf0, self.max_new, self.n_new = f, nf0, int(max_new), 0
        self.g2l = {int(g): i for i, g in enumerate(f)}

    def local_end(self):
        if self.ext is None:
            raise Invalid("no period is open")
        t = self.full.t
        na0, dimA, dim0 = self.A0.shape[0], 3 + 2 * (self.feat.shape[0] + self.n_new), self.full.dim
        M, s = self.ext.P, self.ext.x
        phi, psi, theta = M[:dimA, dimA:], -M[dimA:, dimA:], s[dimA:]
        A = np.concatenate([self.A0, dim0 + np.arange(2 * self.n_new)]).astype(np.int64)
        B, Y = self.B, self.Y
        D = dim0 + 2 * self.n_new
        P, x = np.zeros((D, D), t), np.zeros(D, t)
        P[:dim0, :dim0], x[:dim0] = self.full.P, self.full.x
        PAB = (phi @ Y).astype(t)
        P[np.ix_(A, B)] = PAB
        P[np.ix_(B, A)] = PAB.T
        P[np.ix_(B, B)] = (P[np.ix_(B, B)] - Y.T @ (psi @ Y)).astype(t)
        x[B] = (x[B] + Y.T @ theta).astype(t)
        P[np.ix_(A, A)] = M[:dimA, :dimA]
        x[A] = s[:dimA]
        self.full.x, self.full.P = x, P
        self.ext = None
        self.commits += 1

    def _local(self, idf):
        out = []
        for f in np.asarray(idf, np.int64).reshape(-1):
            f = int(f)
            l = self.g2l.get(f, -1) if f < self.nf0 else (self.feat.shape[0] + f - self.nf0 if 0 <= f - self.nf0 < self.n_new else -1)
            if l < 0:
                raise Invalid("feature %d is not active" % f)
            out.append(l)
        return np.array(out, np.int64)

    def _global(self, lab):
        k = self.feat.shape[0]
        return np.array([l if l < 0 else (self.feat[l] if l < k else self.nf0 + l - k) for l in lab], np.int32)

    # ---- the stages ---------------------------------------------------------------------------------------------------------------------
    def predict(self, V, G, Q, dt):
        (self.ext or self.full).predict(V, G, Q, dt)

    def observe_heading(self, phi):
        (self.ext or self.full).observe_heading(phi)

    def associate(self, z, Re, want_margin=False):
        if self.ext is None:
            return self.full.associate(z, Re, want_margin)
        out = self.ext.associate(z, Re, want_margin)
        return (self._global(out[0]), out[1]) if want_margin else self._global(out)

    def update(self, zf, idf, R):
        if self.ext is None:
            return self.full.update(zf, idf, R)
        self.ext.update(zf, self._local(idf), R)

    def augment(self, zn, Re):
        if self.ext is None:
            return self.full.augment(zn, Re)
        zn = np.asarray(zn, self.full.t).reshape(-1, 2)
        if self.n_new + zn.shape[0] > self.max_new:
            raise Capacity("max_new")
        for one in zn:
            e = self.ext
            dimA, n = 3 + 2 * e.nreal, e.dim
            e.augment(one[None], Re)  # appended behind the carried entries: Gv phi[pose rows] over them, as over every column
            order = np.concatenate([np.arange(dimA), [n, n + 1], np.arange(dimA, n)])
            e.x, e.P = e.x[order], e.P[np.ix_(order, order)]
            e.nreal += 1
            self.n_new += 1

    def sim(self, V, G, Q, dt, phi, z=None, ids=None, Re=None, R=None, observe=0):
        if self.ext is None:
            return self.full.sim(V, G, Q, dt, phi, z, ids, Re, R, observe)
        m = self.full
        z = np.zeros((0, 2), m.t) if z is None else np.asarray(z, m.t).reshape(-1, 2)
        known = m.association_known
        if observe and known:  # before anything runs
            lab = np.array([m.table.get(int(i), ASSOC_NEW) for i in ids], np.int32).reshape(-1)
            self._local(lab[lab >= 0])
            if self.n_new + int((lab == ASSOC_NEW).sum()) > self.max_new:
                raise Capacity("max_new")
        self.predict(V, G, Q, dt)
        if m.use_heading:
            self.observe_heading(phi)
        if not observe:
            return None
        if not known:
            lab = self.associate(z, Re)
        nf0 = self.nf
        if m.batch_update and (lab >= 0).any():
            self.update(z[lab >= 0], lab[lab >= 0], R)
        self.augment(z[lab == ASSOC_NEW], Re)
        if known:
            for k, i in enumerate(np.asarray(ids).reshape(-1)[lab == ASSOC_NEW]):
                m.table[int(i)] = nf0 + k
        return lab


# ---- synthetic states and scripts ---------------------------------------------------------------------------------------------------------
def synthetic_state(nf, seed, spread=1.0):
    """a pose near the origin, nf landmarks on a ring (radius 20 .. 25 times spread), and a covariance shaped like a SLAM posterior:
    every landmark inherits the pose's uncertainty through a Jacobian of its own and adds a small block of its own.  float32 values,
    the lower triangle mirrored"""
    rng = np.random.default_rng(seed)
    D = 3 + 2 * nf
    ang = np.linspace(0, 2 * np.pi, nf, endpoint=False) + 0.05
    rad = (20.0 + 5.0 * rng.random(nf)) * spread
    x = np.zeros(D)
    x[:3] = (0.3, -0.2, 0.1)
    x[3::2], x[4::2] = x[0] + rad * np.cos(ang), x[1] + rad * np.sin(ang)
    J = np.zeros((D, 3))
    J[:3] = np.eye(3)
    J[3:] = rng.normal(0, 1.0, (2 * nf, 3))
    P = J @ np.diag([0.05, 0.05, 0.002]) @ J.T
    for j in range(nf):
        a = rng.normal(0, 0.15, (2, 2))
        P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] += a @ a.T + 0.01 * np.eye(2)
    P = P.astype(np.float32)
    P = np.tril(P) + np.tril(P, -1).T
    return x.astype(np.float32), P


def observations(x, idf, rng, noise=1.0):
    f = 3 + 2 * np.asarray(idf, np.int64)
    dx, dy = x[f] - x[0], x[f + 1] - x[1]
    z = np.stack([np.sqrt(dx * dx + dy * dy) + rng.normal(0, 0.1 * noise, len(f)),
                  np.arctan2(dy, dx) - x[2] + rng.normal(0, 0.01 * noise, len(f))], axis=1)
    return z.astype(np.float32)


def build_script(x0, P0, periods, use_heading, seed):
    """The stage calls of a run, made while a float64 full EkfModel runs them (it is where the observations come from); returns
    (script, that model).  The model applies an update in the device's chunks (ekf_model.py: chunk=64, each chunk linearised where the
    previous one left the state; up to 64 observations that is the one batch).  periods: dicts of features (global, ascending), max_new, steps, m (observations of active features per
    step; those the period created are always among them), new (features created at step s: new[s], 0 beyond the list).  A script
    entry is (name, args); begin / end are skipped by a filter without periods"""
    rng = np.random.default_rng(seed)
    ref = EkfModel(chunk=CHUNK, use_heading=use_heading, association_known=True, **CONF)
    ref.upload(x0, P0)
    script = []
    for p in periods:
        feats = np.asarray(p["features"], np.int64)
        script.append(("begin", (feats.astype(np.int32), int(p.get("max_new", 0)))))
        created = []
        for s in range(p["steps"]):
            V, G = 3.0, float(np.float32(0.05 * (-1) ** s))
            script.append(("predict", (V, G, Q, DT)))
            ref.predict(V, G, Q, DT)
            if use_heading:
                phi = float(np.float32(ref.x[2] + rng.normal(0, 0.004)))
                script.append(("heading", (phi,)))
                ref.observe_heading(phi)
            m = min(int(p.get("m", 0)), feats.shape[0])
            idf = np.concatenate([rng.permutation(feats)[:m], created]).astype(np.int32)
            if idf.shape[0]:
                zf = observations(ref.x, idf, rng)
                script.append(("update", (zf, idf, R)))
                ref.update(zf, idf, R)
            n = p.get("new", [])[s] if s < len(p.get("new", [])) else 0
            if n:
                zn = np.stack([15.0 + 2.0 * rng.random(n), rng.uniform(-3, 3, n)], axis=1).astype(np.float32)
                script.append(("augment", (zn, R)))
                created += list(range(ref.nf, ref.nf + n))
                ref.augment(zn, R)
        script.append(("end", ()))
    return script, ref


BLOCKS = ("P[A,A]", "P[A,B]", "P[B,B]", "x_A", "x_B")


def blocks_of(script, dim0, dim):
    """(A, B) of a script of ONE period that opens on a state of dimension dim0 and leaves one of dimension dim: the state entries of
    the pose, the begin entry's features and the features created since, and the rest"""
    begins = [a for n, a in script if n == "begin"]
    assert len(begins) == 1
    f = np.asarray(begins[0][0], np.int64)
    A = np.concatenate([np.arange(3), np.stack([3 + 2 * f, 4 + 2 * f], axis=1).reshape(-1), np.arange(dim0, dim)]).astype(np.int64)
    return A, np.setdiff1d(np.arange(dim0), A)


def block_errors(x, P, xm, Pm, A, B):
    """{block: max |difference| over the block relative to the model's largest magnitude IN that block}, empty blocks left out"""
    parts = {"P[A,A]": (P[np.ix_(A, A)], Pm[np.ix_(A, A)]), "P[A,B]": (P[np.ix_(A, B)], Pm[np.ix_(A, B)]),
             "P[B,B]": (P[np.ix_(B, B)], Pm[np.ix_(B, B)]), "x_A": (x[A], xm[A]), "x_B": (x[B], xm[B])}
    return {name: float(np.abs(got - want).max() / np.abs(want).max()) for name, (got, want) in parts.items() if want.size}


def drive(f, script, periods=True):
    """run a script on a filter with EkfModel's method names (EkfModel, EkfLocalModel, slam_amd.EkfGpu)"""
    for name, a in script:
        if name == "begin":
            if periods:
                f.local_begin(*a)
        elif name == "end":
            if periods:
                f.local_end()
        elif name == "heading":
            f.observe_heading(*a)
        else:
            getattr(f, name)(*a)
