"""EKF-SLAM as EkfSlam::sim computes it (slam_amd/csrc/host/ekfslam.cpp; the reference's algorithms/ekfslam.cpp:17-323 and
core.cpp:275-317), restated with numpy: the formulas, not the order of the sums.  dtype float64 is the yardstick the float32
filters (host and device) are measured against; dtype float32 is the yardstick where no host batch exists (more than 64
observations).  chunk=None applies a batch update as ONE batch, as the reference does; chunk=64 is the device's rule: chunks of at
most 64 observations one after another, each linearised at the state the previous chunk left."""
import numpy as np

ASSOC_NEW, ASSOC_DISCARD = -1, -2


def pi_to_pi(a):
    a = float(a)
    if a < -2 * np.pi or a > 2 * np.pi:
        a = a - np.floor(a / (2 * np.pi)) * (2 * np.pi)
    if a > np.pi:
        a -= 2 * np.pi
    if a < -np.pi:
        a += 2 * np.pi
    return a


class EkfModel:
    def __init__(self, dtype=np.float64, chunk=None, use_heading=False, batch_update=True, association_known=False, wheel_base=4.0,
                 sigma_phi=0.0, gate_reject=4.0, gate_augment=25.0):
        self.t = np.dtype(dtype).type
        self.chunk = chunk
        self.use_heading, self.batch_update, self.association_known = bool(use_heading), bool(batch_update), bool(association_known)
        self.wheel_base, self.sigma_phi = self.t(wheel_base), self.t(sigma_phi)
        self.gate_reject, self.gate_augment = float(gate_reject), float(gate_augment)
        self.x = np.zeros(3, self.t)
        self.P = np.zeros((3, 3), self.t)
        self.table = {}

    @property
    def dim(self):
        return self.x.shape[0]

    @property
    def nf(self):
        return (self.x.shape[0] - 3) // 2

    def upload(self, x, P):
        self.x = np.array(x, self.t)
        self.P = np.array(P, self.t)
        self.table = {f: f for f in range(self.nf)}

    def _m(self, a):
        return np.asarray(a, self.t).reshape(2, 2)

    # ---- the stages ---------------------------------------------------------------------------------------------------------
    def predict(self, V, G, Q, dt):
        t = self.t
        V, G, dt, Q = t(V), t(G), t(dt), self._m(Q)
        x, P = self.x, self.P
        s, c = np.sin(G + x[2]), np.cos(G + x[2])
        vts, vtc = V * dt * s, V * dt * c
        Gv = np.array([[1, 0, -vts], [0, 1, vtc], [0, 0, 1]], t)
        Gu = np.array([[dt * c, -vts], [dt * s, vtc], [dt * np.sin(G) / self.wheel_base, V * dt * np.cos(G) / self.wheel_base]], t)
        P[:3, :3] = Gv @ P[:3, :3] @ Gv.T + Gu @ Q @ Gu.T
        if self.dim > 3:
            P[:3, 3:] = Gv @ P[:3, 3:]
            P[3:, :3] = P[:3, 3:].T
        x[0] += vtc
        x[1] += vts
        x[2] = t(pi_to_pi(x[2] + V * dt * np.sin(G) / self.wheel_base))

    def observe_heading(self, phi):
        t = self.t
        x, P, n = self.x, self.P, self.dim
        v = t(pi_to_pi(t(phi) - x[2]))
        R = self.sigma_phi * self.sigma_phi
        PHt = P[:, 2].copy()
        S = PHt[2] + R
        W = PHt / S
        x += W * v
        C = np.eye(n, dtype=t)
        C[:, 2] -= W
        self.P = (C @ P @ C.T + np.outer(W, W) * R + np.eye(n, dtype=t) * t(2.2204e-16)).astype(t)

    def _model(self, idf):
        """zp [m, 2] and H [m, 2, 5] over the columns {0, 1, 2, f, f + 1} for features idf"""
        x = self.x
        idf = np.asarray(idf, np.int64)
        f = 3 + 2 * idf
        dx, dy = x[f] - x[0], x[f + 1] - x[1]
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2)
        xd, yd, xd2, yd2 = dx / d, dy / d, dx / d2, dy / d2
        zp = np.stack([d, np.arctan2(dy, dx) - x[2]], axis=1)
        o, z = np.ones_like(d), np.zeros_like(d)
        H = np.stack([np.stack([-xd, -yd, z, xd, yd], axis=1), np.stack([yd2, -xd2, -o, -yd2, xd2], axis=1)], axis=1)
        cols = np.stack([0 * f, 0 * f + 1, 0 * f + 2, f, f + 1], axis=1)
        return zp, H, cols

    def associate(self, z, Re, want_margin=False):
        """EKFSLAM::dataAssociate (ekfslam.cpp:151-189): labels[nz]; with want_margin also margin[nz], how close each decision was: the
        smallest of |nis_j - gate_reject| and |nis_j - gate_augment| over all features and, where two or more features pass the reject
        gate, the gap between the two smallest nd_j among them (inf without features: nothing is compared)"""
        z = np.asarray(z, self.t).reshape(-1, 2)
        Re = self._m(Re)
        lab = np.full(z.shape[0], ASSOC_DISCARD, np.int32)
        margin = np.full(z.shape[0], np.inf)
        nf = self.nf
        if nf == 0:
            lab[:] = ASSOC_NEW
            return (lab, margin) if want_margin else lab
        zp, H, cols = self._model(np.arange(nf))
        M = self.P[cols[:, :, None], cols[:, None, :]]
        S = H @ M @ H.transpose(0, 2, 1) + Re
        Si = np.linalg.inv(S)
        logdet = np.log(np.linalg.det(S))
        for i in range(z.shape[0]):
            v = z[i] - zp
            v[:, 1] = [pi_to_pi(a) for a in v[:, 1]]
            nis = np.einsum("ja,jab,jb->j", v, Si, v)
            nd = nis + logdet
            jbest, nbest, outer = -1, np.inf, np.inf
            for j in range(nf):
                if nis[j] < self.gate_reject and nd[j] < nbest:
                    nbest, jbest = nd[j], j
                elif nis[j] < outer:
                    outer = nis[j]
            lab[i] = jbest if jbest >= 0 else (ASSOC_NEW if outer > self.gate_augment else ASSOC_DISCARD)
            if want_margin:
                n64 = nis.astype(np.float64)
                margin[i] = min(np.abs(n64 - self.gate_reject).min(), np.abs(n64 - self.gate_augment).min())
                gated = np.sort(nd.astype(np.float64)[n64 < self.gate_reject])
                if gated.shape[0] > 1:
                    margin[i] = min(margin[i], gated[1] - gated[0])
        return (lab, margin) if want_margin else lab

    def _batch(self, zf, idf, R):
        t = self.t
        m, D = len(idf), self.dim
        zp, H5, cols = self._model(idf)
        H = np.zeros((2 * m, D), t)
        for i in range(m):
            H[2 * i:2 * i + 2, cols[i]] = H5[i]
        v = (zf - zp).reshape(-1)
        v[1::2] = [pi_to_pi(a) for a in v[1::2]]
        v = v.astype(t)
        RR = np.kron(np.eye(m, dtype=t), R)
        # choleskyUpdate (core.cpp:275-291)
        PHt = self.P @ H.T
        S = H @ PHt + RR
        S = (S + S.T) * t(0.5)
        L = np.linalg.cholesky(S)
        Ui = np.linalg.inv(L.T)
        W1 = PHt @ Ui
        self.x = (self.x + W1 @ (Ui.T @ v)).astype(t)
        self.P = (self.P - W1 @ W1.T).astype(t)

    def update(self, zf, idf, R):
        zf = np.asarray(zf, self.t).reshape(-1, 2)
        idf = np.asarray(idf, np.int64)
        R = self._m(R)
        m = idf.shape[0]
        step = m if self.chunk is None else self.chunk
        for at in range(0, m, max(step, 1)):
            self._batch(zf[at:at + step], idf[at:at + step], R)

    def augment(self, zn, Re):
        t = self.t
        Re = self._m(Re)
        for r, b in np.asarray(zn, t).reshape(-1, 2):
            x, P, n = self.x, self.P, self.dim
            s, c = np.sin(x[2] + b), np.cos(x[2] + b)
            Gv = np.array([[1, 0, -r * s], [0, 1, r * c]], t)
            Gz = np.array([[c, -r * s], [s, r * c]], t)
            Pn = np.zeros((n + 2, n + 2), t)
            Pn[:n, :n] = P
            Pn[n:, n:] = Gv @ P[:3, :3] @ Gv.T + Gz @ Re @ Gz.T
            Pn[n:, :n] = Gv @ P[:3, :]
            Pn[:n, n:] = Pn[n:, :n].T
            self.x = np.concatenate([x, np.array([x[0] + r * c, x[1] + r * s], t)])
            self.P = Pn

    # ---- EKFSLAM::sim (ekfslam.cpp:17-43) ------------------------------------------------------------------------------------
    def sim(self, V, G, Q, dt, phi, z=None, ids=None, Re=None, R=None, observe=0):
        """returns the labels the step used (feature, ASSOC_NEW or ASSOC_DISCARD per observation), or None without an observation"""
        self.predict(V, G, Q, dt)
        if self.use_heading:
            self.observe_heading(phi)
        if not observe:
            return None
        z = np.zeros((0, 2), self.t) if z is None else np.asarray(z, self.t).reshape(-1, 2)
        if self.association_known:
            lab = np.array([self.table.get(int(i), ASSOC_NEW) for i in ids], np.int32).reshape(-1)
        else:
            lab = self.associate(z, Re)
        nf0 = self.nf
        if self.batch_update and (lab >= 0).any():
            self.update(z[lab >= 0], lab[lab >= 0], R)
        self.augment(z[lab == ASSOC_NEW], Re)
        if self.association_known:
            for k, i in enumerate(np.asarray(ids).reshape(-1)[lab == ASSOC_NEW]):
                self.table[int(i)] = nf0 + k
        return lab
