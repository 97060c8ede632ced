"""Model of the device EKF ensemble (include/slamgpu.h: slamgpu_ens_*): B independent ekf_model.EkfModel instances stepped on
per-member inputs, the noise rule of sim_noise restated with the oracle's Philox integers and a float64 Box-Muller, and the
consistency accumulators from pose_model.nees' definitions.  Written from the header's text; the yardstick of
tests/test_ekf_ens_cpu.py and tests/test_gpu_ekf_ens.py."""
import math

import numpy as np

import ekf_model
import pose_model

STATUS_NOT_PD, STATUS_CAPACITY = 1, 2
NOISE_CONTROL, NOISE_HEADING, NOISE_SENSOR = 1, 2, 4
STREAM = 5
f32, f64 = np.float32, np.float64


class Ensemble:
    """B EkfModel instances; ids and nz are shared, VG / phi / z are per member"""

    def __init__(self, members, max_landmarks, dtype=np.float64, chunk=None, **cfg):
        self.B, self.max_landmarks = members, max_landmarks
        self.m = [ekf_model.EkfModel(dtype=dtype, chunk=chunk, **cfg) for _ in range(members)]
        self.status = np.zeros(members, np.int32)
        self.acc = np.zeros((members, 6))
        self.labels = [None] * members

    def upload(self, b, x, P):
        self.m[b].upload(x, P)

    def dims(self):
        return np.array([m.dim for m in self.m], np.int32)

    def sim(self, VG, phi, Q, dt, z=None, ids=None, Re=None, R=None, observe=0, truth=None):
        VG, phi = np.asarray(VG).reshape(self.B, 2), np.asarray(phi).reshape(self.B)
        z = None if z is None else np.asarray(z).reshape(self.B, -1, 2)
        for b, m in enumerate(self.m):
            self.labels[b] = self._member(b, m, VG[b], phi[b], Q, dt, None if z is None else z[b], ids, Re, R, observe)
        if truth is not None:
            self.accumulate(np.array([m.x[:3] for m in self.m], f64), np.array([m.P[:3, :3] for m in self.m], f64), truth)

    def _member(self, b, m, vg, phi, Q, dt, z, ids, Re, R, observe):
        """EkfModel.sim with the per-member capacity rule: a step that needs more than max_landmarks features applies its predict and
        heading only and sets STATUS_CAPACITY.  (Known association: every member keeps a table of its own here; the device's ONE shared
        table refuses a step for all members alike, which is the same thing as long as the members have the same dimension)"""
        m.predict(vg[0], vg[1], Q, dt)
        if m.use_heading:
            m.observe_heading(phi)
        if not observe:
            return None
        z = np.zeros((0, 2), m.t) if z is None else np.asarray(z, m.t).reshape(-1, 2)
        if m.association_known:
            lab = np.array([m.table.get(int(i), ekf_model.ASSOC_NEW) for i in ids], np.int32).reshape(-1)
        else:
            lab = m.associate(z, Re)
        if m.nf + int((lab == ekf_model.ASSOC_NEW).sum()) > self.max_landmarks:
            self.status[b] |= STATUS_CAPACITY
            return lab
        nf0 = m.nf
        if m.batch_update and (lab >= 0).any():
            m.update(z[lab >= 0], lab[lab >= 0], R)
        m.augment(z[lab == ekf_model.ASSOC_NEW], Re)
        if m.association_known:
            for k, i in enumerate(np.asarray(ids).reshape(-1)[lab == ekf_model.ASSOC_NEW]):
                m.table[int(i)] = nf0 + k
        return lab

    def accumulate(self, xyt, Pvv, truth):
        accumulate(self.acc, xyt, Pvv, truth)


def accumulate(acc, xyt, Pvv, truth):
    """one step of the six accumulators for every member: xyt[B, 3], Pvv[B, 3, 3] as the filters hold them (float32 values), in double"""
    t = [float(v) for v in np.asarray(truth, f32)]
    for b in range(len(acc)):
        x = [float(v) for v in np.asarray(xyt[b], f64)]
        P = np.asarray(Pvv[b], f64)
        e = (x[0] - t[0], x[1] - t[1], math.remainder(x[2] - t[2], pose_model.TWO_PI) if math.isfinite(x[2]) else math.nan)
        val = nees3(e, [float(P[i, j]) for i, j in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))])
        if val is None:
            acc[b, 1] += 1
            continue
        acc[b, 0] += 1
        acc[b, 2] += val
        acc[b, 3] += val <= pose_model.CHI2_3_95
        acc[b, 4] += e[0] * e[0] + e[1] * e[1]
        acc[b, 5] += e[2] * e[2]


def nees3(e, p):
    """e^T P^-1 e through the Cholesky factor of the 3 x 3 P (p: its lower triangle 00, 10, 11, 20, 21, 22), each operation rounded on
    its own, in the order the header's definition reads: L row by row, then the forward substitution.  None where P is not positive
    definite or anything is not finite (slamhost_pose_nees's NaN)"""
    p00, p10, p11, p20, p21, p22 = p
    if not all(math.isfinite(v) for v in (*e, *p)) or not p00 > 0.0:
        return None
    l00 = math.sqrt(p00)
    l10, l20 = p10 / l00, p20 / l00
    d1 = p11 - l10 * l10
    if not d1 > 0.0:
        return None
    l11 = math.sqrt(d1)
    l21 = (p21 - l20 * l10) / l11
    d2 = (p22 - l20 * l20) - l21 * l21
    if not d2 > 0.0:
        return None
    l22 = math.sqrt(d2)
    y0 = e[0] / l00
    y1 = (e[1] - l10 * y0) / l11
    y2 = ((e[2] - l20 * y0) - l21 * y1) / l22
    val = (y0 * y0 + y1 * y1) + y2 * y2
    return val if math.isfinite(val) else None


# ---- the noise rule ---------------------------------------------------------------------------------------------------------------
def u01(word):
    """device_math.h: ((x >> 8) + 0.5) / 2^24, exact in float32 and in double"""
    return ((int(word) >> 8) + 0.5) / 16777216.0


def normals(words):
    """box_muller3's g0 (sin) and g1 (cos) of a Philox block, in float64"""
    amp = math.sqrt(-2.0 * math.log(u01(words[0])))
    ang = 2.0 * math.pi * u01(words[1])
    return amp * math.sin(ang), amp * math.cos(ang)


def chol2(Q):
    """the lower Cholesky factor of Q, computed in float as the host side does"""
    Q = np.asarray(Q, f32).reshape(2, 2)
    l00 = f32(np.sqrt(Q[0, 0]))
    l10 = f32(Q[1, 0] / l00)
    l11 = f32(np.sqrt(f32(Q[1, 1] - f32(l10 * l10))))
    return float(l00), float(l10), float(l11)


def draw(philox, seed, members, step, V, G, phi_true, z_true, Q, R, sigma_phi, noise):
    """(VG[B, 2], phi[B], z[B, nz, 2], g) in float64: the inputs member b draws at `step`; g[B, 2 + 2 nz] are the unit normals behind VG
    and z (NaN where the noise is off), the tests' handle on the tolerance.  philox(c, k) -> 4 words (orc.Oracle.philox)"""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    z_true = np.zeros((0, 2)) if z_true is None else np.asarray(z_true, f32).astype(f64).reshape(-1, 2)
    nz = z_true.shape[0]
    V, G, phi_true, sigma_phi = (float(f32(a)) for a in (V, G, phi_true, sigma_phi))
    l00, l10, l11 = chol2(Q) if noise & NOISE_CONTROL else (0.0, 0.0, 0.0)
    R = np.asarray(R, f32).reshape(2, 2)
    sr = float(f32(np.sqrt(R[0, 0]))), float(f32(np.sqrt(R[1, 1])))
    VG, phi, z, g = np.zeros((members, 2)), np.zeros(members), np.zeros((members, nz, 2)), np.full((members, 2 + 2 * nz), np.nan)
    for b in range(members):
        VG[b], phi[b], z[b] = (V, G), phi_true, z_true
        if noise & NOISE_CONTROL:
            g0, g1 = normals(philox((b, step, STREAM, 0), key))
            VG[b] = (V + l00 * g0, G + l10 * g0 + l11 * g1)
            g[b, :2] = g0, g1
        if noise & NOISE_HEADING:
            phi[b] = phi_true + sigma_phi * u01(philox((b, step, STREAM, 1), key)[0])
        if noise & NOISE_SENSOR:
            for i in range(nz):
                g0, g1 = normals(philox((b, step, STREAM, 2 + i), key))
                z[b, i] = (z_true[i, 0] + g0 * sr[0], z_true[i, 1] + g1 * sr[1])
                g[b, 2 + 2 * i:4 + 2 * i] = g0, g1
    return VG, phi, z, g
