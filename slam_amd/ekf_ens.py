"""ctypes binding of the device EKF-SLAM ensemble (include/slamgpu.h: slamgpu_ens_*), in the manner of ekf.py: no fallback, a
missing library or GPU is an error."""
import ctypes as C

import numpy as np

from .capi import SlamGpuError, load_library, _f32, _ptr

EKF_STATUS_CAPACITY = 2  # SLAMGPU_EKF_STATUS_CAPACITY
NOISE_CONTROL, NOISE_HEADING, NOISE_SENSOR = 1, 2, 4  # SLAMGPU_EKF_ENS_NOISE_*
CONSISTENCY_FIELDS = ("counted", "not_counted", "sum_nees", "inside_95", "sum_pos_err2", "sum_heading_err2")
MAX_RUN = 4096  # steps of one run_noise
TRACE_TAG_NONE = 0xFFFFFFFF  # the tag of a traced step of sim, which has no Philox step word
# slamgpu_ens_tape_step
TAPE_STEP_DTYPE = np.dtype([("V", np.float32), ("G", np.float32), ("phi_true", np.float32), ("dt", np.float32), ("truth", np.float32, (3,)),
                            ("has_truth", np.int32), ("observe", np.int32), ("nz", np.int32), ("first", np.int32), ("step", np.uint32)])


def pack_tape(list_of_steps):
    """A list of per-step dicts -> (steps, z_true, ids) as run_noise takes them.  A step has V, G, phi_true, dt, step and may have
    truth (3 floats; absent or None: the step is not counted), observe, z_true [nz, 2] and ids [nz].  The observations of the steps lie one
    behind the other; a step that does not observe has nz 0 whatever it carries, and `first` is where its observations would start."""
    steps = np.zeros(len(list_of_steps), TAPE_STEP_DTYPE)
    zs, idl, at = [], [], 0
    for k, d in enumerate(list_of_steps):
        r = steps[k]
        r["V"], r["G"], r["phi_true"], r["dt"], r["step"] = d["V"], d["G"], d["phi_true"], d["dt"], d["step"]
        truth = d.get("truth")
        if truth is not None:
            r["truth"], r["has_truth"] = np.asarray(truth, np.float32), 1
        r["observe"] = int(bool(d.get("observe", 0)))
        z = d.get("z_true")
        z = np.zeros((0, 2), np.float32) if z is None or not r["observe"] else np.asarray(z, np.float32).reshape(-1, 2)
        r["nz"], r["first"] = z.shape[0], at
        if z.shape[0]:
            i = d.get("ids")
            i = np.zeros(z.shape[0], np.int32) if i is None else np.asarray(i, np.int32).reshape(-1)
            if i.shape[0] != z.shape[0]:
                raise ValueError("step %d: %d ids for %d observations" % (k, i.shape[0], z.shape[0]))
            zs.append(z)
            idl.append(i)
            at += z.shape[0]
    z_true = np.concatenate(zs) if zs else np.zeros((0, 2), np.float32)
    ids = np.concatenate(idl) if idl else np.zeros(0, np.int32)
    return steps, np.ascontiguousarray(z_true, np.float32), np.ascontiguousarray(ids, np.int32)


def trace_summary(records):
    """The trace's records [n, 6] (trace_fetch) as the figures of a consistency plot, [n, 5] in double, one row per step: the mean NEES
    over the counted members, the share of them inside the 95 % bound, the rms position error, the members counted and not counted
    (what slam-backend -RUNS_TRACE writes per line).  NaN where no member was counted."""
    r = np.asarray(records, np.float64).reshape(-1, 6)
    out = np.full((r.shape[0], 5), np.nan)
    ok = r[:, 0] > 0
    out[ok, 0] = r[ok, 2] / r[ok, 0]
    out[ok, 1] = r[ok, 3] / r[ok, 0]
    out[ok, 2] = np.sqrt(r[ok, 4] / r[ok, 0])
    out[:, 3], out[:, 4] = r[:, 0], r[:, 1]
    return out


def _max_corr(M):
    """the largest |correlation| between two different components of a covariance (NaN: fewer than two, or a variance that is not
    positive)"""
    d = np.diag(M)
    if M.shape[0] < 2 or not (d > 0).all():
        return float("nan")
    r = np.abs(M / np.sqrt(np.outer(d, d)))
    np.fill_diagonal(r, 0.0)
    return float(r.max())


def moments_summary(mean, C, Pbar, truth_pose=None, truth_landmarks=None):
    """What EkfEnsemble.moments says about the filter's consistency, as a dict.  C is the spread the members have, Pbar the spread
    their filters claim: a consistent filter has ratios near 1 (below 1: pessimistic, above: optimistic) and a bias whose square is
    far below Pbar.
      pos_ratio      tr C[0:2, 0:2] / tr Pbar[0:2, 0:2]        heading_ratio  C[2, 2] / Pbar[2, 2]
      feature_ratio_mean / _min / _max   tr C_ff / tr Pbar_ff over the features (NaN without features)
      max_corr_C, max_corr_Pbar          the largest |correlation| between two different components
    and with truth_pose (x, y, theta): bias_pos (m), bias_heading (rad, the short way round); with truth_landmarks [nf, 2] in the
    features' order: bias_landmarks, the mean distance of the mean's features from them"""
    mean, C, Pbar = np.asarray(mean, np.float64), np.asarray(C, np.float64), np.asarray(Pbar, np.float64)
    D = mean.shape[0]
    nf = (D - 3) // 2
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"pos_ratio": float((C[0, 0] + C[1, 1]) / (Pbar[0, 0] + Pbar[1, 1])), "heading_ratio": float(C[2, 2] / Pbar[2, 2])}
        i = 3 + 2 * np.arange(nf)
        fr = (C[i, i] + C[i + 1, i + 1]) / (Pbar[i, i] + Pbar[i + 1, i + 1])
    out["feature_ratio_mean"] = float(fr.mean()) if nf else float("nan")
    out["feature_ratio_min"] = float(fr.min()) if nf else float("nan")
    out["feature_ratio_max"] = float(fr.max()) if nf else float("nan")
    out["max_corr_C"], out["max_corr_Pbar"] = _max_corr(C), _max_corr(Pbar)
    if truth_pose is not None:
        t = np.asarray(truth_pose, np.float64)
        out["bias_pos"] = float(np.hypot(mean[0] - t[0], mean[1] - t[1]))
        out["bias_heading"] = float(np.remainder(mean[2] - t[2] + np.pi, 2 * np.pi) - np.pi)
    if truth_landmarks is not None:
        t = np.asarray(truth_landmarks, np.float64).reshape(-1, 2)
        if t.shape[0] != nf:
            raise ValueError("%d true landmarks for %d features" % (t.shape[0], nf))
        out["bias_landmarks"] = float(np.hypot(*(mean[3:].reshape(-1, 2) - t).T).mean()) if nf else float("nan")
    return out


class EkfEnsConfig(C.Structure):  # slamgpu_ekf_ens_config
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("members", C.c_int32), ("max_landmarks", C.c_int32),
                ("use_heading", C.c_int32), ("batch_update", C.c_int32), ("association_known", C.c_int32), ("wheel_base", C.c_float),
                ("sigma_phi", C.c_float), ("gate_reject", C.c_float), ("gate_augment", C.c_float), ("seed", C.c_uint64),
                ("external_stream", C.c_uint64)]


_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, u32, f = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
        L.slamgpu_ens_create.argtypes = [C.POINTER(EkfEnsConfig), C.POINTER(vp)]
        L.slamgpu_ens_destroy.argtypes = [vp]
        L.slamgpu_ens_destroy.restype = None
        L.slamgpu_ens_sync.argtypes = [vp]
        L.slamgpu_ens_sim.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, f, i32, vp]
        L.slamgpu_ens_sim_noise.argtypes = [vp, f, f, f, vp, vp, i32, u32, vp, vp, vp, vp, f, i32, vp, u32]
        L.slamgpu_ens_last_inputs.argtypes = [vp, vp, vp, vp]
        L.slamgpu_ens_dims.argtypes = [vp, vp]
        L.slamgpu_ens_poses.argtypes = [vp, vp]
        L.slamgpu_ens_state.argtypes = [vp, i32, vp, vp, i32]
        L.slamgpu_ens_slab.argtypes = [vp, i32, vp, vp]
        L.slamgpu_ens_upload.argtypes = [vp, i32, i32, vp, vp, i32]
        L.slamgpu_ens_status.argtypes = [vp, vp]
        L.slamgpu_ens_consistency.argtypes = [vp, vp]
        L.slamgpu_ens_consistency_reset.argtypes = [vp]
        if hasattr(L, "slamgpu_ens_run_noise"):  # (an older build loaded through SLAMGPU_LIB for an A/B lacks the run and the trace)
            L.slamgpu_ens_run_noise.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, u32]
            L.slamgpu_ens_trace_enable.argtypes = [vp, i32]
            L.slamgpu_ens_trace_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(i32)]
            L.slamgpu_ens_trace_fetch.argtypes = [vp, C.c_int64, i32, vp, vp]
        if hasattr(L, "slamgpu_ens_moments"):  # (likewise)
            L.slamgpu_ens_moments.argtypes = [vp, i32, u32, vp, vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
        _bound = True
    return L


def _chk(rc):
    if rc < 0:
        raise SlamGpuError(rc, load_library().slamgpu_last_error().decode())
    return rc


class EkfEnsemble:
    """`members` independent EKF-SLAM filters resident on the GPU: one launch per EKFSLAM::sim of all of them."""

    def __init__(self, members, max_landmarks, use_heading=False, batch_update=True, association_known=False, wheel_base=4.0, sigma_phi=0.0,
                 gate_reject=4.0, gate_augment=25.0, seed=0, device=0, external_stream=0):
        self.L = _lib()
        cfg = EkfEnsConfig(C.sizeof(EkfEnsConfig), device, members, max_landmarks, int(use_heading), int(batch_update), int(association_known),
                           wheel_base, sigma_phi, gate_reject, gate_augment, seed, external_stream)
        h = C.c_void_p()
        _chk(self.L.slamgpu_ens_create(C.byref(cfg), C.byref(h)))
        self.h, self.cfg, self.members, self.max_landmarks = h, cfg, members, max_landmarks
        self.cap_dim = 3 + 2 * max_landmarks
        self.ld = (self.cap_dim + 31) // 32 * 32
        self._nz = 0

    def close(self):
        if self.h:
            self.L.slamgpu_ens_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        _chk(self.L.slamgpu_ens_sync(self.h))

    def sim(self, VG, phi, Q, dt, z=None, ids=None, Re=None, R=None, observe=0, truth=None):
        """explicit inputs: VG[members, 2], phi[members], z[members, nz, 2]; ids[nz] shared"""
        B = self.members
        VG, phi = _f32(VG, (B, 2)), _f32(phi, (B,))
        z = None if z is None else _f32(z, (B, -1, 2))
        ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
        Q, Re, R, truth = (None if a is None else _f32(a) for a in (Q, Re, R, truth))
        nz = 0 if z is None else z.shape[1]
        _chk(self.L.slamgpu_ens_sim(self.h, _ptr(VG), _ptr(phi), _ptr(z), _ptr(ids), nz, _ptr(Q), _ptr(Re), _ptr(R), dt, int(observe), _ptr(truth)))
        self._nz = nz if observe else 0

    def sim_noise(self, V, G, phi_true, Q, dt, step, z_true=None, ids=None, Re=None, R=None, observe=0, truth=None, Qe=None,
                  noise=NOISE_CONTROL | NOISE_HEADING | NOISE_SENSOR):
        """shared noise-free inputs; every member draws its own (Philox stream 5, counter (member, step, 5, q))"""
        z_true = None if z_true is None else _f32(z_true, (-1, 2))
        ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
        Q, Qe, Re, R, truth = (None if a is None else _f32(a) for a in (Q, Qe, Re, R, truth))
        nz = 0 if z_true is None else z_true.shape[0]
        _chk(self.L.slamgpu_ens_sim_noise(self.h, V, G, phi_true, _ptr(z_true), _ptr(ids), nz, int(step), _ptr(Q), _ptr(Qe), _ptr(Re), _ptr(R), dt,
                                              int(observe), _ptr(truth), int(noise)))
        self._nz = nz if observe else 0

    def last_inputs(self):
        """(VG[members, 2], phi[members], z[members, nz, 2]) the last step used"""
        B = self.members
        VG, phi, z = np.zeros((B, 2), np.float32), np.zeros(B, np.float32), np.zeros((B, self._nz, 2), np.float32)
        _chk(self.L.slamgpu_ens_last_inputs(self.h, _ptr(VG), _ptr(phi), _ptr(z)))
        return VG, phi, z

    def dims(self):
        d = np.zeros(self.members, np.int32)
        _chk(self.L.slamgpu_ens_dims(self.h, _ptr(d)))
        return d

    def poses(self):
        """(xyt[members, 3], Pvv[members, 3, 3]) in double"""
        out = np.zeros((self.members, 12))
        _chk(self.L.slamgpu_ens_poses(self.h, _ptr(out)))
        return out[:, :3].copy(), out[:, 3:].reshape(-1, 3, 3).copy()

    def state(self, b, want_P=True):
        x = np.zeros(self.cap_dim, np.float32)
        P = np.zeros((self.cap_dim, self.cap_dim), np.float32) if want_P else None
        d = _chk(self.L.slamgpu_ens_state(self.h, b, _ptr(x), _ptr(P), self.cap_dim))
        return x[:d].copy(), (np.ascontiguousarray(P[:d, :d]) if want_P else None)

    def slab(self, b):
        """member b's whole slab: x[ld], P[cap_dim, ld], padding included"""
        x, P = np.zeros(self.ld, np.float32), np.zeros((self.cap_dim, self.ld), np.float32)
        _chk(self.L.slamgpu_ens_slab(self.h, b, _ptr(x), _ptr(P)))
        return x, P

    def upload(self, b, x, P):
        x, P = _f32(x), _f32(P)
        _chk(self.L.slamgpu_ens_upload(self.h, b, x.shape[0], _ptr(x), _ptr(P), P.shape[1]))

    def status(self):
        s = np.zeros(self.members, np.int32)
        _chk(self.L.slamgpu_ens_status(self.h, _ptr(s)))
        return s

    def consistency(self):
        """[members, 6]: CONSISTENCY_FIELDS"""
        out = np.zeros((self.members, 6))
        _chk(self.L.slamgpu_ens_consistency(self.h, _ptr(out)))
        return out

    def consistency_reset(self):
        _chk(self.L.slamgpu_ens_consistency_reset(self.h))

    def run_noise(self, steps, z_true, ids, Q, Re, R, Qe=None, noise=NOISE_CONTROL | NOISE_HEADING | NOISE_SENSOR):
        """len(steps) steps of sim_noise in one launch: steps is a TAPE_STEP_DTYPE array (pack_tape), z_true[total, 2] and ids[total] hold
        the observations of all of them.  Bit for bit what the sim_noise calls leave; a bad tape is refused whole"""
        if steps is not None:
            steps = np.ascontiguousarray(steps)
            if steps.dtype != TAPE_STEP_DTYPE:
                raise TypeError("steps must have TAPE_STEP_DTYPE")
        K = 0 if steps is None else steps.shape[0]
        z_true = None if z_true is None else _f32(z_true, (-1, 2))
        ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
        total = 0 if z_true is None else z_true.shape[0]
        Q, Qe, Re, R = (None if a is None else _f32(a) for a in (Q, Qe, Re, R))
        _chk(self.L.slamgpu_ens_run_noise(self.h, _ptr(steps), K, _ptr(z_true), _ptr(ids), total, _ptr(Q), _ptr(Qe), _ptr(Re), _ptr(R), int(noise)))
        if K:
            self._nz = int(steps[-1]["nz"]) if steps[-1]["observe"] else 0

    def trace_enable(self, capacity):
        """retain the records of the last `capacity` steps that were given a truth; 0 turns the trace off and frees it"""
        _chk(self.L.slamgpu_ens_trace_enable(self.h, int(capacity)))

    def trace_info(self):
        """(first, next, capacity): records [first, next) are retained"""
        first, nxt, cap = C.c_int64(), C.c_int64(), C.c_int32()
        _chk(self.L.slamgpu_ens_trace_info(self.h, C.byref(first), C.byref(nxt), C.byref(cap)))
        return first.value, nxt.value, cap.value

    def trace_fetch(self, first, count, out=None, step=None):
        """(records[count, 6] in double: CONSISTENCY_FIELDS over the members of one step, tags[count]) of records [first, first + count)"""
        out = np.zeros((count, 6)) if out is None else out
        step = np.zeros(count, np.uint32) if step is None else step
        _chk(self.L.slamgpu_ens_trace_fetch(self.h, int(first), int(count), _ptr(out), _ptr(step)))
        return out, step

    def moments(self, D=None, exclude_status=0, want_C=True, want_Pbar=True):
        """The sample mean[D] and (population) covariance C[D, D] of the members' leading D state components, and the mean Pbar[D, D] of
        their own P, over the members whose dimension reaches D, whose status has none of the bits of exclude_status and whose state is
        finite: a dict of mean, C, Pbar (None where not wanted), counted, left_out, pivot.  D defaults to the smallest member's
        dimension.  (slamgpu_ens_moments; moments_summary turns it into ratios)"""
        D = int(self.dims().min()) if D is None else int(D)
        n = max(D, 0)
        mean = np.zeros(n)
        Cm = np.zeros((n, n)) if want_C else None
        Pb = np.zeros((n, n)) if want_Pbar else None
        counted, left_out, pivot = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(self.L.slamgpu_ens_moments(self.h, D, int(exclude_status), _ptr(mean), _ptr(Cm), _ptr(Pb), C.byref(counted), C.byref(left_out),
                                        C.byref(pivot)))
        return {"mean": mean, "C": Cm, "Pbar": Pb, "counted": counted.value, "left_out": left_out.value, "pivot": pivot.value}
