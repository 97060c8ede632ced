"""ctypes binding of the device EKF-SLAM filter (include/slamgpu.h: slamgpu_ekf_*), in the manner of capi.py: no fallback, a
missing library or GPU is an error."""
import contextlib
import ctypes as C

import numpy as np

from .capi import SlamGpuError, load_library, _f32, _ptr

EKF_STATUS_NOT_PD = 1  # SLAMGPU_EKF_STATUS_NOT_PD
ASSOC_NEW, ASSOC_DISCARD = -1, -2


class EkfConfig(C.Structure):  # slamgpu_ekf_config
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("max_landmarks", C.c_int32), ("use_heading", C.c_int32),
                ("batch_update", C.c_int32), ("association_known", C.c_int32), ("wheel_base", C.c_float), ("sigma_phi", C.c_float),
                ("gate_reject", C.c_float), ("gate_augment", C.c_float), ("external_stream", C.c_uint64)]


_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, f = C.c_void_p, C.c_int32, C.c_float
        L.slamgpu_ekf_create.argtypes = [C.POINTER(EkfConfig), C.POINTER(vp)]
        L.slamgpu_ekf_destroy.argtypes = [vp]
        L.slamgpu_ekf_destroy.restype = None
        L.slamgpu_ekf_sim.argtypes = [vp, f, f, vp, f, f, vp, vp, i32, vp, vp, i32]
        L.slamgpu_ekf_predict.argtypes = [vp, f, f, vp, f]
        L.slamgpu_ekf_observe_heading.argtypes = [vp, f]
        L.slamgpu_ekf_associate.argtypes = [vp, vp, i32, vp, vp]
        L.slamgpu_ekf_update.argtypes = [vp, vp, vp, i32, vp]
        L.slamgpu_ekf_augment.argtypes = [vp, vp, i32, vp]
        L.slamgpu_ekf_dim.argtypes = [vp]
        L.slamgpu_ekf_pose.argtypes = [vp, vp, vp]
        L.slamgpu_ekf_state.argtypes = [vp, vp, vp, i32]
        L.slamgpu_ekf_block.argtypes = [vp, vp, i32, vp]
        L.slamgpu_ekf_upload.argtypes = [vp, i32, vp, vp, i32]
        L.slamgpu_ekf_status.argtypes = [vp, C.POINTER(i32)]
        L.slamgpu_ekf_sync.argtypes = [vp]
        L.slamgpu_ekf_local_begin.argtypes = [vp, vp, i32, i32]
        L.slamgpu_ekf_local_end.argtypes = [vp]
        L.slamgpu_ekf_local_info.argtypes = [vp, vp]
        L.slamgpu_ekf_lookup.argtypes = [vp, vp, i32, vp]
        L.slamgpu_ekf_remove.argtypes = [vp, vp, i32]
        L.slamgpu_ekf_feature_stats.argtypes = [vp, vp, vp, vp, C.POINTER(i32)]
        _bound = True
    return L


def _chk(rc):
    if rc < 0:
        raise SlamGpuError(rc, load_library().slamgpu_last_error().decode())
    return rc


class EkfGpu:
    """One EKF-SLAM filter resident on the GPU: EKFSLAM::sim per call of sim(), or its stages one by one."""

    def __init__(self, max_landmarks, use_heading=False, batch_update=True, association_known=False, wheel_base=4.0, sigma_phi=0.0,
                 gate_reject=4.0, gate_augment=25.0, device=0, external_stream=0):
        self.L = _lib()
        cfg = EkfConfig(C.sizeof(EkfConfig), device, max_landmarks, int(use_heading), int(batch_update), int(association_known), wheel_base,
                        sigma_phi, gate_reject, gate_augment, external_stream)
        h = C.c_void_p()
        _chk(self.L.slamgpu_ekf_create(C.byref(cfg), C.byref(h)))
        self.h, self.cfg = h, cfg

    def close(self):
        if self.h:
            self.L.slamgpu_ekf_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def dim(self):
        return _chk(self.L.slamgpu_ekf_dim(self.h))

    def sim(self, V, G, Q, dt, phi, z=None, ids=None, Re=None, R=None, observe=0):
        z = None if z is None else _f32(z, (-1, 2))
        ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
        Q, Re, R = (None if a is None else _f32(a) for a in (Q, Re, R))
        _chk(self.L.slamgpu_ekf_sim(self.h, V, G, _ptr(Q), dt, phi, _ptr(z), _ptr(ids), 0 if z is None else z.shape[0], _ptr(Re), _ptr(R), int(observe)))

    def predict(self, V, G, Q, dt):
        Q = _f32(Q)
        _chk(self.L.slamgpu_ekf_predict(self.h, V, G, _ptr(Q), dt))

    def observe_heading(self, phi):
        _chk(self.L.slamgpu_ekf_observe_heading(self.h, phi))

    def associate(self, z, Re):
        """labels[nz]: feature >= 0, ASSOC_NEW or ASSOC_DISCARD"""
        z, Re = _f32(z, (-1, 2)), _f32(Re)
        lab = np.zeros(z.shape[0], np.int32)
        _chk(self.L.slamgpu_ekf_associate(self.h, _ptr(z), z.shape[0], _ptr(Re), _ptr(lab)))
        return lab

    def update(self, zf, idf, R):
        zf, idf, R = _f32(zf, (-1, 2)), np.ascontiguousarray(idf, np.int32), _f32(R)
        _chk(self.L.slamgpu_ekf_update(self.h, _ptr(zf), _ptr(idf), idf.shape[0], _ptr(R)))

    def augment(self, zn, Re):
        zn, Re = _f32(zn, (-1, 2)), _f32(Re)
        _chk(self.L.slamgpu_ekf_augment(self.h, _ptr(zn), zn.shape[0], _ptr(Re)))

    def pose(self):
        xyt, Pvv = np.zeros(3), np.zeros((3, 3))
        _chk(self.L.slamgpu_ekf_pose(self.h, _ptr(xyt), _ptr(Pvv)))
        return xyt, Pvv

    def state(self, want_P=True):
        d = self.dim
        x = np.zeros(d, np.float32)
        P = np.zeros((d, d), np.float32) if want_P else None
        _chk(self.L.slamgpu_ekf_state(self.h, _ptr(x), _ptr(P), d))
        return x, P

    def block(self, idx):
        idx = np.ascontiguousarray(idx, np.int32)
        out = np.zeros((idx.shape[0], idx.shape[0]), np.float32)
        _chk(self.L.slamgpu_ekf_block(self.h, _ptr(idx), idx.shape[0], _ptr(out)))
        return out

    def upload(self, x, P):
        x, P = _f32(x), _f32(P)
        _chk(self.L.slamgpu_ekf_upload(self.h, x.shape[0], _ptr(x), _ptr(P), P.shape[1]))

    def status(self):
        s = C.c_int32()
        _chk(self.L.slamgpu_ekf_status(self.h, C.byref(s)))
        return s.value

    def sync(self):
        _chk(self.L.slamgpu_ekf_sync(self.h))

    # ---- local periods (slamgpu_ekf_local_*): the stages above on an active set, one deferred commit ----------------------------
    def local_begin(self, features, max_new=0):
        """features: global feature indices, ascending and distinct; max_new: the features the period may create"""
        f = np.ascontiguousarray(features, np.int32).reshape(-1)
        _chk(self.L.slamgpu_ekf_local_begin(self.h, _ptr(f), f.shape[0], int(max_new)))

    def local_end(self):
        _chk(self.L.slamgpu_ekf_local_end(self.h))

    def local_info(self):
        out = np.zeros(6, np.int32)
        _chk(self.L.slamgpu_ekf_local_info(self.h, _ptr(out)))
        return dict(zip(("open", "k", "new", "max_new", "calls", "commits"), (int(v) for v in out)))

    def lookup(self, ids):
        """known association: the feature of each id, -1 not seen yet"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.zeros(ids.shape[0], np.int32)
        _chk(self.L.slamgpu_ekf_lookup(self.h, _ptr(ids), ids.shape[0], _ptr(out)))
        return out

    # ---- features taken out in place (slamgpu_ekf_remove) and the per-feature counts -----------------------------------------------
    def remove(self, features):
        """features: global feature indices, ascending and distinct; enqueued, does not wait for the device"""
        f = np.ascontiguousarray(features, np.int32).reshape(-1)
        _chk(self.L.slamgpu_ekf_remove(self.h, _ptr(f), f.shape[0]))

    def feature_stats(self):
        """dict(hits, born, last: int32 [nf]; epoch: int)"""
        nf = (self.dim - 3) // 2
        hits, born, last = (np.zeros(nf, np.int32) for _ in range(3))
        epoch = C.c_int32()
        _chk(self.L.slamgpu_ekf_feature_stats(self.h, _ptr(hits), _ptr(born), _ptr(last), C.byref(epoch)))
        return dict(hits=hits, born=born, last=last, epoch=int(epoch.value))

    @contextlib.contextmanager
    def local(self, features, max_new=0):
        """with ekf.local(features, max_new): ... -- the period is committed on the way out, also when the body raises"""
        self.local_begin(features, max_new)
        try:
            yield self
        finally:
            self.local_end()
