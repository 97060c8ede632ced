"""Helpers of the tests of the ensemble's K-step run and trace (include/slamgpu.h: slamgpu_ens_run_noise, slamgpu_ens_trace_*): the
trace's float64 model, tapes as lists of per-step dicts, the twin route (one sim_noise per step) and bit-for-bit snapshots of a handle.
The models of the filter and of the noise stay tests/ekf_ens_model.py's."""
import numpy as np

f32, f64 = np.float32, np.float64


def same_bits(a, b):
    """bit-for-bit equality of two arrays of one dtype (float32, float64 or integers)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def trace_record(values):
    """the trace's record of one step from the members' own values of that step, values[members, 6] (what the accumulators gain in
    the step): the float64 sum over the members"""
    return np.asarray(values, f64).sum(axis=0)


def trace_records(per_step_values):
    return np.array([trace_record(v) for v in per_step_values]).reshape(-1, 6)


def step_dict(k, V, G, phi_true, dt, truth=None, observe=0, z_true=None, ids=None):
    return dict(step=k, V=V, G=G, phi_true=phi_true, dt=dt, truth=truth, observe=observe, z_true=z_true, ids=ids)


def drive_single(ens, tape, nz, noise=7):
    """the twin route: one sim_noise per step of the tape, in tape order"""
    for d in tape:
        ob = bool(d.get("observe", 0))
        ens.sim_noise(d["V"], d["G"], d["phi_true"], nz["Q"], d["dt"], d["step"], d.get("z_true") if ob else None, d.get("ids") if ob else None,
                      nz["Re"], nz["R"], int(ob), truth=d.get("truth"), Qe=nz["Qe"], noise=noise)


def drive_run(ens, tape, nz, cuts=None, noise=7):
    """the K-step route: the tape in calls of the given lengths (None: one call)"""
    import slam_amd
    at = 0
    for n in (cuts or [len(tape)]):
        steps, z_true, ids = slam_amd.pack_tape(tape[at:at + n])
        ens.run_noise(steps, z_true, ids, nz["Q"], nz["Re"], nz["R"], Qe=nz["Qe"], noise=noise)
        at += n
    assert at == len(tape)


def snapshot(ens, inputs=True):
    """everything the contract speaks of, as bytes-comparable arrays"""
    out = dict(dims=ens.dims(), status=ens.status(), acc=ens.consistency())
    for b in range(ens.members):
        out["x%d" % b], out["P%d" % b] = ens.slab(b)
    if inputs:
        out["VG"], out["phi"], out["z"] = ens.last_inputs()
    first, nxt, cap = ens.trace_info()
    out["trace_info"] = np.array([first, nxt, cap], np.int64)
    if cap:
        out["trace"], out["tags"] = ens.trace_fetch(first, nxt - first)
    return out


def identical(a, b):
    """the keys that differ (empty: identical)"""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    return [k for k in a if not same_bits(a[k], b[k])]


def world_tape(n_steps, observe_at, dt, wheel_base, landmarks, seed=0, truth_every=1):
    """a synthetic run: the true pose driven by smooth controls, at the steps of observe_at {step: list of landmark indices} the
    noise-free ranges and bearings of those landmarks (ids = the indices).  Starts at the origin, as a fresh filter does"""
    rng = np.random.default_rng(seed)
    t = np.zeros(3, f32)
    lm = np.asarray(landmarks, f64)
    tape = []
    for k in range(n_steps):
        V, G = 3.0 + 0.2 * rng.standard_normal(), 0.04 * np.sin(0.3 * k)
        t = np.array([t[0] + V * dt * np.cos(G + t[2]), t[1] + V * dt * np.sin(G + t[2]), t[2] + V * dt * np.sin(G) / wheel_base], f32)
        d = step_dict(k, float(V), float(G), float(t[2]), dt, truth=t.copy() if k % truth_every == 0 else None)
        if k in observe_at:
            idx = np.asarray(observe_at[k], np.int64)
            dl = lm[idx] - t[:2].astype(f64)
            d.update(observe=1, z_true=np.stack([np.hypot(dl[:, 0], dl[:, 1]), np.arctan2(dl[:, 1], dl[:, 0]) - t[2]], axis=1).astype(f32).reshape(-1, 2),
                     ids=idx.astype(np.int32))
        tape.append(d)
    return tape
