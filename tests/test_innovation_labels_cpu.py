"""Innovation posterior with every particle's own match (slamgpu_innovation_summary_labels, SLAMGPU_INNOV_SLOT_PER_PARTICLE): the float64
model the GPU tests use (tests/innovation_labels_model.py) is innovation_model with the slot taken per particle -- unanimous labels give
innovation_model.summary's floats, and a set worked by hand gives the hand's answers; the entry point is declared, exported and bound --
no GPU needed for any of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import innovation_labels_model as ilm
import innovation_model as im
from conftest import DATA

ROOT = os.path.dirname(DATA)
f32, f64 = np.float32, np.float64


def _cloud(N, nf, seed):
    rng = np.random.default_rng(seed)
    xv = np.stack([rng.normal(0.0, 1.0, N), -3.0 + rng.normal(0.0, 0.5, N), rng.normal(0.7, 0.1, N)], axis=1).astype(f32)
    lm = rng.uniform(-25.0, 25.0, (nf, 2)) + np.array([40.0, 0.0])
    xf = (lm[None] + rng.normal(0.0, 0.3, (N, nf, 2))).astype(f32)
    A = rng.normal(0.0, 0.2, (N, nf, 2, 2))
    Pf = (A @ A.transpose(0, 1, 3, 2) + 0.01 * np.eye(2)).astype(f32)
    return xv, xf, Pf


def test_unanimous_labels_are_the_known_association_model():
    """labels[i][q] = idf[q]: the same floats as innovation_model.summary, holders and terms included; absent records, a slot twice,
    linear and log weights"""
    N, nf = 37, 4
    xv, xf, Pf = _cloud(N, nf, 11)
    xf[5:9, 2] = np.nan
    Pf[5:9, 2] = np.nan
    rng = np.random.default_rng(3)
    idf = np.array([2, 0, 3, 2, 1], np.int32)
    z = np.stack([rng.uniform(20.0, 60.0, 5), rng.uniform(-1.0, 1.0, 5)], axis=1).astype(f32)
    R = np.array([0.01, 0.0, 0.0, 0.0004], f32)
    for logw, w in ((False, rng.uniform(0.0, 1.0, N).astype(f32)), (True, rng.normal(-700.0, 2.0, N).astype(f32))):
        exp, eh, et = im.summary(xv, w, xf, Pf, z, idf, R, logw)
        got, gh, gt = ilm.summary_labels(xv, w, xf, Pf, z, np.tile(idf, (N, 1)), R, logw)
        assert got.tobytes() == exp.tobytes() and np.array_equal(gh, eh)
        assert list(eh) == [N - 4, N, N, N - 4, N]
        assert np.array_equal(im.bounds(gt, N, got), im.bounds(et, N, exp))


def test_hand_worked_set():
    """4 particles, 3 slots, 2 observations: an absent record, a NEW label, a DISCARD label, an observation nobody matched: to 1e-13"""
    xv, w, xf, Pf, z, labels, R = ilm.hand_set()
    assert (labels == ilm.NEW).any() and (labels == ilm.DISCARD).any() and np.isnan(xf[2, labels[2, 0]]).all()
    got, holders, _ = ilm.summary_labels(xv, w, xf, Pf, z, labels, R)
    exp, eh = ilm.hand_answers()
    assert np.array_equal(holders, eh) and list(eh) == [2, 0]
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    err = np.abs(got[ok] - exp[ok]) / np.maximum(1.0, np.abs(exp[ok]))
    print("hand-worked set: largest relative error %.3g" % err.max())
    assert err.max() <= 1e-13
    assert got[1, 0] == 0.0 and np.isnan(got[1, 1:]).all()
    assert abs(got[0, 0] - 0.375) <= 1e-15 and abs(abs(got[0, 2]) - 2.0 * np.pi / 3.0) < 1e-13
    # a label outside [0, nf) that is neither NEW nor DISCARD is no slot either
    lab2 = labels.copy()
    lab2[1, 0] = 3
    lab2[1, 1] = -7
    again, h2, _ = ilm.summary_labels(xv, w, xf, Pf, z, lab2, R)
    assert again.tobytes() == got.tobytes() and np.array_equal(h2, holders)
    # the mixture's NIS of the entries: the share-0 entry is the one bad entry
    v, bad = ilm.nis(got)
    assert bad == 1 and np.isfinite(v[0]) and np.isnan(v[1])


DECL = (r"int slamgpu_innovation_summary_labels\(slamgpu_ctx \*ctx, const float \*z, int32_t nz, const int32_t \*labels /\* host, \[N\]\[nz\] \*/,\s*"
        r"const float R\[4\], double \*out /\* \[nz\]\[SLAMGPU_INNOV_STRIDE\] \*/, int32_t \*holders /\* \[nz\], may be NULL \*/\);")


def test_header_declares_the_entry_and_the_tag():
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    stable = hdr[:hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")]
    assert re.search(DECL, stable)
    assert re.search(r"#define SLAMGPU_INNOV_SLOT_PER_PARTICLE \(-3\)", stable)
    assert stable.index("int slamgpu_innovation_summary(") < stable.index("int slamgpu_innovation_summary_labels(") < stable.index("int slamgpu_innovation_history_enable(")
    doc = stable[stable.index("The per-particle form"):stable.index("int slamgpu_upload(")]
    for piece in ("Every label >= 0 counts", "slamgpu_set_particle_mutex on, the gates produce no", "a label outside [-2, slamgpu_num_landmarks)",
                  "slamgpu_update_particle and slamgpu_update_labels", "slamgpu_run_particle are NOT recorded", "SLAMGPU_INNOV_SLOT_PER_PARTICLE"):
        assert piece in doc, piece
    assert re.search(r"#define SLAMGPU_ABI_VERSION 3\b", hdr)  # an addition to the stable part: the version stays
    assert ilm.SLOT_PER_PARTICLE == -3 and ilm.NEW == -1 and ilm.DISCARD == -2


def test_library_exports_and_binds_it():
    import slam_amd
    from slam_amd import capi
    out = subprocess.run(["nm", "-D", "--defined-only", slam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT slamgpu_innovation_summary_labels$", out, re.M), "libslamgpu.so does not export slamgpu_innovation_summary_labels"
    assert "slamgpu_innovation_summary_labels" in slam_amd.DECLARED_SYMBOLS
    L = capi.load_library()
    vp, i32 = C.c_void_p, C.c_int32
    assert L.slamgpu_innovation_summary_labels.argtypes == [vp, vp, i32, vp, vp, vp, vp]
    assert capi.INNOV_SLOT_PER_PARTICLE == -3 and callable(capi.SlamGpu.innovation_summary_labels)
    # a null context is refused with the outputs untouched
    outp, hold = np.full((2, 10), -1.0), np.full(2, -1, np.int32)
    z, lab, R = np.ones((2, 2), f32), np.zeros((4, 2), np.int32), np.array([0.01, 0, 0, 0.0004], f32)
    p = lambda x: x.ctypes.data_as(vp)
    assert L.slamgpu_innovation_summary_labels(None, p(z), 2, p(lab), p(R), p(outp), p(hold)) < 0 and L.slamgpu_last_error()
    assert np.all(outp == -1.0) and np.all(hold == -1)
