"""update_kernel_special<SPEC, WPAR> against the general instantiation (SLAMGPU_NO_SPECIAL=1, read when the context is created): state
and history BIT FOR BIT.  What the specialised kernels do differently from the general one, besides their compiled-in mode flags
(tests/test_gpu_special.py): the weight scratch's parity is a template parameter the launcher picks from the ws.wpar it has just
written, the three pointers the step stores through at its end (weight prefix, block totals, estimate partials) are read at the head
and held in registers, and the scan's block totals are pinned behind the head's other requests.  A launch that took the wrong parity
would write its prefix and totals over the table the same launch is still searching, and its estimate partials into the wrong step.
FastSLAM 2, Philox, both builds.  Sizes: 300 particles -- two tiles, the last one partial (lanes beyond the particle count store a
prefix through the pinned pointer too) -- and 1 024, four tiles.  peek() every 3 steps puts a general launch (no resampling stage
pending: plan_inline = 0) between specialised launches of either parity; every 4 steps the general launches all fall on one parity
and the specialised ones on both.  The helpers are those of tests/test_gpu_special.py."""
import numpy as np
import pytest

from test_gpu_special import assert_same, assert_selected, run, sg, tape_of  # noqa: F401  (sg: fixture)

pytestmark = pytest.mark.gpu


def check(a, b):
    assert_same(a, b)
    # launches that apply a resample and launches that do not (the resample decided in step k is applied by the launch of step k + 1)
    res = np.asarray(a[1][2])[:-1]
    print("%d of %d steps resampled" % (int(res.sum()), len(res)))
    assert res.any() and not res.all(), res
    # the specialised instantiation ran at every launch that carried a resampling stage -- all but the first and, at most, the one after
    # each peek() -- and never under SLAMGPU_NO_SPECIAL
    assert_selected(a, b, True)


@pytest.mark.parametrize("every", [3, 4])
@pytest.mark.parametrize("N", [300, 1024])
@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_webmap_parity_special_equals_general(sg, monkeypatch, math_mode, N, every):
    """example_webmap, the first 60 observation steps: spec 1 (composed predicts; the strict build: the sequential ones)"""
    tape = tape_of("example_webmap", 2, 60)
    assert len(tape["steps"]) == 60
    a = run(sg, monkeypatch, False, tape, N, every=every, method=2, math_mode=math_mode)
    b = run(sg, monkeypatch, True, tape, N, every=every, method=2, math_mode=math_mode)
    check(a, b)


@pytest.mark.parametrize("math_mode", [0, 1], ids=["strict", "fast"])
def test_loop902_parity_special_equals_general(sg, monkeypatch, math_mode):
    """example_loop902, 512 particles, 40 observation steps: spec 2 (the heading is observed at every predict)"""
    tape = tape_of("example_loop902", 2, 40)
    conf = tape["conf"]
    assert bool(conf.SWITCH_HEADING_KNOWN)
    kw = dict(method=2, math_mode=math_mode, use_heading=True, wheel_base=float(conf.WHEELBASE), sigma_phi=float(conf.sigmaT))
    a = run(sg, monkeypatch, False, tape, 512, every=3, **kw)
    b = run(sg, monkeypatch, True, tape, 512, every=3, **kw)
    check(a, b)
