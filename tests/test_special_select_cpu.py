"""Which instantiation of the update kernel a launch takes (kernels.h: update_special, reached through slamgpu_update_special -- host
arithmetic, no device): every combination of the mode flags maps to a specialised instantiation whose compiled-in values EQUAL the
launch's, or to the general one; never to one that disagrees in a flag, never to one at all for another kernel or under
SLAMGPU_NO_SPECIAL."""
import itertools
import os
import re

from conftest import DATA

ROOT = os.path.dirname(DATA)
# slamgpu.h: bit 0 inline plan, 1 scan kernel's prefix, 2 log-weights, 3 front end, 4 Philox, 5 composed predicts, 6 heading, 7 control noise, 8 resampling
PLAN, SCAN, LOGW, FRONT, PHILOX, COMP, HEADING, NOISE, RESAMPLE = (1 << b for b in range(9))


def lib():
    import slam_amd
    return slam_amd.load_library()


def specs(L):
    out = {}
    s = 1
    while L.slamgpu_update_special_modes(s) >= 0:
        out[s] = L.slamgpu_update_special_modes(s)
        s += 1
    assert L.slamgpu_update_special_modes(0) == -1 and L.slamgpu_update_special_modes(-3) == -1 and L.slamgpu_update_special_modes(s + 5) == -1
    return out


def test_declared_and_counted():
    hdr = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    nbits = int(re.search(r"#define SLAMGPU_UPDATE_MODE_BITS (\d+)", hdr).group(1))
    assert nbits == 9
    assert hdr.index("int slamgpu_update_special(") > hdr.index("#ifdef SLAMGPU_EXPERIMENTAL")
    sp = specs(lib())
    # the two the bench workloads run: configs 3 / 4 (composed predicts) and config 6 (heading observed)
    assert PLAN | PHILOX | COMP | RESAMPLE in sp.values() and PLAN | PHILOX | HEADING | RESAMPLE in sp.values()
    assert len(set(sp.values())) == len(sp) and all(0 <= v < (1 << nbits) for v in sp.values())


def test_every_combination_maps_to_its_own_mode_set_or_to_the_general_instantiation():
    L = lib()
    sp = specs(L)
    hit = set()
    for bits in range(1 << 9):
        s = L.slamgpu_update_special(2, 0, 0, 0, 0, bits)
        assert s == 0 or sp[s] == bits, (bits, s)
        assert (s != 0) == (bits in sp.values()), bits
        hit.add(s)
    assert hit == set(sp) | {0}  # every instantiation is reachable, and so is the general one


def test_other_kernels_and_the_switch_take_the_general_instantiation():
    L = lib()
    sp = specs(L)
    for bits in sp.values():
        assert L.slamgpu_update_special(2, 0, 0, 0, 0, bits) > 0
        for method, arrivals, big, pp, off in itertools.product((1, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1)):
            if (method, arrivals, big, pp, off) == (2, 0, 0, 0, 0):
                continue
            assert L.slamgpu_update_special(method, arrivals, big, pp, off, bits) == 0, (method, arrivals, big, pp, off, bits)
        assert L.slamgpu_update_special(2, 0, 0, 0, 0, bits | (1 << 9)) == 0  # (a bit the table does not know: no match)
