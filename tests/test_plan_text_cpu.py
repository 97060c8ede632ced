"""The inline plan at the head of the specialised and counted update kernels (update_step.inl; kernels.hip: scan_totals / scan_prefix,
find_ancestor_win; device_math.h: dpp_i) as the compiler makes it, against the figures of the same kernels built from the three source
files of the commit before the plan was trimmed (tests/golden/plan_text_parent.json):
  the ancestor window is read as LDS -- no flat load of it is left;
  the DPP moves of the double scans' row_shr steps carry bound_ctrl:1 and no v_mov_b32 of the zero they used to keep;
  the window's bounds are still the DPP min / max reductions, in every per-step kernel;
  no scratch, and no more vector registers than before.
No GPU needed: hipcc cross-compiles both builds with the Makefile's flags (as tests/test_counted_cpu.py does).

The parent's figures are a recorded fixture, not a second compile: a checkout need not carry the history to `git show` the parent's
files from.  They were taken by this module's own figures() from the assembly of the parent's device_math.h, kernels.hip and
update_step.inl (commit 65b2320), compiled with the same command and flags as below:
python tests/test_plan_text_cpu.py k_strict.s k_fast.s > tests/golden/plan_text_parent.json"""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import DATA

ROOT = os.path.dirname(DATA)
SRC = os.path.join(ROOT, "slam_amd", "csrc")
INC = os.path.join(ROOT, "include")
KERNEL = re.compile(r"^_ZN\d+slam_(?:strict|fast)\d+(update_(?:kernel|kernel_special|kernel_wide|kernel_counted)I\w+?E)Ev\w*:")
K_COUNTED = 8   # kernels.h: kCountedMax
SPECS = (1, 2)  # kernels.h: kUpdateSpecs
# the commit before this test, as figures(): the last tree whose double scans kept their zeros and whose window was read through flat loads
PARENT = os.path.join(os.path.dirname(DATA), "tests", "golden", "plan_text_parent.json")
ZERO_MOV = re.compile(r"^v_mov_b32(?:_e32)? v\d+, 0$")


def parse(path):
    """{kernel (the mangled name from `update_` to the end of its template arguments): (instructions, descriptor)}"""
    code, desc, cur, dcur = {}, {}, None, None
    for ln in open(path):
        s = ln.strip()
        m = KERNEL.match(s)
        if m and cur is None:
            cur = code.setdefault(m.group(1), [])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and s and not s.startswith((";", ".")):
            cur.append(s)
        m = re.match(r"\.amdhsa_kernel (\S+)", s)
        if m:
            k = KERNEL.match(m.group(1) + ":")
            dcur = desc.setdefault(k.group(1), {}) if k else None
        m = re.match(r"\.amdhsa_(\w+) (\d+)$", s)
        if m and dcur is not None:
            dcur[m.group(1)] = int(m.group(2))
    assert set(code) == set(desc)
    return {k: (code[k], desc[k]) for k in code}


def count(code, pred):
    return sum(1 for c in code if pred(c))


def figures(code, desc):
    """what the comparisons with the parent need of a kernel"""
    return {"mov0": count(code, ZERO_MOV.match), "flat": count(code, lambda c: c.startswith("flat_")), "vgpr": desc["next_free_vgpr"],
            "dpp_min": count(code, lambda c: c.startswith("v_min_i32_dpp")), "dpp_max": count(code, lambda c: c.startswith("v_max_i32_dpp")),
            "dpp_mov_bound_ctrl": count(code, lambda c: c.startswith("v_mov_b32_dpp") and "bound_ctrl" in c)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{"tree": {build: {kernel: (instructions, descriptor)}}, "parent": {build: {kernel: figures()}}}: every per-step update kernel of
    both builds"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(SRC, "Makefile")).read()
    builds = {"strict": re.search(r"^STRICT := (.*)$", mk, re.M).group(1).split(), "fast": re.search(r"^FAST := (.*)$", mk, re.M).group(1).split()}
    tmp = tmp_path_factory.mktemp("plan")
    outs = {b: str(tmp / ("k_%s.s" % b)) for b in builds}
    procs = [subprocess.Popen([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + SRC, "-I" + INC, *builds[b], "-S", "--cuda-device-only",
                               "-o", outs[b], os.path.join(SRC, "kernels.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for b in outs]
    assert all(p.wait() == 0 for p in procs)
    return {"tree": {b: parse(outs[b]) for b in builds}, "parent": json.load(open(PARENT))}


def planned_kernels():
    """the 4 update_kernel_special and the 32 update_kernel_counted of a build"""
    for s in SPECS:
        for p in (0, 1):
            yield "update_kernel_specialILi%dELi%dEE" % (s, p)
            for m in range(1, K_COUNTED + 1):
                yield "update_kernel_countedILi%dELi%dELi%dEE" % (s, p, m)


def each_planned(asm):
    for build, ks in asm["tree"].items():
        for name in planned_kernels():
            yield build, name, ks[name], asm["parent"][build][name]


def test_every_planned_kernel_is_in_both_trees(asm):
    for tree in asm.values():
        assert sorted(tree) == ["fast", "strict"]
        for build, ks in tree.items():
            assert len(list(planned_kernels())) == 36 and all(k in ks for k in planned_kernels()), build
    for build, ks in asm["tree"].items():
        assert set(ks) == set(asm["parent"][build]), build


def test_the_window_is_not_read_through_flat_loads(asm):
    """Counted kernels: no flat_ memory instruction at all.  update_kernel_special: exactly two, neither of them the plan's -- the
    record of a re-observed landmark beyond the staged kStage in the second pass (update_step.inl: `if (k < kStage)`: staged in LDS, or
    read from memory), one flat_load_dwordx4 and one flat_load_dword, as the parent has them (the counted kernels have no staging and
    no such loop).  The parent holds 19 more in every one of them: the window's 16 pivots and 16-byte reads."""
    for build, name, (code, _), old in each_planned(asm):
        flat = [c.split()[0] for c in code if c.startswith("flat_")]
        was = old["flat"]
        print(build, name, flat, was)
        if "counted" in name:
            assert flat == [], (build, name, flat)
        else:
            assert sorted(flat) == ["flat_load_dword", "flat_load_dwordx4"], (build, name, flat)
        assert was - len(flat) == 19, (build, name, was, len(flat))


def test_row_shr_moves_of_the_sums_carry_bound_ctrl(asm):
    """Every v_mov_b32_dpp with a row_shr control carries bound_ctrl:1, but for exactly eight: the four row_shr steps of each of the
    kernel's two wave_max_f reductions (device_math.h: dpp_f_or; the maximum weight of the estimate's terms, in the plan and at the
    tail), whose lanes without a source must read the maximum's identity, -inf, and not 0: the min / max helpers are not the sums'.
    The moves of the sums -- the halves of the doubles of wave_scan_d, 4 row_shr steps per scan, 2 moves per step; the plan alone scans
    four doubles, the tail two more -- all carry it; the parent's carried none."""
    for build, name, (code, _), old in each_planned(asm):
        shr = [c for c in code if c.startswith("v_mov_b32_dpp") and "row_shr" in c]
        bare = [c for c in shr if "bound_ctrl:1" not in c]
        assert len(shr) - len(bare) >= 6 * 4 * 2, (build, name, len(shr), len(bare))
        assert len(bare) == 8, (build, name, bare)
        assert old["dpp_mov_bound_ctrl"] == 0, (build, name)


def test_the_zeros_are_gone(asm):
    """at least 32 fewer plain `v_mov_b32 vX, 0` than the same kernel of the parent (two per row_shr step of a double scan)"""
    for build, name, (code, _), old in each_planned(asm):
        now, was = count(code, ZERO_MOV.match), old["mov0"]
        print(build, name, was, now)
        assert was - now >= 32, (build, name, was, now)


def test_no_scratch_and_no_more_registers(asm):
    for build, name, (code, desc), old in each_planned(asm):
        odesc = {"next_free_vgpr": old["vgpr"]}
        print(build, name, desc["next_free_vgpr"], odesc["next_free_vgpr"])
        assert desc["private_segment_fixed_size"] == 0 and count(code, lambda c: c.startswith("scratch_")) == 0, (build, name)
        assert desc["next_free_vgpr"] <= odesc["next_free_vgpr"], (build, name, desc["next_free_vgpr"], odesc["next_free_vgpr"])


def test_window_bounds_stay_reductions_over_the_wave(asm):
    """Every per-step kernel -- general, specialised, counted -- still reduces the ancestor window's bounds over the wave with the DPP
    min / max helpers (six v_min_i32_dpp and six v_max_i32_dpp per search; identities that are not 0, so `old` and bound_ctrl off
    stay): reading them from the first and the last lane in use was measured for the specialised kernels and not kept
    (profiles/plan_trim.txt)."""
    dpp_min = lambda c: c.startswith("v_min_i32_dpp")  # noqa: E731
    dpp_max = lambda c: c.startswith("v_max_i32_dpp")  # noqa: E731
    for build, ks in asm["tree"].items():
        general = [k for k in ks if k.startswith(("update_kernelI", "update_kernel_wideI"))]
        assert len(general) >= 17, (build, sorted(ks))
        for k in general + list(planned_kernels()):
            n_min, n_max = count(ks[k][0], dpp_min), count(ks[k][0], dpp_max)
            assert n_min >= 6 and n_max == n_min, (build, k, n_min, n_max)
            assert (n_min, n_max) == (asm["parent"][build][k]["dpp_min"], asm["parent"][build][k]["dpp_max"]), (build, k)


if __name__ == "__main__":  # the fixture: see the module's docstring
    import sys
    print(json.dumps({b: {k: figures(*v) for k, v in sorted(parse(f).items())} for b, f in zip(("strict", "fast"), sys.argv[1:3])}, indent=0))
