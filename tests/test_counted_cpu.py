"""The counted instantiations of the update launch (kernels.hip: update_kernel_counted<SPEC, WPAR, M>: update_kernel_special with the
packet's number of re-observed landmarks compiled in) as the compiler makes them: all of them present, no scratch, the records kept in
registers instead of staged in LDS, the head and the tail of the specialised kernels kept.
No GPU needed: hipcc cross-compiles both builds with the Makefile's flags (as tests/test_update_tail_cpu.py does)."""
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
K_COUNTED = 8  # kernels.h: kCountedMax
SPECS = (1, 2)  # kernels.h: kUpdateSpecs


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{build: {kernel (the mangled name from `update_` to the end of its template arguments): (instructions, descriptor)}}: every
    per-step update kernel of both builds; labels, directives and comments left out of the instructions; the descriptor: its
    .amdhsa_ entries with a number"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(SRC, "Makefile")).read()
    builds = {"strict": re.search(r"^STRICT := (.*)$", mk, re.M).group(1).split(), "fast": re.search(r"^FAST := (.*)$", mk, re.M).group(1).split()}
    tmp = tmp_path_factory.mktemp("counted")
    outs = {name: str(tmp / ("k_%s.s" % name)) for name in builds}
    procs = [subprocess.Popen([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + SRC, "-I" + INC, *flags, "-S", "--cuda-device-only",
                               "-o", outs[name], os.path.join(SRC, "kernels.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
             for name, flags in builds.items()]
    assert all(p.wait() == 0 for p in procs)
    res = {}
    for name in builds:
        code, desc, cur, dcur = {}, {}, None, None
        for ln in open(outs[name]):
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
        assert set(code) == set(desc), name
        res[name] = {k: (code[k], desc[k]) for k in code}
    return res


def counted_name(s, p, m):
    return "update_kernel_countedILi%dELi%dELi%dEE" % (s, p, m)


def special_name(s, p):
    return "update_kernel_specialILi%dELi%dEE" % (s, p)


def each_counted(ks):
    for s in SPECS:
        for p in (0, 1):
            for m in range(1, K_COUNTED + 1):
                yield s, p, m, ks[counted_name(s, p, m)]


def count(code, prefix):
    return sum(1 for c in code if c.startswith(prefix))


def tail_of(code):
    bars = [i for i, c in enumerate(code) if c.startswith("s_barrier")]
    assert bars
    return code[bars[-1] + 1:]


def test_every_counted_instantiation_exists(asm):
    for build, ks in asm.items():
        got = sorted(k for k in ks if "update_kernel_counted" in k)
        assert got == sorted(counted_name(s, p, m) for s in SPECS for p in (0, 1) for m in range(1, K_COUNTED + 1)), (build, got)


def test_counted_kernels_fit_their_registers(asm):
    """no scratch, at most 256 vector registers (two workgroups per CU at most: nothing up to there costs occupancy)"""
    for build, ks in asm.items():
        for s, p, m, (code, desc) in each_counted(ks):
            print(build, s, p, m, desc["next_free_vgpr"], desc["next_free_sgpr"], desc["private_segment_fixed_size"])
            assert desc["private_segment_fixed_size"] == 0, (build, s, p, m)
            assert desc["next_free_vgpr"] <= 256, (build, s, p, m, desc["next_free_vgpr"])
            assert count(code, "scratch_") == 0 and count(code, "buffer_store") == 0 and count(code, "buffer_load") == 0, (build, s, p, m)


def test_counted_kernels_stage_no_records(asm):
    """The records are not staged in LDS between the passes.  A counted kernel holds fewer LDS instructions than update_kernel_special
    of its spec and parity -- fewer stores and fewer loads -- and its 16-byte LDS stores (what is left: the ancestor windows) are as
    many whatever M is and fewer than the specialised kernel's by at least the kStage / 2 records of the smaller staging."""
    for build, ks in asm.items():
        for s in SPECS:
            for p in (0, 1):
                sp = ks[special_name(s, p)][0]
                w128 = set()
                for m in range(1, K_COUNTED + 1):
                    code = ks[counted_name(s, p, m)][0]
                    got = {w: (count(code, w), count(sp, w)) for w in ("ds_", "ds_write", "ds_read", "ds_write_b128")}
                    print(build, s, p, m, got)
                    assert all(a < b for a, b in got.values()), (build, s, p, m, got)
                    assert got["ds_write_b128"][0] <= got["ds_write_b128"][1] - K_COUNTED // 2, (build, s, p, m, got)
                    w128.add(got["ds_write_b128"][0])
                assert len(w128) == 1, (build, s, p, w128)


def test_counted_kernels_load_exactly_their_records(asm):
    """no clamped duplicates: one more re-observed landmark is one more record -- five more global loads over the kernel's text (the
    16-byte and the 4-byte half of the record, on the fresh and on the slot-then-record path, and the slot)"""
    for build, ks in asm.items():
        for s in SPECS:
            for p in (0, 1):
                loads = [count(ks[counted_name(s, p, m)][0], "global_load") for m in range(1, K_COUNTED + 1)]
                print(build, s, p, loads)
                assert all(b - a == 5 for a, b in zip(loads, loads[1:])), (build, s, p, loads)
                assert loads[-1] < count(ks[special_name(s, p)][0], "global_load"), (build, s, p, loads)


def test_counted_tail_reads_nothing(asm):
    """the tail properties of the specialised kernels: behind the last barrier no vector load, no wait for vector memory, no scalar load"""
    for build, ks in asm.items():
        for s, p, m, (code, _) in each_counted(ks):
            tail = tail_of(code)
            got = {"global_load": count(tail, "global_load"), "s_load": count(tail, "s_load"),
                   "vmcnt": sum(1 for c in tail if c.startswith("s_waitcnt") and "vmcnt" in c)}
            assert got == {"global_load": 0, "vmcnt": 0, "s_load": 0}, (build, s, p, m, got)


def test_counted_kernels_keep_the_barriers_of_the_specialised_ones(asm):
    """the same head and tail as update_kernel_special of the spec and parity: as many s_barrier"""
    for build, ks in asm.items():
        for s, p, m, (code, _) in each_counted(ks):
            assert count(code, "s_barrier") == count(ks[special_name(s, p)][0], "s_barrier"), (build, s, p, m)
