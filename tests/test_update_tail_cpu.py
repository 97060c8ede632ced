"""The end of the update launch (update_step.inl, behind the step's last barrier: weight prefix, block totals, estimate partials) must
not fetch a pointer from the kernel-argument segment: `ws` is a by-value argument, and `ws.lcum[ws.wpar]` with a run-time parity is a
load of the pointer table in memory -- a vector load and an s_waitcnt vmcnt(0) that also waits for every store of the step, twice in
a row at the end of every block of every launch.  The specialised instantiations have the parity as a template parameter
(update_kernel_special<SPEC, WPAR>) and their three pointers pinned at the head; the general ones select between the two entries.
No GPU needed: hipcc cross-compiles both builds with the Makefile's flags (as tests/test_host_frontend.py does for the scratch guard)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import DATA

ROOT = os.path.dirname(DATA)
SRC = os.path.join(ROOT, "slam_amd", "csrc")
INC = os.path.join(ROOT, "include")
KERNEL = re.compile(r"^(_ZN\d+slam_(?:strict|fast)\d+update_(?:kernel|kernel_special|kernel_wide)I\w+):")


def spec_count():
    """rows of kUpdateSpecs (kernels.h); row 0 is the general instantiation"""
    h = open(os.path.join(SRC, "kernels.h")).read()
    body = re.search(r"constexpr UpdateModes kUpdateSpecs\[\] = \{(.*?)\n\};", h, re.S).group(1)
    return len(re.findall(r"^\s*\{", body, re.M))


@pytest.fixture(scope="module")
def tails(tmp_path_factory):
    """{build: {mangled kernel name: the instructions behind its last s_barrier, out-of-line blocks included}}, every per-step update
    kernel of both builds (labels, directives and comments left out); whole kernels under the key build + "/code".
    """
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(SRC, "Makefile")).read()
    builds = {"strict": re.search(r"^STRICT := (.*)$", mk, re.M).group(1).split(), "fast": re.search(r"^FAST := (.*)$", mk, re.M).group(1).split()}
    tmp = tmp_path_factory.mktemp("tail")
    outs = {name: str(tmp / ("k_%s.s" % name)) for name in builds}
    procs = [subprocess.Popen([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + SRC, "-I" + INC, *flags, "-S", "--cuda-device-only",
                               "-o", outs[name], os.path.join(SRC, "kernels.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
             for name, flags in builds.items()]
    assert all(p.wait() == 0 for p in procs)
    res = {}
    for name in builds:
        kernels, cur = {}, None
        for ln in open(outs[name]):
            s = ln.strip()
            m = KERNEL.match(s)
            if m:
                cur = kernels.setdefault(m.group(1), [])
            elif s.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and s and not s.startswith((";", ".")):
                cur.append(s)
        res[name] = {}
        for k, code in kernels.items():
            bars = [i for i, c in enumerate(code) if c.startswith("s_barrier")]
            assert bars, (name, k)
            res[name][k] = code[bars[-1] + 1:]
        res[name + "/code"] = kernels
    return res


def builds_of(tails):
    return {b: ks for b, ks in tails.items() if not b.endswith("/code")}


def count(tail, what):
    if what == "vmcnt":
        return sum(1 for c in tail if c.startswith("s_waitcnt") and "vmcnt" in c)
    return sum(1 for c in tail if c.startswith(what))


def test_both_parities_of_every_spec_exist(tails):
    n = spec_count()
    assert n >= 3
    for build, ks in builds_of(tails).items():
        special = sorted(re.search(r"update_kernel_specialILi(\d+)ELi(\d+)E", k).groups() for k in ks if "update_kernel_special" in k)
        assert special == sorted((str(s), str(w)) for s in range(1, n) for w in (0, 1)), (build, special)
        # the general FastSLAM 2 kernel of single compact contexts keeps its name: exactly one kernel (tests/test_host_frontend.py)
        assert len([k for k in ks if re.search(r"update_kernelILi2ELi0ELb0E", k)]) == 1, build


def test_specialised_tail_reads_nothing(tails):
    """behind the last barrier: LDS reads, arithmetic, stores -- no vector load, no wait for vector memory, no scalar load"""
    for build, ks in builds_of(tails).items():
        for k, tail in ks.items():
            if "update_kernel_special" not in k:
                continue
            got = {w: count(tail, w) for w in ("global_load", "vmcnt", "s_load")}
            print(build, k, len(tail), got)
            assert got == {"global_load": 0, "vmcnt": 0, "s_load": 0}, (build, k, got)


def test_general_tails_fetch_no_pointer_through_vector_memory(tails):
    """The general instantiations select (update_step.inl: WS_AT), all of them: no vector load and no wait for vector memory behind
    the last barrier.  Two variants keep vector-memory traffic of their own there, which is not the weight scratch's, and are held to
    exactly that:
      update_kernel<*, 2, false> (distributed, compact): the push collective reads the peers' totals-table pointer,
        B.peers[h].gtot[parity], in its loop over the shards (the collectives' own text): one load, one wait;
      update_kernel<2, 1, true> (sharded, plain rows, FastSLAM 2): two s_waitcnt vmcnt(1) for a load issued long before the barrier;
        no load, and nothing waited down to zero."""
    seen = 0
    for build, ks in builds_of(tails).items():
        for k, tail in ks.items():
            if "update_kernel_special" in k:
                continue
            gl, vm = count(tail, "global_load"), count(tail, "vmcnt")
            fl = count(tail, "flat_load") + count(tail, "buffer_load") + count(tail, "scratch_load")
            vm0 = sum(1 for c in tail if c.startswith("s_waitcnt") and "vmcnt(0)" in c)
            print(build, k, len(tail), gl, vm, vm0, fl)
            assert fl == 0, (build, k, fl)
            m = re.search(r"update_kernelILi(\d)ELi(\d)ELb(\d)E", k)
            mode_big = (m.group(2), m.group(3)) if m else ("0", "0")  # (update_kernel_wide: single context, compact)
            if mode_big == ("2", "0"):
                assert (gl, vm, vm0) == (1, 1, 1), (build, k, gl, vm, vm0)
            elif m and (m.group(1), m.group(2), m.group(3)) == ("2", "1", "1"):
                assert (gl, vm0) == (0, 0) and vm <= 2, (build, k, gl, vm, vm0)
            else:
                assert (gl, vm) == (0, 0), (build, k, gl, vm)
            seen += 1
    assert seen == 2 * 17  # both builds: sixteen instantiations of update_kernel and the wide kernel


def test_specialised_head_waits_behind_its_requests(tails):
    """The specialised kernels wait for vector memory for the first time only when the Ctrl words have been requested as well (the scan's
    block totals are pinned behind the head's other requests, update_step.inl): left alone, the compiler waits for the totals inside the
    branch that loads them, before the packet, the queued controls and the Ctrl words are asked for.  The Ctrl words: the two
    single-dword scalar loads at offsets 0 and 8 of one base (Ctrl::live[slot], Ctrl::pend[slot])."""
    for build in builds_of(tails):
        for k, code in tails[build + "/code"].items():
            if "update_kernel_special" not in k:
                continue
            first_wait = next(i for i, c in enumerate(code) if c.startswith("s_waitcnt") and "vmcnt" in c)
            first_load = next(i for i, c in enumerate(code) if c.startswith("global_load"))
            ctrl = {}
            for i, c in enumerate(code):
                m = re.match(r"s_load_dword s\d+, (s\[\d+:\d+\]), 0x([08])$", c)
                if m and i > first_load:
                    ctrl.setdefault(m.group(2), i)
                if len(ctrl) == 2:
                    break
            print(build, k, "first global_load", first_load, "Ctrl words", ctrl, "first vmcnt wait", first_wait)
            assert len(ctrl) == 2 and first_load < max(ctrl.values()) < first_wait, (build, k, first_load, ctrl, first_wait)
