"""The host's genealogy row book (slam_amd/csrc/rows.h: RowBook, DenseLayout) on its own, no GPU: tests/rows/rows_driver.cpp, built as a
plain program with the address and undefined-behaviour sanitizers, runs seeded random scripts of the book's operations; what it
returns and lists must be what tests/rows_model.py says, line for line, and the book's invariants must hold after every operation."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

from rows_model import RowModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 32  # sizeof(ObsPacket): eight int32 (slam_amd/csrc/kernels.h)
N_SCRIPTS = 240


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows") / "rows_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "rows", "rows_driver.cpp"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.splitlines()
    return run


class Script:
    """a random script, the model's lines for it, and the placed landmarks and the live buffers after each operation"""

    def __init__(self, seed):
        rng = self.rng = np.random.default_rng(seed)
        # both edges of the row capacity: 2 rows, the compact layout's 40, one row per landmark and one more
        self.cap_nf = cap_nf = int(rng.integers(1, 60))
        cap_rows = [2, 40, cap_nf + 1][seed % 3]
        self.compact = cap_rows != cap_nf + 1
        self.m = RowModel(cap_nf, cap_rows)
        self.ops, self.expect, self.placed, self.live, self.checks = [], [], [], [], []
        self.stats = dict(emptied=0, free_empty=0, unused=0, revived=0, nothing=0, grown=0, round_trips=0, refused=0)
        self.emit("init %d %d" % (cap_nf, cap_rows), 0)
        for _ in range(int(rng.integers(12, 30))):
            self.between()
            self.step()

    def emit(self, op, ret, check=None):
        self.ops.append(op)
        self.expect.append(self.m.line(op.split()[0], ret))
        self.placed.append(dict(self.m.where))
        self.live.append(dict(self.m.live))
        self.checks.append(check)

    def nf(self):
        return len(self.m.where)

    def between(self):
        rng, m = self.rng, self.m
        u = rng.random()
        if u < 0.04:
            nf = int(rng.integers(0, self.cap_nf + 1))
            m.reset(nf)
            self.emit("reset %d" % nf, 0)
        elif u < 0.08:
            m.flip_all(self.nf())
            self.emit("flip_all %d" % self.nf(), 0)
        elif u < 0.12:
            m.rebuild()
            self.emit("rebuild", 0, "ascending")
        elif u < 0.24:
            # to the device and back: as book_push / book_pull (nf entries) or pp_push / pp_pull (all of them) do
            n_lmk = self.nf() if rng.random() < 0.5 else self.cap_nf
            t = m.export(self.cap_nf)
            self.emit("export %d" % self.cap_nf, 0)
            assert m.import_(self.nf(), n_lmk, t) == 0
            self.emit("import %d %d" % (self.nf(), n_lmk), 0, "ascending")
            self.stats["round_trips"] += 1
        elif u < 0.30:
            # tables that cannot be: refused, nothing changes
            t = m.export(self.cap_nf)
            self.emit("export %d" % self.cap_nf, 0)
            before = (dict(m.where), list(m.in_use), list(m.free), dict(m.live))
            if self.nf() and rng.random() < 0.6:
                l = int(rng.integers(0, self.nf()))
                t["row"][l] = bad = int(rng.choice([m.cap_rows, m.cap_rows + 5, -1]))
                self.emit("corrupt %d %d" % (l, bad), 0)
                nf, ret = self.nf(), 2
            else:
                nf, ret = int(rng.choice([self.cap_nf + 1, -1])), 1
            assert m.import_(nf, self.cap_nf, t) == ret
            assert before == (m.where, m.in_use, m.free, m.live)
            self.emit("import %d %d" % (nf, self.cap_nf), ret, "unchanged")
            self.stats["refused"] += 1
        elif u < 0.34 and m.cap_rows < self.cap_nf + 1:
            self.grow()

    def grow(self):
        self.m.grow(self.cap_nf + 1)
        self.compact = False
        self.emit("grow %d" % (self.cap_nf + 1), 0, "descending")
        self.stats["grown"] += 1

    def step(self):
        rng, m = self.rng, self.m
        if rng.random() < 0.1:  # an update that writes nothing
            self.emit("open 0", m.open(False))
            self.emit("chunks", m.live_chunks())
            m.close(self.compact)
            self.emit("close %d" % self.compact, 0)
            self.stats["nothing"] += 1
            return
        if not m.free:  # (do_update's guard: a compact context out of rows goes to plain rows first)
            self.grow()
        nf = self.nf()
        placed = list(rng.permutation(nf))
        style = rng.random()
        n_obs = int(rng.integers(0, min(nf, 6) + 1))
        n_cons = nf - n_obs if style < 0.15 else (int(rng.integers(0, nf - n_obs + 1)) if style < 0.5 else 0)  # (all the rest: several rows empty at once)
        obs, cons, rest = placed[:n_obs], placed[n_obs:n_obs + n_cons], placed[n_obs + n_cons:]
        revive = [int(l) for l in rest[:int(rng.integers(0, 3))]] if rng.random() < 0.2 else []
        n_new = int(rng.integers(0, min(3, self.cap_nf - nf) + 1))
        new = list(range(nf, nf + n_new))
        if rng.random() < 0.5:
            new.reverse()  # (not in the order nf + k)
        sharded = rng.random() < 0.2
        self.emit("open 1", m.open(True))
        for l in cons:
            self.emit("move %d 1" % l, m.move(int(l), True))
        for l in obs:
            self.emit("move %d %d" % (l, not sharded), m.move(int(l), not sharded))
        for l in revive:
            m.place_new(l, True)
            self.emit("new %d 1" % l, 0)
        for l in new:
            m.place_new(l, False)
            self.emit("new %d 0" % l, 0)
        self.emit("chunks", m.live_chunks())
        fresh = -1 if sharded else m.e
        m.fresh = fresh
        self.emit("fresh %d" % fresh, 0)
        self.stats["emptied"] = max(self.stats["emptied"], len(m.emptied))
        self.stats["unused"] += not m.landmarks_in(m.e)
        self.stats["revived"] += len(revive)
        resort = self.compact  # (as do_update: a compact context closes every step with it, a plain-row one never)
        m.close(resort)
        if not m.free:
            self.stats["free_empty"] += 1
        self.emit("close %d" % resort, 0, "descending" if resort else None)


def _ints(s):
    return [int(x) for x in s.split(",")] if s else []


def _parse(line):
    return {k: _ints(v) for k, v in re.findall(r"(\w+)=\[([^\]]*)\]", line)}


def test_book_equals_model_and_keeps_its_invariants(driver):
    total = dict()
    scripts = [Script(seed) for seed in range(N_SCRIPTS)]
    everything = driver([op for s in scripts for op in s.ops])  # (one run of the driver: every script begins with its init)
    assert len(everything) == 2 * sum(len(s.ops) for s in scripts)
    at = 0
    for seed, s in enumerate(scripts):
        out = everything[at:at + 2 * len(s.ops)]
        at += len(out)
        assert out[0::2] == s.expect, next((i, s.ops[i], a, b) for i, (a, b) in enumerate(zip(out[0::2], s.expect)) if a != b)
        cap_rows, prev = None, None
        for i, (op, placed, live, check) in enumerate(zip(s.ops, s.placed, s.live, s.checks)):
            lists, st = _parse(out[2 * i]), _parse(out[2 * i + 1])
            where = (seed, i, op)
            cap_rows = len(st["ref"])
            in_step = op.split()[0] in ("open", "move", "new", "chunks", "fresh") and not op.startswith("open 0")
            # the counts are the placed landmarks, row by row
            assert sum(st["ref"]) == len(placed), where
            count = collections.Counter(placed.values())
            assert st["ref"] == [count.get(r, 0) for r in range(cap_rows)], where
            assert all(st["row"][l] == r for l, r in placed.items()), where
            assert all(st["live"][l] == v for l, v in live.items()), where
            # the rows in use: exactly those with a count, once each (but for the open row); pos is the inverse
            opened = int(re.search(r"ret=(-?\d+)", out[2 * i]).group(1)) if op == "open 1" else (prev if in_step else -1)
            prev = opened
            used = {r for r in range(cap_rows) if st["ref"][r] > 0}
            assert len(set(lists["in_use"])) == len(lists["in_use"]) and set(lists["in_use"]) == used - {opened}, where
            inverse = [-1] * cap_rows
            for q, r in enumerate(lists["in_use"]):
                inverse[r] = q
            assert st["pos"] == inverse, where
            # free and in use partition the rows (but for the open one; the rows a step emptied wait for its close)
            assert len(set(lists["free"])) == len(lists["free"]) and not set(lists["free"]) & set(lists["in_use"]), where
            if not in_step:
                assert sorted(lists["free"] + lists["in_use"]) == list(range(cap_rows)), where
            if check == "descending":
                assert lists["free"] == sorted(lists["free"], reverse=True), where
            if check == "ascending":
                assert lists["in_use"] == sorted(lists["in_use"]) and lists["free"] == sorted(lists["free"], reverse=True), where
            if check == "unchanged":
                q = 2 * (i - (2 if s.ops[i - 1].startswith("corrupt") else 1))
                assert out[q].split(" ", 2)[2] == out[2 * i].split(" ", 2)[2] and out[q + 1] == out[2 * i + 1], where
        for k, v in s.stats.items():
            total[k] = max(total.get(k, 0), v) if k == "emptied" else total.get(k, 0) + v
    # the scripts reached what they were written to reach
    assert total["emptied"] >= 3 and total["free_empty"] > 0 and total["unused"] > 0 and total["revived"] > 0, total
    assert total["nothing"] > 0 and total["grown"] > 0 and total["round_trips"] >= 100 and total["refused"] >= 50, total


def test_dense_layout(driver):
    def capacity_today(cap_nf):  # the big-packet ring's slot: header + idf[cap] + zf[2 cap] + zn[2 cap] + row[cap] + rows[cap + 1], to 256 bytes
        return (HEADER + 4 * cap_nf + 4 * 4 * cap_nf + 4 * (2 * cap_nf + 1) + 255) // 256 * 256

    for cap_nf in (1, 39, 40, 117, 1000):
        cap = int(driver(["capacity %d %d" % (HEADER, cap_nf)])[0].split()[1])
        assert cap == capacity_today(cap_nf)
        for m, nc, n, n_rows in ((0, 0, 0, 0), (1, 0, 0, 1), (cap_nf, 0, 0, cap_nf), (cap_nf // 2, cap_nf - cap_nf // 2, 0, cap_nf),
                                 (cap_nf, 0, cap_nf, cap_nf + 1)):
            f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", driver(["layout %d %d %d %d %d" % (HEADER, m + nc, m, n, n_rows)])[0])}
            assert f["idf"] == HEADER and f["zf"] == f["idf"] + 4 * (m + nc) and f["zn"] == f["zf"] + 8 * m and f["row"] == f["zn"] + 8 * n
            assert f["rows"] == f["row"] + 4 * (m + nc) and f["used"] == f["rows"] + 4 * n_rows
            assert f["used"] <= cap, (cap_nf, m, nc, n, n_rows)
