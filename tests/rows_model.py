"""The rules of the genealogy row book (slam_amd/csrc/rows.h), stated again without its arrays: which row every placed landmark is in,
which record buffer of a landmark is live, the ordered list of rows in use and the stack of free rows.  tests/test_rows_cpu.py holds
the C++ to it, operation by operation.

The rules:
  - a landmark is PLACED once a step put a new landmark there, or a reset / an import said so; a placed landmark is in exactly one row;
  - a row is IN USE while some placed landmark is in it; the list of rows in use changes only where a row fills (appended) or empties
    (the last of the list takes its place); the other rows are FREE, on a stack;
  - a step opens the row on top of the free stack (none, if it writes nothing); every landmark it writes moves there and, unless it is
    new, flips its live buffer; what it reports for a moved landmark is where it was BEFORE: row | live << 30 | fresh << 29, fresh
    meaning "in the row the last update opened", where the caller allows the bit;
  - the rows a step empties join the free stack only when it closes, behind the opened row if nothing went there; a close that is
    asked to and that pushed anything leaves the stack descending (lowest row on top);
  - reset: landmarks [0, nf) placed in row 0, every other row free, lowest on top; the live buffers stay;
  - what comes back from the device (import) places landmarks [0, nf) where the tables say and lists the rows in use ascending; a count
    or a row out of range is refused and changes nothing."""

LIVE, FRESH = 1 << 30, 1 << 29


class RowModel:
    def __init__(self, cap_nf, cap_rows):
        self.cap_nf, self.cap_rows = cap_nf, cap_rows
        self.live = {}    # landmark -> buffer, 0 where never written
        self.reset(0)

    # ---- whole-book operations ----
    def reset(self, nf):
        self.where = {l: 0 for l in range(nf)}   # placed landmark -> row
        self.fresh = -1
        self._lists_from_rows()

    def _lists_from_rows(self):
        used = set(self.where.values())
        self.in_use = sorted(used)
        self.free = sorted((r for r in range(self.cap_rows) if r not in used), reverse=True)
        self.e = -1

    def rebuild(self):
        self._lists_from_rows()

    def grow(self, new_rows):
        self.free = sorted(self.free + list(range(self.cap_rows, new_rows)), reverse=True)
        self.cap_rows = new_rows

    def flip_all(self, nf):
        for l in range(nf):
            self.live[l] = self.live.get(l, 0) ^ 1

    def landmarks_in(self, r):
        return [l for l, x in self.where.items() if x == r]

    # ---- a step ----
    def open(self, writes):
        self.emptied = []
        self.e = self.free.pop() if writes else -1
        return self.e

    def _leave(self, l):
        r = self.where[l]
        self.where[l] = self.e
        if not self.landmarks_in(r):
            i = self.in_use.index(r)
            self.in_use[i] = self.in_use[-1]
            self.in_use.pop()
            self.emptied.append(r)

    def move(self, l, fresh_ok):
        r, buf = self.where[l], self.live.get(l, 0)
        self.live[l] = buf ^ 1
        self._leave(l)
        return r | (LIVE if buf else 0) | (FRESH if fresh_ok and r == self.fresh else 0)

    def place_new(self, l, held):
        if held:
            self._leave(l)
        else:
            self.where[l] = self.e
        self.live[l] = 0

    def live_chunks(self):
        top = max([self.e] + self.in_use)
        return top // 4 + 1

    def close(self, resort):
        pushed = list(self.emptied)
        if self.e >= 0:
            if self.landmarks_in(self.e):
                self.in_use.append(self.e)
            else:
                pushed.insert(0, self.e)
        self.free += pushed
        if resort and pushed:
            self.free.sort(reverse=True)
        self.e = -1

    # ---- to the device and back ----
    def export(self, n_lmk):
        return dict(row={l: self.where.get(l, 0) for l in range(n_lmk)}, live={l: self.live.get(l, 0) for l in range(n_lmk)})

    def import_(self, nf, n_lmk, tables):
        """0: taken over; 1: count out of range; 2: a row out of range"""
        if not (0 <= nf <= self.cap_nf and nf <= n_lmk <= self.cap_nf):
            return 1
        if any(not 0 <= tables["row"][l] < self.cap_rows for l in range(nf)):
            return 2
        self.where = {l: tables["row"][l] for l in range(nf)}
        for l in range(n_lmk):
            self.live[l] = tables["live"][l]
        self._lists_from_rows()
        return 0

    def line(self, op, ret):
        return "%s ret=%d in_use=[%s] free=[%s]" % (op, ret, ",".join(map(str, self.in_use)), ",".join(map(str, self.free)))
