// Ring (slam_amd/csrc/ring.h) against a brute-force model: a circular buffer written entry by entry with a cursor of its own, no modulo.
// Every (cap, appends, first, count) with cap <= 5 and up to 3 cap + 2 appends, appends of m = 0 .. cap entries at once (a fixed m and
// a varying one).  tests/test_ring_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ring.h"

namespace {

struct Model {
    std::vector<long long> content;  // the entry each slot holds, -1: none
    int cursor = 0;
    long long total = 0;
    explicit Model(int cap) : content((size_t) cap, -1) {}
    void write_one() {
        content[(size_t) cursor] = total++;
        if (++cursor == (int) content.size()) cursor = 0;
    }
    bool retained(long long id) const {
        for (long long e : content)
            if (id >= 0 && e == id) return true;
        return false;
    }
    long long oldest() const {  // == total when nothing is held
        long long lo = total;
        for (long long e : content)
            if (e >= 0 && e < lo) lo = e;
        return lo;
    }
};

long long checks = 0;
#define EXPECT(cond)                                                                                                          \
    do {                                                                                                                      \
        checks++;                                                                                                             \
        if (!(cond)) {                                                                                                        \
            std::fprintf(stderr, "ring_check: %s fails (cap %d, %lld appended, window [%lld, +%lld)), line %d\n", #cond, cap, \
                         m.total, from, count, __LINE__);                                                                     \
            std::exit(1);                                                                                                     \
        }                                                                                                                     \
    } while (0)

void check_state(const Ring &r, const Model &m, int cap) {
    long long from = 0, count = 0;
    EXPECT(r.cap == cap);
    EXPECT(r.next == m.total);
    EXPECT(r.first == m.oldest());
    for (from = r.first; from < r.next; from++) {  // every retained entry sits where slot() says
        const int64_t s = r.slot(from);
        EXPECT(s >= 0 && s < cap);
        EXPECT(m.content[(size_t) s] == from);
    }
    {  // the slot the next append writes is the model's cursor
        from = r.next;
        EXPECT(r.slot(r.next) == m.cursor);
    }
    for (from = -1; from <= m.total + 1; from++) {
        for (count = -1; count <= cap + 2; count++) {
            bool want = count >= 0;
            for (long long id = from; want && id < from + count; id++) want = m.retained(id);
            if (count == 0) want = from >= m.oldest() && from <= m.total;  // an empty window: inside the retained range, its end included
            EXPECT(r.check(from, count) == want);
            if (!want || count == 0) continue;
            const Ring::Runs s = r.stretches(from, count);  // (a window that ends at next, and one that wraps, are among these)
            EXPECT(s.n0 >= 1 && s.n1 >= 0 && s.n0 + s.n1 == count);
            EXPECT(s.at >= 0 && s.at + s.n0 <= cap && s.n1 <= s.at);
            EXPECT(s.n1 == 0 || s.at + s.n0 == cap);
            long long id = from;
            for (int64_t q = 0; q < s.n0; q++) EXPECT(m.content[(size_t) (s.at + q)] == id++);
            for (int64_t q = 0; q < s.n1; q++) EXPECT(m.content[(size_t) q] == id++);
        }
    }
}

void run(int cap, int m0, int step) {  // appends of m0, m0 + step, ... entries (mod cap + 1)
    Ring r;
    r.reset(cap);
    Model m(cap);
    check_state(r, m, cap);
    int batch = m0;
    for (int appends = 0; appends < 3 * cap + 2; appends++) {
        for (int q = 0; q < batch; q++) m.write_one();  // the writer fills slots slot(next) .. and then advances
        r.advance(batch);
        check_state(r, m, cap);
        batch = (batch + step) % (cap + 1);
    }
}

}  // namespace

int main() {
    for (int cap = 1; cap <= 5; cap++)
        for (int m0 = 0; m0 <= cap; m0++)
            for (int step = 0; step <= 2; step++) run(cap, m0, step);
    std::printf("ring_check ok: %lld checks\n", checks);
    return 0;
}
