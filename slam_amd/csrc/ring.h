// A ring of `cap` slots that retains the newest entries of an unbounded sequence: entries [first, next) are held, entry r in slot
// r % cap.  Plain C++ (the pose, innovation and path histories of libslamgpu.so keep their counters in one; tests/ring_check.cpp
// checks it against a brute-force model).
#pragma once
#include <cstdint>

struct Ring {
    int32_t cap = 0;  // 0: the ring is off
    int64_t first = 0, next = 0;

    void reset(int32_t capacity) {
        cap = capacity;
        first = next = 0;
    }
    int64_t slot(int64_t r) const { return r % cap; }
    // m entries (0 <= m <= cap) have been written to slots slot(next) .. : a full ring drops its oldest
    void advance(int64_t m) {
        next += m;
        if (next - first > cap) first = next - cap;
    }
    // whether [from, from + count) is retained
    bool check(int64_t from, int64_t count) const { return count >= 0 && from >= first && from + count <= next; }
    // the at most two contiguous runs of slots that hold a retained window: slots [at, at + n0), then slots [0, n1)
    struct Runs {
        int64_t at, n0, n1;
    };
    Runs stretches(int64_t from, int64_t count) const {
        const int64_t at = slot(from), n0 = count < cap - at ? count : cap - at;
        return Runs{at, n0, count - n0};
    }
};
