// The host's genealogy row book and the dense layout of a host-made observation packet.  Plain C++: nothing of HIP and nothing of the
// context, so that tests/rows/rows_driver.cpp can drive it alone (tests/test_rows_cpu.py, against tests/rows_model.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "row_bits.h"

namespace slamgpu {

// Which genealogy row (kernels.h: gen) every landmark uses, which landmarks use every row, and which record buffer of every landmark is
// live.  The association is global, so the host knows all of it: a step that writes landmarks opens a row for them, the landmarks it
// writes move there, and a row whose last landmark moved on can be opened again.
// What holds between two calls (while a step is open: with its row in neither list):
//   - count(r) is the number of placed landmarks l with row_of(l) == r; a placed landmark is one that place_new, reset or
//     import_tables put into a row;
//   - in_use() holds exactly the rows with count(r) > 0, each once; its ORDER is what the packets and the device's copy carry (a row
//     that empties is replaced by the last one, a row that fills is appended; rebuild and import_tables leave it ascending);
//   - the free stack holds exactly the other rows, each once; reset, rebuild and grow_rows leave it descending, and so does every
//     close(resort) of a book whose steps all close that way (compact contexts), so that open() takes the lowest free row.
// A step writes a landmark once at most (do_update refuses a landmark re-observed twice; a second move would take it out of the open
// row, which is in neither list yet), and open(true) needs a free row (one row per landmark and one more: there always is; a compact
// context of a mid-size map goes to plain rows before it runs out).
class RowBook {
  public:
    enum Import { kImportOk = 0, kImportBadCount, kImportBadRow };
    struct Tables {  // what the device's copies are made of: [cap_nf] [cap_nf] [cap_rows]
        const int32_t *row, *live, *count;
    };

    void init(int cap_nf, int cap_rows) {
        erow.assign((size_t) cap_nf, 0);
        live_flag.assign((size_t) cap_nf, 0);
        seen_step.assign((size_t) cap_nf, 0);
        refcnt.assign((size_t) cap_rows, 0);
        live_pos.assign((size_t) cap_rows, -1);
        reset(0);
    }
    // every landmark [0, nf) in row 0 (own slot): after upload, flatten, a settling unpack.  The live flags stay as they are
    void reset(int nf) {
        fresh_row = -1;
        std::fill(refcnt.begin(), refcnt.end(), 0);
        std::fill(live_pos.begin(), live_pos.end(), -1);
        std::fill(erow.begin(), erow.end(), 0);
        live_rows.clear();
        free_rows.clear();
        for (int r = cap_rows() - 1; r >= (nf > 0 ? 1 : 0); r--) free_rows.push_back(r);  // back() = lowest free row
        if (nf > 0) {
            refcnt[0] = nf;
            add_live(0);
        }
    }
    // the row lists follow from the reference counts (tables that came back from the device)
    void rebuild() {
        std::fill(live_pos.begin(), live_pos.end(), -1);
        live_rows.clear();
        free_rows.clear();
        for (int r = cap_rows() - 1; r >= 0; r--)
            if (refcnt[(size_t) r] == 0) free_rows.push_back(r);  // back() = lowest free row
        for (int r = 0; r < cap_rows(); r++)
            if (refcnt[(size_t) r] > 0) add_live(r);
    }
    // a compact context becomes a plain-row one: rows [cap_rows(), new_rows) join the free ones
    void grow_rows(int new_rows) {
        const int old_rows = cap_rows();
        refcnt.resize((size_t) new_rows, 0);
        live_pos.resize((size_t) new_rows, -1);
        for (int r = old_rows; r < new_rows; r++) free_rows.push_back(r);
        std::sort(free_rows.begin(), free_rows.end(), std::greater<int32_t>());  // back() = lowest free row
    }
    // the records of landmarks [0, nf) now live in their other buffer (flatten, a settling unpack); all of them in buffer 0 (upload)
    void flip_all(int nf) {
        for (int l = 0; l < nf; l++) live_flag[(size_t) l] ^= 1;
    }
    void clear_live() { std::fill(live_flag.begin(), live_flag.end(), 0); }

    // ---- one update's step: open, move / place_new for every landmark it writes, close ----
    // The rows the step empties stay out of the free stack until close(): the launch still reads their records through them.
    // `writes` false: the update writes no landmark and opens no row (-1)
    int open(bool writes) {
        emptied.clear();
        e_new = -1;
        if (writes) {
            e_new = free_rows.back();
            free_rows.pop_back();
        }
        return e_new;
    }
    // landmark l, re-observed or consolidated, moves to the open row and its records to its other buffer; returns its packed row
    // word BEFORE the move: row | live buffer << 30 | fresh << 29 (the fresh bit only where the caller may use it)
    int32_t move(int l, bool fresh_ok) {
        const int r = erow[(size_t) l];
        const int32_t word = r | (live_flag[(size_t) l] ? kRowLiveBit : 0) | (fresh_ok && r == fresh_row ? kRowFreshBit : 0);
        live_flag[(size_t) l] ^= 1;
        leave(l);
        return word;
    }
    // slot l holds a new landmark from this update on: its first records go to buffer 0.  `held`: the slot was placed before (a dead
    // slot of the per-particle association comes back) and leaves the row it was in
    void place_new(int l, bool held) {
        if (held) {
            leave(l);
        } else {
            erow[(size_t) l] = e_new;
            refcnt[(size_t) e_new]++;
        }
        live_flag[(size_t) l] = 0;
    }
    // chunks of four rows up to the highest row in use, the open one included: what a resample of a compact context copies
    int live_chunks(int e) const {
        int top = e;
        for (int r : live_rows) top = std::max(top, r);
        return (top >> 2) + 1;  // (top = -1: 0 chunks)
    }
    // the open row is in use from now on (or free again: nothing moved there); the rows the step emptied can be opened again.
    // `resort`: keep the free stack lowest-first where the step changed it out of order, so that the rows in use stay dense at the
    // bottom (compact contexts copy chunks [0, live_chunks) on a resample)
    void close(bool resort) {
        const bool unused = e_new >= 0 && refcnt[(size_t) e_new] == 0;
        if (e_new >= 0) {
            if (unused) free_rows.push_back(e_new);
            else add_live(e_new);
        }
        for (int r : emptied) free_rows.push_back(r);
        if (resort && (!emptied.empty() || unused)) std::sort(free_rows.begin(), free_rows.end(), std::greater<int32_t>());
        e_new = -1;
    }

    // ---- the hand-over to the device and back ----
    Tables tables() const { return {erow.data(), live_flag.data(), refcnt.data()}; }
    // the first n_lmk landmark entries and every row's count into the caller's staging
    void export_tables(int n_lmk, int32_t *erow_out, int32_t *live_out, int32_t *ref_out) const {
        std::copy(erow.begin(), erow.begin() + n_lmk, erow_out);
        std::copy(live_flag.begin(), live_flag.begin() + n_lmk, live_out);
        std::copy(refcnt.begin(), refcnt.end(), ref_out);
    }
    // the tables of nf landmarks as the device left them (n_lmk >= nf entries are taken over); the row lists follow from the counts.
    // A count or a row out of range is refused and nothing changes (*bad: the landmark whose row it is)
    Import import_tables(int nf, int n_lmk, const int32_t *erow_in, const int32_t *live_in, const int32_t *ref_in, int *bad = nullptr) {
        if (nf < 0 || nf > cap_nf() || n_lmk < nf || n_lmk > cap_nf()) return kImportBadCount;
        for (int l = 0; l < nf; l++)
            if (erow_in[l] < 0 || erow_in[l] >= cap_rows()) {
                if (bad) *bad = l;
                return kImportBadRow;
            }
        std::copy(erow_in, erow_in + n_lmk, erow.begin());
        std::copy(live_in, live_in + n_lmk, live_flag.begin());
        std::copy(ref_in, ref_in + cap_rows(), refcnt.begin());
        rebuild();
        return kImportOk;
    }
    // (compact contexts: the device's landmark table names row and buffer of every landmark; the counts are made anew from it)
    void clear_counts() { std::fill(refcnt.begin(), refcnt.end(), 0); }
    void set_entry(int l, int r, bool live) {
        erow[(size_t) l] = r;
        live_flag[(size_t) l] = live ? 1 : 0;
        refcnt[(size_t) r]++;
    }

    // ---- reading ----
    int cap_nf() const { return (int) erow.size(); }
    int cap_rows() const { return (int) refcnt.size(); }
    int row_of(int l) const { return erow[(size_t) l]; }
    int live_of(int l) const { return live_flag[(size_t) l]; }
    int count(int r) const { return refcnt[(size_t) r]; }
    int pos(int r) const { return live_pos[(size_t) r]; }
    const std::vector<int32_t> &in_use() const { return live_rows; }
    const std::vector<int32_t> &free_stack() const { return free_rows; }
    // the row the last update opened, while nothing but the resample the next update launch applies has touched it: records of its
    // landmarks sit in the source slot itself (-1: none)
    int fresh() const { return fresh_row; }
    void set_fresh(int r) { fresh_row = r; }
    // the observation step that last re-observed landmark l (do_update's duplicate check)
    bool seen(int l, uint32_t step) const { return seen_step[(size_t) l] == step; }
    void mark_seen(int l, uint32_t step) { seen_step[(size_t) l] = step; }

  private:
    void add_live(int r) {
        live_pos[(size_t) r] = (int32_t) live_rows.size();
        live_rows.push_back(r);
    }
    void remove_live(int r) {
        const int p = live_pos[(size_t) r], last = live_rows.back();
        live_rows[(size_t) p] = last;
        live_pos[(size_t) last] = p;
        live_rows.pop_back();
        live_pos[(size_t) r] = -1;
    }
    void leave(int l) {  // landmark l from its row into the open one
        const int r = erow[(size_t) l];
        if (--refcnt[(size_t) r] == 0) {
            remove_live(r);
            emptied.push_back(r);
        }
        erow[(size_t) l] = e_new;
        refcnt[(size_t) e_new]++;
    }

    std::vector<uint32_t> seen_step;  // [cap_nf]
    std::vector<int32_t> live_flag;   // [cap_nf] which record buffer of every landmark is live (flips when it is written)
    std::vector<int32_t> erow;        // [cap_nf] row of every landmark
    std::vector<int32_t> refcnt;      // [cap_rows] landmarks using each row
    std::vector<int32_t> free_rows;   // stack of unused rows
    std::vector<int32_t> live_rows;   // rows with refcnt > 0
    std::vector<int32_t> live_pos;    // [cap_rows] position in live_rows, -1 if not there
    std::vector<int32_t> emptied;     // rows the open step has emptied
    int fresh_row = -1;
    int e_new = -1;                   // the open step's row
};

// The dense layout of a host-made big packet: behind a header of `header` bytes
//   int32 idf[m + cons]; float zf[2 m]; float zn[2 n]; int32 row[m + cons]; int32 rows[n_rows]
// as byte offsets from the packet's start, and the bytes it takes.  A device-made packet of a map of C landmarks has the same layout
// at its capacity (m + cons = m = n = C).
struct DenseLayout {
    size_t idf, zf, zn, row, rows, used;
    static DenseLayout of(size_t header, size_t m_plus_cons, size_t m, size_t n, size_t n_rows) {
        DenseLayout L;
        L.idf = header;
        L.zf = L.idf + sizeof(int32_t) * m_plus_cons;
        L.zn = L.zf + sizeof(float) * 2 * m;
        L.row = L.zn + sizeof(float) * 2 * n;
        L.rows = L.row + sizeof(int32_t) * m_plus_cons;
        L.used = L.rows + sizeof(int32_t) * n_rows;
        return L;
    }
    // a ring slot: every landmark re-observed and as many new ones, every row in use, rounded up to 256 bytes
    static size_t capacity_bytes(size_t header, size_t cap_nf) { return (of(header, cap_nf, cap_nf, cap_nf, cap_nf + 1).used + 255) / 256 * 256; }
};

}  // namespace slamgpu
