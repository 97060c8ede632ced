// Drives slam_amd/csrc/rows.h alone (tests/test_rows_cpu.py builds it with the address and undefined-behaviour sanitizers): a script of
// operations on stdin, one per line; after each, one line with what it returned and the two row lists -- what tests/rows_model.py
// must say too -- and one with the rest of the book's state.
//   init CAP_NF CAP_ROWS | reset NF | rebuild | grow NEW_ROWS | flip_all NF | fresh ROW
//   open WRITES | move L FRESH_OK | new L HELD | chunks | close RESORT
//   export N_LMK | corrupt L ROW | import NF N_LMK        (the exported tables stay with the driver; corrupt changes a row in them)
//   layout HEADER M_PLUS_CONS M N N_ROWS | capacity HEADER CAP_NF
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../slam_amd/csrc/rows.h"

using slamgpu::DenseLayout;
using slamgpu::RowBook;

static void list(const char *name, const std::vector<int32_t> &v) {
    printf(" %s=[", name);
    for (size_t i = 0; i < v.size(); i++) printf(i ? ",%d" : "%d", v[i]);
    printf("]");
}

int main() {
    RowBook book;
    std::vector<int32_t> t_row, t_live, t_ref;  // the exported tables
    int e_new = -1;
    char op[32];
    long a[5];
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        const int got = sscanf(line, "%31s %ld %ld %ld %ld %ld", op, &a[0], &a[1], &a[2], &a[3], &a[4]);
        if (got < 1) continue;
        const std::string o = op;
        long ret = 0;
        if (o == "layout") {
            const DenseLayout L = DenseLayout::of((size_t) a[0], (size_t) a[1], (size_t) a[2], (size_t) a[3], (size_t) a[4]);
            printf("layout idf=%zu zf=%zu zn=%zu row=%zu rows=%zu used=%zu\n", L.idf, L.zf, L.zn, L.row, L.rows, L.used);
            continue;
        }
        if (o == "capacity") {
            printf("capacity %zu\n", DenseLayout::capacity_bytes((size_t) a[0], (size_t) a[1]));
            continue;
        }
        if (o == "init") book.init((int) a[0], (int) a[1]);
        else if (o == "reset") book.reset((int) a[0]);
        else if (o == "rebuild") book.rebuild();
        else if (o == "grow") book.grow_rows((int) a[0]);
        else if (o == "flip_all") book.flip_all((int) a[0]);
        else if (o == "fresh") book.set_fresh((int) a[0]);
        else if (o == "open") ret = e_new = book.open(a[0] != 0);
        else if (o == "move") ret = book.move((int) a[0], a[1] != 0);
        else if (o == "new") book.place_new((int) a[0], a[1] != 0);
        else if (o == "chunks") ret = book.live_chunks(e_new);
        else if (o == "close") book.close(a[0] != 0), e_new = -1;
        else if (o == "export") {
            t_row.assign((size_t) book.cap_nf(), -7);
            t_live.assign((size_t) book.cap_nf(), -7);
            t_ref.assign((size_t) book.cap_rows(), -7);
            book.export_tables((int) a[0], t_row.data(), t_live.data(), t_ref.data());
        } else if (o == "corrupt") t_row[(size_t) a[0]] = (int32_t) a[1];
        else if (o == "import") ret = book.import_tables((int) a[0], (int) a[1], t_row.data(), t_live.data(), t_ref.data());
        else {
            fprintf(stderr, "unknown operation %s\n", op);
            return 2;
        }
        printf("%s ret=%ld", op, ret);
        list("in_use", book.in_use());
        list("free", book.free_stack());
        printf("\nstate fresh=%d", book.fresh());
        std::vector<int32_t> row, live, ref, pos;
        for (int l = 0; l < book.cap_nf(); l++) row.push_back(book.row_of(l)), live.push_back(book.live_of(l));
        for (int r = 0; r < book.cap_rows(); r++) ref.push_back(book.count(r)), pos.push_back(book.pos(r));
        list("row", row);
        list("live", live);
        list("ref", ref);
        list("pos", pos);
        printf("\n");
    }
    return 0;
}
