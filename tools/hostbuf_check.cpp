// PoRagged (poreover_amd/csrc/po_hostbuf.h) against values written out by hand.  Plain C++, no HIP: built and run under
// -fsanitize=address,undefined by tests/test_hostbuf_cpu.py.  Exit status 0 and "ok" when every case holds.
#define PO_HOSTBUF_PURE
#include "../poreover_amd/csrc/po_hostbuf.h"

#include <cstdio>

static int failures = 0;

static void check(const char* name, const std::vector<int64_t>& table, bool ask, const std::vector<int64_t>& off, int64_t base,
                  int64_t total, int64_t max, bool ordered) {
    // the table sits in a heap block of exactly its size: a read past off_h[n] is an AddressSanitizer report
    std::vector<int64_t> exact(table);
    const PoRagged r(exact.data(), (int)exact.size() - 1, ask);
    const bool ok = r.off == off && r.base == base && r.total == total && r.max == max && r.ordered == ordered &&
                    r.bytes() == 8 * table.size();
    if (!ok) { std::printf("FAILED %s\n", name); ++failures; }
}

int main() {
    check("from 0", {0, 8, 48, 69}, false, {0, 8, 48, 69}, 0, 69, 40, true);
    check("from 13", {13, 21, 61, 82}, false, {0, 8, 48, 69}, 13, 69, 40, true);
    check("from 13, order asked for", {13, 21, 61, 82}, true, {0, 8, 48, 69}, 13, 69, 40, true);
    check("n = 1", {5, 9}, true, {0, 4}, 5, 4, 4, true);
    check("n = 1, empty", {7, 7}, true, {0, 0}, 7, 0, 0, true);
    check("empty items", {3, 3, 6, 6, 6, 10}, true, {0, 0, 3, 3, 3, 7}, 3, 7, 4, true);
    check("all empty", {0, 0, 0}, true, {0, 0, 0}, 0, 0, 0, true);
    check("decreasing, asked for", {2, 9, 7, 12}, true, {0, 7, 5, 10}, 2, 10, 7, false);
    check("decreasing below the base, asked for", {4, 1}, true, {0, -3}, 4, -3, 0, false);
    check("decreasing, not asked for", {2, 9, 7, 12}, false, {0, 7, 5, 10}, 2, 10, 7, true);
    check("past 2^31", {int64_t(1) << 32, (int64_t(1) << 32) + 5, (int64_t(1) << 33)}, true, {0, 5, int64_t(1) << 32},
          int64_t(1) << 32, int64_t(1) << 32, (int64_t(1) << 32) - 5, true);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
