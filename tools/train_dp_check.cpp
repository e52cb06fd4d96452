// The rules of data-parallel training (poreover_amd/csrc/po_train_dp_rules.h), the part of the all-reduce that needs no device:
// the same source po_train_group.hip runs.  Plain C++, no HIP: built and run under -fsanitize=address,undefined by
// tests/test_train_dp_cpu.py.  Exit status 0 and "ok" when every case holds.
//
// For n = 0 .. 70, n around 16 384 and the weight counts the device tests use, and R = 1 .. 9: the slices of the partition
// cover [0, n) exactly once (every element is marked in a heap array of exactly n entries), slice r starts where slice r - 1
// ends, every slice but the last is whole 16-byte groups, the slices' group counts differ by one at most with the longer ones
// first, the tail lies in the last slice, and po_dp_slice_of names the slice that holds each group.  The sum: a walk over the
// contributing replicas with po_dp_add against a brute-force loop, bit for bit, with replicas left out, -0.0 and values of
// very different size.
#include "../poreover_amd/csrc/po_train_dp_rules.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
static long checked = 0;

static void fail(const char* what, long n, long a = 0, long b = 0) {
    if (failures < 20) std::printf("FAILED %s (n %ld: %ld, %ld)\n", what, n, a, b);
    ++failures;
}

static void check_partition(int64_t n, int R) {
    ++checked;
    const int64_t nvec = n / 4;
    std::vector<unsigned char> seen((size_t)n, 0);
    int64_t prev_end = 0, prev_groups = -1;
    for (int r = 0; r < R; ++r) {
        int64_t e0, e1;
        po_dp_slice_elems(n, R, r, &e0, &e1);
        if (e0 != prev_end) fail("a slice does not start where the last one ends", n, r, e0);
        if (e0 % 4 != 0) fail("a slice does not start at a 16-byte group", n, r, e0);
        if (r < R - 1 && e1 % 4 != 0) fail("a slice but the last holds part of a group", n, r, e1);
        if (e1 < e0 || e1 > n) fail("slice bounds", n, e0, e1);
        const int64_t g0 = po_dp_slice_begin(nvec, R, r), g1 = po_dp_slice_begin(nvec, R, r + 1);
        if (4 * g0 != e0 || (r < R - 1 && 4 * g1 != e1)) fail("groups and elements disagree", n, r);
        const int64_t groups = g1 - g0;
        if (prev_groups >= 0 && (groups > prev_groups || prev_groups - groups > 1)) fail("uneven slices", n, r, groups);
        prev_groups = groups;
        for (int64_t g = g0; g < g1; ++g)
            if (po_dp_slice_of(nvec, R, g) != r) fail("po_dp_slice_of", n, r, g);
        for (int64_t e = e0; e < e1; ++e) ++seen[(size_t)e];
        prev_end = e1;
    }
    if (prev_end != n) fail("the last slice does not end at n", n, prev_end);
    if (po_dp_slice_begin(nvec, R, 0) != 0 || po_dp_slice_begin(nvec, R, R) != nvec) fail("the ends of the partition", n, R);
    for (int64_t e = 0; e < n; ++e)
        if (seen[(size_t)e] != 1) { fail("coverage", n, e, seen[(size_t)e]); break; }
}

static unsigned bits(float x) {
    unsigned u;
    std::memcpy(&u, &x, 4);
    return u;
}

static void check_sum() {
    const float vals[] = {1e-20f, 3.5f, -0.0f, 1e18f, -1e18f, 0.1f, -7.25e-3f, 16777216.f, 1.f};
    const int NV = (int)(sizeof(vals) / sizeof(vals[0]));
    for (int R = 1; R <= 9; ++R)
        for (unsigned mask = 1; mask < (1u << R); ++mask) {     // every non-empty set of contributing replicas
            for (int shift = 0; shift < NV; ++shift) {
                // the walk the kernel does: the first contributor's value, then po_dp_add in ascending order
                float acc = 0.f;
                bool first = true;
                for (int r = 0; r < R; ++r) {
                    if (!(mask >> r & 1)) continue;
                    const float x = vals[(r + shift) % NV];
                    acc = first ? x : po_dp_add(acc, x);
                    first = false;
                }
                // brute force: the contributors' values listed, then summed left to right in volatile steps
                std::vector<float> list;
                for (int r = 0; r < R; ++r)
                    if (mask >> r & 1) list.push_back(vals[(r + shift) % NV]);
                volatile float want = list[0];
                for (size_t k = 1; k < list.size(); ++k) {
                    volatile float y = list[k];
                    want = want + y;
                }
                if (bits(acc) != bits(want)) fail("the sum in replica order", R, (long)mask, shift);
                ++checked;
            }
        }
    // a lone -0.0 keeps its sign: it is not added to a zero
    if (bits(-0.0f) == bits(po_dp_add(0.f, -0.0f))) fail("-0.0 + 0.0 is +0.0: skipping matters", 0);
    // the order matters, so the rule has to fix it: (1e18 + -1e18) + 1 is 1, 1e18 + (-1e18 + 1) is 0
    if (po_dp_add(po_dp_add(1e18f, -1e18f), 1.f) != 1.f || po_dp_add(1e18f, po_dp_add(-1e18f, 1.f)) != 0.f) fail("association", 0);
    checked += 2;
}

int main() {
    static_assert(PO_DP_MAX_REPLICAS >= 9, "the device tests use up to 8 replicas, this program 9");
    for (int R = 1; R <= 9; ++R) {
        for (int64_t n = 0; n <= 70; ++n) check_partition(n, R);
        for (int64_t d = -40; d <= 40; ++d) check_partition(16384 + d, R);
        for (int64_t n : {11589, 107141, 456309, 893189}) check_partition(n, R);
    }
    check_sum();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok (%ld cases)\n", checked);
    return 0;
}
