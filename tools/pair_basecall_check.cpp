// The host-side rules of po_pair_basecall_batch_h and po_pair_tables_h (poreover_amd/csrc/po_pair_basecall_plan.h), the
// part of the entries that needs no device.  Plain C++, no HIP: built and run under -fsanitize=address,undefined by
// tests/test_pair_basecall_cpu.py.  Exit status 0 and "ok" when every case holds.
//   - the two offset tables, the totals and the maxima of a plan, against loops over the pairs;
//   - the row mapping (side, output row) -> (read, source row) that pair_table_kernel follows, against a table built pair by
//     pair and row by row: every output row has exactly one source row, it lies inside the read the pair names, and with
//     reverse2 the mapping of side 1 is an involution inside each item; and backwards: every row of a read is the source
//     of exactly one output row of each (pair, side) that names the read;
//   - every refusal, with its code and the pair (or the value) in its message.
// Every table lives in a heap block of exactly its size: a read past its end is a sanitizer report.
#include "../poreover_amd/csrc/po_pair_basecall_plan.h"

#include <cstdio>
#include <map>
#include <utility>

static int failures = 0;

static void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
    ++failures;
}

static std::vector<int64_t> offsets(const std::vector<int64_t>& lens) {
    std::vector<int64_t> off(1, 0);
    for (int64_t L : lens) off.push_back(off.back() + L);
    return off;
}

static void check_case(const std::vector<int64_t>& lens, const std::vector<int32_t>& pairs, int reverse2) {
    const std::vector<int64_t> sig_off = offsets(lens);
    const int n_reads = (int)lens.size(), n_pairs = (int)pairs.size() / 2;
    PoPairBasecallPlan p;
    std::string err;
    if (po_pair_basecall_make_plan(sig_off.data(), n_reads, pairs.data(), n_pairs, nullptr, nullptr, &p, &err) != PO_OK) {
        fail("plan accepted", n_reads, n_pairs);
        return;
    }
    for (int side = 0; side < 2; ++side) {
        // ---- the tables, against loops
        int64_t total = 0, longest = 0;
        if (p.y_off[side].size() != (size_t)n_pairs + 1 || p.y_off[side][0] != 0) fail("table size", side);
        for (int i = 0; i < n_pairs; ++i) {
            const int64_t L = lens[(size_t)pairs[2 * (size_t)i + side]];
            if (p.y_off[side][(size_t)i + 1] - p.y_off[side][i] != L) fail("item length", side, i);
            total += L;
            longest = L > longest ? L : longest;
        }
        if (p.rows[side] != total || p.max_rows[side] != longest) fail("totals and maxima", side);
        // ---- forwards: the expected source of every output row, pair by pair and row by row
        std::vector<int64_t> want;
        std::vector<int> want_read;
        for (int i = 0; i < n_pairs; ++i) {
            const int r = pairs[2 * (size_t)i + side];
            for (int64_t k = 0; k < lens[(size_t)r]; ++k) {
                want.push_back(sig_off[(size_t)r] + ((side == 1 && reverse2) ? lens[(size_t)r] - 1 - k : k));
                want_read.push_back(r);
            }
        }
        if ((int64_t)want.size() != p.rows[side]) fail("rows of a table", side);
        std::map<std::pair<int, int64_t>, int> hits;   // (item, source row) -> output rows that read it
        const std::vector<int64_t> y_off(p.y_off[side]);
        for (int64_t row = 0; row < p.rows[side]; ++row) {
            int read = -1;
            const int item = po_pair_table_item(y_off.data(), n_pairs, row);
            const int64_t src = po_pair_table_source(sig_off.data(), pairs.data(), y_off.data(), n_pairs, side, reverse2, row, &read);
            if (row < y_off[(size_t)item] || row >= y_off[(size_t)item + 1]) fail("the item holds the row", side, (long)row);
            if (src != want[(size_t)row] || read != want_read[(size_t)row]) fail("source row", side, (long)row, (long)src);
            if (src < sig_off[(size_t)read] || src >= sig_off[(size_t)read + 1]) fail("source row inside the read", side, (long)row);
            ++hits[std::make_pair(item, src)];
            // applying the mapping to the row at the source's place in the item leads back (identity without a reversal)
            const int64_t back_row = y_off[(size_t)item] + (src - sig_off[(size_t)read]);
            const int64_t back = po_pair_table_source(sig_off.data(), pairs.data(), y_off.data(), n_pairs, side, reverse2, back_row, nullptr);
            if (back - sig_off[(size_t)read] != row - y_off[(size_t)item]) fail("involution inside the item", side, (long)row);
        }
        // ---- backwards: every row of a named read is the source of exactly one output row of each item that names it
        for (int i = 0; i < n_pairs; ++i) {
            const int r = pairs[2 * (size_t)i + side];
            for (int64_t s = sig_off[(size_t)r]; s < sig_off[(size_t)r + 1]; ++s)
                if (hits[std::make_pair(i, s)] != 1) fail("one output row per source row and item", side, i, (long)s);
        }
    }
}

static void refused(const char* name, const std::vector<int64_t>& sig_off, const std::vector<int32_t>& pairs, int n_pairs,
                    const std::vector<int64_t>* seq1d_off, const std::vector<int64_t>* seq_off, int code, const char* needle) {
    PoPairBasecallPlan p;
    std::string err;
    const std::vector<int64_t> a(sig_off);
    const std::vector<int32_t> b(pairs);
    const int rc = po_pair_basecall_make_plan(a.data(), (int)a.size() - 1, b.data(), n_pairs, seq1d_off ? seq1d_off->data() : nullptr,
                                              seq_off ? seq_off->data() : nullptr, &p, &err);
    if (rc != code || err.find(needle) == std::string::npos || err.find("po_pair_basecall_batch_h: ") != 0) {
        std::printf("FAILED refusal %s: code %d, message \"%s\"\n", name, rc, err.c_str());
        ++failures;
    }
}

int main() {
    // reads of 1, 2, 5, 40 and 333 rows; a read on both sides of one pair, in three pairs, in either role; one read unused
    const std::vector<int64_t> lens = {1, 2, 5, 40, 333, 7};
    const std::vector<std::vector<int32_t>> lists = {
        {0, 0},
        {0, 1},
        {4, 3, 3, 4, 4, 4},
        {2, 3, 3, 2, 2, 2, 1, 2, 2, 0, 4, 2},
        {0, 1, 1, 0, 0, 0, 1, 1},
        {},
    };
    for (const auto& pairs : lists)
        for (int reverse2 = 0; reverse2 < 2; ++reverse2) check_case(lens, pairs, reverse2);
    // every pair of every two of four short reads
    {
        const std::vector<int64_t> small = {3, 1, 4, 2};
        std::vector<int32_t> all;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) { all.push_back(a); all.push_back(b); }
        check_case(small, all, 0);
        check_case(small, all, 1);
    }
    // the search on a table with many items
    {
        std::vector<int64_t> many;
        std::vector<int32_t> pairs;
        for (int i = 0; i < 37; ++i) { many.push_back(1 + (i * 7) % 5); pairs.push_back(i); pairs.push_back(36 - i); }
        check_case(many, pairs, 1);
    }

    const std::vector<int64_t> off = {0, 5, 9, 9, 12};   // read 2 has no rows
    const std::vector<int64_t> cap1 = {0, 5, 9}, tight1 = {0, 5, 8}, shifted1 = {1, 6, 10}, cap = {0, 9}, back = {0, -1}, shifted = {2, 11};
    const std::vector<int64_t> cap2 = {0, 5, 9, 13, 17}, two = {0, 9, 9}, two_back = {0, 9, 8};
    refused("n_pairs -1", off, {0, 1}, -1, nullptr, nullptr, PO_E_ARG, "n_pairs -1");
    refused("index = n_reads", off, {0, 1, 1, 4}, 2, nullptr, nullptr, PO_E_ARG, "pair 1 names read 4");
    refused("negative index", off, {-1, 1}, 1, nullptr, nullptr, PO_E_ARG, "pair 0 names read -1");
    refused("empty read on side 0", off, {0, 1, 2, 1}, 2, nullptr, nullptr, PO_E_ARG, "pair 1: read 2 has 0 rows");
    refused("empty read on side 1", off, {0, 2}, 1, nullptr, nullptr, PO_E_ARG, "pair 0: read 2 has 0 rows");
    refused("decreasing offsets", {0, 5, 3}, {0, 1}, 1, nullptr, nullptr, PO_E_ARG, "pair 0: read 1 has -2 rows");
    refused("short room of read 2", off, {0, 1}, 1, &tight1, &cap, PO_E_CAP, "pair 0: read 1 has 4 rows and room for 3");
    refused("short room in the second pair", off, {0, 1, 1, 0}, 2, &cap2, &two, PO_E_CAP, "pair 1: read 0 has 5 rows and room for 4");
    refused("seq1d_off not from 0", off, {0, 1}, 1, &shifted1, &cap, PO_E_ARG, "seq1d_off[0] is 1");
    refused("seq_off not from 0", off, {0, 1}, 1, &cap1, &shifted, PO_E_ARG, "seq_off[0] is 2");
    refused("seq_off decreases", off, {0, 1}, 1, &cap1, &back, PO_E_CAP, "pair 0 has room for -1");
    {
        const std::vector<int64_t> cap4 = {0, 5, 9, 14, 18};
        refused("seq_off decreases at the second pair", off, {0, 1, 0, 1}, 2, &cap4, &two_back, PO_E_CAP, "pair 1 has room for -1");
    }
    {   // and the same call with nothing wrong
        PoPairBasecallPlan p;
        std::string err;
        const std::vector<int32_t> pr = {0, 1};
        if (po_pair_basecall_make_plan(off.data(), 4, pr.data(), 1, cap1.data(), cap.data(), &p, &err) != PO_OK || !err.empty()) fail("accepted");
    }
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
