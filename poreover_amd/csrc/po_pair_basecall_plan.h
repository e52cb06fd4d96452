// The host-side rules of `pair-basecall`, once: the checks of the pair list and of the output capacities,
// the two pair-major offset tables, and the row mapping (side, output row) -> (read, source row) that pair_table_kernel
// follows.  The device kernel of po_pair_basecall.hip and the host entries use the same functions.  No HIP in this file:
// tools/pair_basecall_check.cpp compiles it alone under sanitizers and holds it against brute-force loops.
//
// Pair i = reads pair_idx[2i] (side 0) and pair_idx[2i + 1] (side 1).  Table `side` holds, pair after pair, one row per
// row of that side's read: y_off[side][i + 1] - y_off[side][i] = the read's rows.  Output row k of pair i on a side comes
// from row sig_off[read] + k of the read-major logits, or (side 1 with reverse2) from row sig_off[read] + (L - 1 - k).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"

#ifdef __HIPCC__
#define PO_PB_HD __host__ __device__
#else
#define PO_PB_HD
#endif

// the item (pair) that owns row `row` of a table of n >= 1 items: the last i with off[i] <= row (ingest_kernel's search)
PO_PB_HD inline int po_pair_table_item(const int64_t* off, int n, int64_t row) {
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= row) lo = mid; else hi = mid; }
    return lo;
}

// the read-major source row of output row `row` of table `side`; *read_out (or NULL) gets the read
PO_PB_HD inline int64_t po_pair_table_source(const int64_t* sig_off, const int32_t* pair_idx, const int64_t* y_off, int n_pairs,
                                             int side, int reverse2, int64_t row, int* read_out) {
    const int i = po_pair_table_item(y_off, n_pairs, row);
    const int r = pair_idx[2 * i + side];
    const int64_t k = row - y_off[i], L = y_off[i + 1] - y_off[i];
    if (read_out) *read_out = r;
    return sig_off[r] + ((side && reverse2) ? L - 1 - k : k);
}

struct PoPairBasecallPlan {
    std::vector<int64_t> y_off[2];   // [n_pairs + 1] each: row offsets of the pairs in table 0 / 1
    int64_t rows[2] = {0, 0};        // rows of each table
    int64_t max_rows[2] = {0, 0};    // the longest item of each table
};

// Checks the pair list against the reads' offsets (sig_off_h[0] == 0, as po_basecall_make_plan has it) and, where given,
// the output capacities (seq1d_off_h: 2 n_pairs + 1 entries, each read's basecall needs room for its rows; seq_off_h:
// n_pairs + 1 entries, from 0, non-decreasing), then fills *p.  Returns PO_OK, or PO_E_ARG / PO_E_CAP with *err naming the
// pair under the name of the entry that asks.  Touches no device.
inline int po_pair_basecall_make_plan(const int64_t* sig_off_h, int n_reads, const int32_t* pair_idx_h, int n_pairs,
                                      const int64_t* seq1d_off_h, const int64_t* seq_off_h, PoPairBasecallPlan* p, std::string* err,
                                      const char* entry = "po_pair_basecall_batch_h") {
    const std::string me = std::string(entry) + ": ";
    if (n_reads < 0) { *err = me + "n_reads " + std::to_string(n_reads); return PO_E_ARG; }
    if (n_pairs < 0) { *err = me + "n_pairs " + std::to_string(n_pairs); return PO_E_ARG; }
    if (seq1d_off_h && seq1d_off_h[0] != 0) { *err = me + "seq1d_off[0] is " + std::to_string(seq1d_off_h[0]) + " (must be 0)"; return PO_E_ARG; }
    if (seq_off_h && seq_off_h[0] != 0) { *err = me + "seq_off[0] is " + std::to_string(seq_off_h[0]) + " (must be 0)"; return PO_E_ARG; }
    for (int side = 0; side < 2; ++side) {
        p->y_off[side].assign((size_t)n_pairs + 1, 0);
        p->rows[side] = p->max_rows[side] = 0;
    }
    for (int i = 0; i < n_pairs; ++i) {
        for (int side = 0; side < 2; ++side) {
            const int64_t r = pair_idx_h[2 * (size_t)i + side];
            if (r < 0 || r >= n_reads) {
                *err = me + "pair " + std::to_string(i) + " names read " + std::to_string(r) + " (reads 0 to " + std::to_string(n_reads - 1) + ")";
                return PO_E_ARG;
            }
            const int64_t L = sig_off_h[r + 1] - sig_off_h[r];
            if (L < 1) {
                *err = me + "pair " + std::to_string(i) + ": read " + std::to_string(r) + " has " + std::to_string(L) + " rows (at least 1)";
                return PO_E_ARG;
            }
            if (seq1d_off_h) {
                const int64_t room = seq1d_off_h[2 * (size_t)i + side + 1] - seq1d_off_h[2 * (size_t)i + side];
                if (room < L) {
                    *err = me + "pair " + std::to_string(i) + ": read " + std::to_string(r) + " has " + std::to_string(L) +
                           " rows and room for " + std::to_string(room) + " characters";
                    return PO_E_CAP;
                }
            }
            p->y_off[side][(size_t)i + 1] = p->y_off[side][i] + L;
            p->max_rows[side] = L > p->max_rows[side] ? L : p->max_rows[side];
        }
        if (seq_off_h && seq_off_h[i + 1] < seq_off_h[i]) {
            *err = me + "pair " + std::to_string(i) + " has room for " + std::to_string(seq_off_h[i + 1] - seq_off_h[i]) + " characters";
            return PO_E_CAP;
        }
    }
    for (int side = 0; side < 2; ++side) p->rows[side] = p->y_off[side][n_pairs];
    return PO_OK;
}
