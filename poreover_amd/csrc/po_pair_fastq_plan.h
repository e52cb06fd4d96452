// The host-side index and offset rules of the pair quality stages, once.  No HIP in this file:
// tools/pair_fastq_check.cpp compiles it alone under sanitizers and holds it against brute-force loops.
//
// A pair has four scored items, k = 0 .. 3: seq1 on table 1, seq2 on table 2, the consensus on table 1, the consensus on
// table 2.  Item k is scored on the table of side k & 1; items 0 and 1 are strings of the interleaved 1-D buffer (pair i's
// at seq1d_off[2i + side]), items 2 and 3 the consensus (at seq_off[i]).  The items of a pair whose decode status is not 0
// are empty.  An item is scored in one of two po_qual_batch calls of its kind: the banded one, or — where the band is off
// or the caller flags it (unbanded[4i + k] != 0, the retry of a lost lattice) — the one without a band; in the other call
// it has L = 0.  Each call has a dense label layout of its own; the labels, the odds and the statuses of an item type live
// in buffers that hold the banded layout first and the unbanded one behind it:
//   labels / odds row of base j of item (k, i):  pos[k][i] + j        (pos = off_b[k][i], or total_b[k] + off_u[k][i])
//   status of item (k, i):                       sel[k][i]            (i, or n + i)
#pragma once
#include <cstdint>
#include <vector>

#define PO_PQ_ITEMS 4
#define PO_PQ_NONE 0       // an empty item: L = 0 in both calls
#define PO_PQ_BANDED 1
#define PO_PQ_UNBANDED 2

inline int po_pq_side(int k) { return k & 1; }

struct PoPairFastqPlan {
    int n = 0;
    std::vector<int64_t> off1d[2];              // [n + 1]: off1d[s][i] = seq1d_off[2i + s]; [n] = seq1d_off[2n]
    std::vector<int32_t> len[PO_PQ_ITEMS];      // [n] the scored length of an item (0 where the pair is not decoded)
    std::vector<int32_t> cls[PO_PQ_ITEMS];      // [n] PO_PQ_*
    std::vector<int32_t> len_b[PO_PQ_ITEMS];    // [n] the length in the banded call: what the guides are made for
    std::vector<int64_t> off_b[PO_PQ_ITEMS];    // [n + 1] the banded call's dense label offsets
    std::vector<int64_t> off_u[PO_PQ_ITEMS];    // [n + 1] the unbanded call's
    std::vector<int64_t> pos[PO_PQ_ITEMS];      // [n]
    std::vector<int32_t> sel[PO_PQ_ITEMS];      // [n]
    std::vector<int64_t> cons_off;              // [n + 1] dense offsets of the consensus strings (len[2])
    int64_t total_b[PO_PQ_ITEMS] = {0, 0, 0, 0}, total_u[PO_PQ_ITEMS] = {0, 0, 0, 0};
    int64_t total(int k) const { return total_b[k] + total_u[k]; }
};

// status / len1 / len2 / seq_len: what the pair decoder wrote (n entries each); a negative length counts as 0
inline void po_pair_fastq_make_plan(const int64_t* seq1d_off, int n, const int32_t* status, const int32_t* len1, const int32_t* len2,
                                    const int32_t* seq_len, int band_size, const int32_t* unbanded, PoPairFastqPlan* p) {
    p->n = n;
    for (int s = 0; s < 2; ++s) {
        p->off1d[s].assign((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) p->off1d[s][i] = seq1d_off[2 * (size_t)i + s];
        p->off1d[s][n] = seq1d_off[2 * (size_t)n];
    }
    p->cons_off.assign((size_t)n + 1, 0);
    for (int k = 0; k < PO_PQ_ITEMS; ++k) {
        p->len[k].assign(n, 0); p->cls[k].assign(n, PO_PQ_NONE); p->len_b[k].assign(n, 0);
        p->off_b[k].assign((size_t)n + 1, 0); p->off_u[k].assign((size_t)n + 1, 0);
        p->pos[k].assign(n, 0); p->sel[k].assign(n, 0);
        for (int i = 0; i < n; ++i) {
            const int32_t raw = k == 0 ? len1[i] : k == 1 ? len2[i] : seq_len[i];
            const int32_t L = (status[i] == 0 && raw > 0) ? raw : 0;
            const bool flagged = band_size <= 0 || (unbanded && unbanded[4 * (size_t)i + k] != 0);
            const int c = L == 0 ? PO_PQ_NONE : flagged ? PO_PQ_UNBANDED : PO_PQ_BANDED;
            p->len[k][i] = L;
            p->cls[k][i] = c;
            p->len_b[k][i] = c == PO_PQ_BANDED ? L : 0;
            p->off_b[k][(size_t)i + 1] = p->off_b[k][i] + (c == PO_PQ_BANDED ? L : 0);
            p->off_u[k][(size_t)i + 1] = p->off_u[k][i] + (c == PO_PQ_UNBANDED ? L : 0);
        }
        p->total_b[k] = p->off_b[k][n];
        p->total_u[k] = p->off_u[k][n];
        for (int i = 0; i < n; ++i) {
            const bool u = p->cls[k][i] == PO_PQ_UNBANDED;
            p->pos[k][i] = u ? p->total_b[k] + p->off_u[k][i] : p->off_b[k][i];
            p->sel[k][i] = u ? n + i : i;
        }
    }
    for (int i = 0; i < n; ++i) p->cons_off[(size_t)i + 1] = p->cons_off[i] + p->len[2][i];
}

// the status of item (k, i) after both calls: st = [banded call's n | unbanded call's n]; an empty item has 0
inline int32_t po_pair_fastq_status(const PoPairFastqPlan& p, int k, int i, const int32_t* st) {
    return p.cls[k][i] == PO_PQ_NONE ? 0 : st[p.sel[k][i]];
}

// the block of item type k in the guide output: the four types' guides one behind the other, each with the rows of its side
inline int64_t po_pair_fastq_guide_base(int k, int64_t rows1, int64_t rows2) {
    return k == 0 ? 0 : k == 1 ? rows1 : k == 2 ? rows1 + rows2 : 2 * rows1 + rows2;
}
