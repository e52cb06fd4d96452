// pair-decode --skip_matches, once: the anchors and boxes of pair_decode.py:53-89,412-467 as a rule on
// integers, used by the kernels of po_skip.hip and by tools/skip_check.cpp, which compiles this file alone (no HIP) under
// sanitizers.  poreover_amd/decoding/pair_decode.get_anchors and tests/_skip_oracle.py state the same rule in Python.
//
// Column state of a 2-row alignment: mat when a1 == a2, else ins when a1 == '-', else del when a2 == '-', else mis.
// A run is a maximal stretch of equal non-mis states; a mis column ends any run and never starts one (every mis column is
// a run of its own that is never reported).  A run is reported - it is an ANCHOR (cs, ce, type), columns [cs, ce) - only
// when a later column ends it (the run open at the last column is not), and when it has at least `matches` columns (mat)
// or `indels` columns (ins / del).
//
// a2s[r][c] = number of non-gap characters of row r in columns 0..c inclusive (pair_decode.py:403-410).  With the frame
// maps map1 / map2 (frame of every base), U / V frames and anchors 0..na-1:
//   position of anchor k   map1[a2s[0][cs_k]]         text: columns [cs, ce) of row 2 for ins, of row 1 otherwise
//   box 0                  (0, map1[a2s[0][cs_0]], 0, map2[a2s[1][cs_0]])
//   box k                  (map1[a2s[0][ce_{k-1}]], map1[a2s[0][cs_k]], map2[a2s[1][ce_{k-1}]], map2[a2s[1][cs_k]])
//   box na                 (map1[a2s[0][ce_{na-1}]], U, map2[a2s[1][ce_{na-1}]], V)
// Only b0 / b1 (read 1's frames) select rows: read 2's range is lo = env[b0][0], hi = env[b1 - 1][1], and the box's
// envelope is env[b0:b1] - lo.  Where the reference raises, the pair gets a status and its neighbours are unaffected:
//   no anchor                              PO_E_NO_ANCHOR   (the reference's assert)
//   a map index equal to the basecall's length (a2s counts INCLUSIVE, so the column after the last base of a read
//   indexes one past its map), or b1 <= b0   PO_E_BOX         (the reference's IndexError)
//
// Join order.  The reference joins sorted(boxes + anchors), tuples (position, string) with a box at its b0.  With strictly
// increasing frame maps (the engine's own Viterbi maps) and no empty box the positions of box 0, anchor 0, box 1, ...,
// anchor na-1, box na never decrease, and the sorted order is that interleaved order but for one tie:
//   * box k before anchor k: box k is (b0, b1 = position of anchor k) and is not empty, so b0 < b1.
//   * anchor k before box k + 1: their positions are map1[a2s[0][cs_k]] and map1[a2s[0][ce_k]], and a2s[0][ce_k] -
//     a2s[0][cs_k] is the number of bases of read 1 in columns cs_k + 1 .. ce_k.  After an ins run the column that ends it
//     is not ins (it would continue the run), so it carries a base of read 1: the difference is 1.  A mat or del run of L
//     columns carries a base of read 1 in every column, and so does the column that ends it unless that is an ins column:
//     the difference is at least L - 1, and positive for L >= 2.
//   * the tie: a ONE-column mat / del anchor (matches == 1 or indels == 1) ended by an ins column has box k + 1 at its own
//     position p.  Box k + 1 is not empty, so everything after it lies beyond p, and sorted() orders the two by their
//     strings: the stitch kernel compares the anchor's text with the box's consensus there (po_skip_text_less).
// The test oracle keeps Python's sorted(), so a flaw in this argument shows up in the tests.
#pragma once
#include <cstdint>

#include "../../include/poreover_hip.h"

#ifdef __HIPCC__
#define PO_SKIP_HD __host__ __device__
#else
#define PO_SKIP_HD
#endif

constexpr int PO_SKIP_MAT = 0, PO_SKIP_INS = 1, PO_SKIP_DEL = 2, PO_SKIP_MIS = 3, PO_SKIP_START = -1;

struct PoSkipAnchor { int32_t cs, ce, type, pos; };   // a row of the anchor table
struct PoSkipBox { int32_t b0, b1, lo, hi; };         // a row of the box table

PO_SKIP_HD inline int po_skip_state(char a1, char a2) {
    return a1 == a2 ? PO_SKIP_MAT : (a1 == '-' ? PO_SKIP_INS : (a2 == '-' ? PO_SKIP_DEL : PO_SKIP_MIS));
}
// column k starts a run (column 0: prev = PO_SKIP_START)
PO_SKIP_HD inline bool po_skip_starts(int state, int prev) { return state != prev || state == PO_SKIP_MIS; }
// a closed run of `len` columns of state `type` is an anchor
PO_SKIP_HD inline bool po_skip_reported(int type, int len, int matches, int indels) {
    if (type == PO_SKIP_MAT) return len >= matches;
    if (type == PO_SKIP_INS || type == PO_SKIP_DEL) return len >= indels;
    return false;
}

// rows of the anchor table before pair i's, for tables of alignment capacities aln_off (pair i may have aln_off[i + 1] -
// aln_off[i] columns at most): a pair of c columns has at most c / min(matches, indels) anchors and one box more, and
// floor((x + c) / m) - floor(x / m) >= floor(c / m), so the table needs no prefix sum.  Pair i's boxes start at row
// po_skip_table_row(..) + i of the box table.
PO_SKIP_HD inline int64_t po_skip_table_row(int64_t aln_off_i, int64_t aln_off_0, int i, int matches, int indels) {
    const int m = matches < indels ? matches : indels;
    return (aln_off_i - aln_off_0) / (m > 0 ? m : 1) + i;
}

// ---- the wave form: 64 columns at a time on 64-bit ballots.  S: the columns that start a run, G0 / G1: the columns whose
// row 1 / row 2 is no gap.  What crosses from one chunk to the next:
struct PoSkipCarry {
    int run_start;    // column at which the open run started
    int a0, a1;       // a2s[0] / a2s[1] at that column
    int prev_state;   // state of the last column seen (PO_SKIP_START before column 0)
    int base0, base1; // non-gap characters of the two rows in the columns seen
};
PO_SKIP_HD inline PoSkipCarry po_skip_carry_init() { return PoSkipCarry{0, 0, 0, PO_SKIP_START, 0, 0}; }
PO_SKIP_HD inline int po_skip_popc(uint64_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}
PO_SKIP_HD inline int po_skip_top(uint64_t x) {   // index of the highest set bit (x != 0)
#ifdef __HIP_DEVICE_COMPILE__
    return 63 - __clzll((long long)x);
#else
    return 63 - __builtin_clzll(x);
#endif
}
PO_SKIP_HD inline uint64_t po_skip_below(int lane) { return lane <= 0 ? 0ull : (lane >= 64 ? ~0ull : ((1ull << lane) - 1ull)); }

// The run that column c0 + lane closes, if that column starts one (bit `lane` of S): rep = it is an anchor, and its columns
// [cs, ce), type and the four a2s values the box rule needs.  prev_state: the state of column c0 + lane - 1 (lane 0: the
// carry's).
struct PoSkipClose { int rep, cs, ce, type, a0cs, a1cs, a0ce, a1ce; };
PO_SKIP_HD inline PoSkipClose po_skip_lane_close(int c0, int lane, uint64_t S, uint64_t G0, uint64_t G1, int prev_state,
                                                 const PoSkipCarry& cy, int matches, int indels) {
    PoSkipClose r = {0, 0, 0, prev_state, 0, 0, 0, 0};
    if (!((S >> lane) & 1ull) || prev_state == PO_SKIP_START) return r;
    const uint64_t before = S & po_skip_below(lane);
    if (before) {
        const int p = po_skip_top(before);
        r.cs = c0 + p;
        r.a0cs = cy.base0 + po_skip_popc(G0 & po_skip_below(p + 1));
        r.a1cs = cy.base1 + po_skip_popc(G1 & po_skip_below(p + 1));
    } else {
        r.cs = cy.run_start; r.a0cs = cy.a0; r.a1cs = cy.a1;
    }
    r.ce = c0 + lane;
    r.a0ce = cy.base0 + po_skip_popc(G0 & po_skip_below(lane + 1));
    r.a1ce = cy.base1 + po_skip_popc(G1 & po_skip_below(lane + 1));
    r.rep = po_skip_reported(prev_state, r.ce - r.cs, matches, indels) ? 1 : 0;
    return r;
}
// the carry after a chunk of `cnt` columns (1..64) whose last column has state `last_state`
PO_SKIP_HD inline PoSkipCarry po_skip_carry_next(int c0, int cnt, uint64_t S, uint64_t G0, uint64_t G1, int last_state,
                                                 PoSkipCarry cy) {
    const uint64_t in = po_skip_below(cnt);
    S &= in; G0 &= in; G1 &= in;
    if (S) {
        const int p = po_skip_top(S);
        cy.run_start = c0 + p;
        cy.a0 = cy.base0 + po_skip_popc(G0 & po_skip_below(p + 1));
        cy.a1 = cy.base1 + po_skip_popc(G1 & po_skip_below(p + 1));
    }
    cy.base0 += po_skip_popc(G0);
    cy.base1 += po_skip_popc(G1);
    cy.prev_state = last_state;
    return cy;
}

// ---- the box rule.  Box k of na + 1 (na >= 1) from the a2s values of anchor k - 1's end (k > 0) and anchor k's start (k < na).
// Returns PO_OK or PO_E_BOX; *pos gets box k's b1, the position of anchor k (k < na).  env: 2 ints per frame of read 1.
PO_SKIP_HD inline int po_skip_box(int k, int na, int a0ce_prev, int a1ce_prev, int a0cs, int a1cs, const int32_t* map1, int len1,
                                  const int32_t* map2, int len2, int U, int V, const int32_t* env, PoSkipBox* box, int* pos) {
    int b0 = 0, b1 = U;
    box->b0 = box->b1 = box->lo = box->hi = 0;
    *pos = 0;
    if (k > 0) {
        if (a0ce_prev >= len1 || a1ce_prev >= len2) return PO_E_BOX;
        b0 = map1[a0ce_prev];
    }
    if (k < na) {
        if (a0cs >= len1 || a1cs >= len2) return PO_E_BOX;
        b1 = map1[a0cs];
        *pos = b1;
    }
    (void)map2; (void)V;   // read 2's side of the reference's box tuple is looked up (and may raise) but selects nothing
    box->b0 = b0; box->b1 = b1;
    if (b1 <= b0 || b0 < 0 || b1 > U) return PO_E_BOX;
    box->lo = env[2 * b0];
    box->hi = env[2 * (b1 - 1) + 1];
    return PO_OK;
}

// Python's a < b for two strings of ACGT: the join order's tie (above)
PO_SKIP_HD inline bool po_skip_text_less(const char* a, int la, const char* b, int lb) {
    const int m = la < lb ? la : lb;
    for (int i = 0; i < m; ++i)
        if (a[i] != b[i]) return (unsigned char)a[i] < (unsigned char)b[i];
    return la < lb;
}

// ---- the serial statement (get_anchors as written), for the check program: returns the number of anchors, writes at most cap
inline int po_skip_anchors_serial(const char* r1, const char* r2, int ncol, int matches, int indels, PoSkipAnchor* out, int cap) {
    int n = 0, start = 0, count = 1, prev = PO_SKIP_START;
    for (int i = 0; i < ncol; ++i) {
        const int state = po_skip_state(r1[i], r2[i]);
        if (state == prev && state != PO_SKIP_MIS) { count++; continue; }
        if (prev != PO_SKIP_START && po_skip_reported(prev, count, matches, indels)) {
            if (n < cap) out[n] = PoSkipAnchor{start, i, prev, 0};
            n++;
        }
        prev = state; count = 1; start = i;
    }
    return n;
}
// ---- the wave form run on the host, lane by lane: what the anchor kernel computes, for the check program
inline int po_skip_anchors_wave(const char* r1, const char* r2, int ncol, int matches, int indels, PoSkipAnchor* out,
                                int32_t* a2s4 /* 4 per anchor: a0cs a1cs a0ce a1ce, or null */, int cap) {
    PoSkipCarry cy = po_skip_carry_init();
    int n = 0;
    for (int c0 = 0; c0 < ncol; c0 += 64) {
        const int cnt = ncol - c0 < 64 ? ncol - c0 : 64;
        int st[64];
        uint64_t S = 0, G0 = 0, G1 = 0;
        for (int l = 0; l < cnt; ++l) {
            st[l] = po_skip_state(r1[c0 + l], r2[c0 + l]);
            if (po_skip_starts(st[l], l ? st[l - 1] : cy.prev_state)) S |= 1ull << l;
            if (r1[c0 + l] != '-') G0 |= 1ull << l;
            if (r2[c0 + l] != '-') G1 |= 1ull << l;
        }
        for (int l = 0; l < cnt; ++l) {
            const PoSkipClose c = po_skip_lane_close(c0, l, S, G0, G1, l ? st[l - 1] : cy.prev_state, cy, matches, indels);
            if (!c.rep) continue;
            if (n < cap) {
                out[n] = PoSkipAnchor{c.cs, c.ce, c.type, 0};
                if (a2s4) { a2s4[4 * n] = c.a0cs; a2s4[4 * n + 1] = c.a1cs; a2s4[4 * n + 2] = c.a0ce; a2s4[4 * n + 3] = c.a1ce; }
            }
            n++;
        }
        cy = po_skip_carry_next(c0, cnt, S, G0, G1, st[cnt - 1], cy);
    }
    return n;
}
