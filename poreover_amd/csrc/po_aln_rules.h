// The per-element rules of tensors.edit_alignment, once: which predecessors achieve a cell of po_acc_rules.h's
// key table, the op a cell's walk takes, the packing of the ops of a row into trace words, the block of trace words a wave
// holds while it walks back, the step of the walk, and the confusion cell of an op.  The kernels of po_aln.hip and the host
// use the same functions.  No HIP in this file: tools/aln_check.cpp compiles it alone under sanitizers and holds it against
// the full table and the walk written naively.  po_acc_rules.h is used as it is; nothing of it is restated or changed.
//   ops      hypothesis a (la symbols) against truth b (lb symbols): '=' 0 and 'X' 1 consume one symbol of each, 'I' 2 a
//            hypothesis symbol the truth lacks, 'D' 3 a truth symbol the hypothesis lacks.  The walk from (la, lb) to (0, 0)
//            takes at each cell the first predecessor that achieves the cell's key: the diagonal, then the hypothesis step
//            (I), then the truth step (D).  Every predecessor that achieves equality lies on an optimal path, so the ops have
//            exactly m codes 0 and m + d columns.
//   wave     the kernel puts the SHORTER string on the lanes (columns j) and the longer on the rows i, as edit_stats_kernel
//            does.  cols_hyp says that the columns are the hypothesis (la <= lb): then a step to the left is I and a step up
//            is D, else a step up is I and a step to the left is D.  The trace holds each cell's direction in the kernel's
//            orientation (diagonal on equal symbols, diagonal on unequal ones, up, left), chosen by the item's rule: the
//            diagonal first, then whichever of left and up is the hypothesis step.  The walk turns directions into ops.
//   achieve  in po_acc_row_local write t'_k = t_k - 4096 j and run_{k-1} for the running minimum before column k.  If
//            t'_k > run_{k-1} the cell is "left" whatever the other lanes bring.  Otherwise run_k == t'_k, which row[k] holds
//            until the finish: there the diagonal or up achieve the cell iff row[k] <= excl, and left achieves it iff
//            min(run_{k-1}, excl) <= row[k].  So the local pass keeps two bits a column, the direction as far as
//            the lane knows it, and no second copy of the row; both passes compare a candidate with a left term (below, at,
//            above) per column and settle 16 columns at once with a few word operations (po_aln_merge).
//   trace    2 bits a cell, rows 1 .. L (row 0 and column 0 need none: the walk moves along them by rule).  U = min(K, 16)
//            columns and R = 16 / U rows share a word: K >= 16 gives a lane K / 16 words a row, stored at once; K < 16 gives it
//            one word every R rows.  word(i, j) = ((i - 1) / R) * (64 K / U) + j / U, bit 2 * (((i - 1) % R) * U + j % U).
//   block    the walk's 64 lanes hold two adjacent words each: lane r serves group (i0 - 1) / R - r / R of R rows with the
//            words window(g) + 2 (r % R) and the next, a window of 32 columns around the column the walk would reach there
//            along the diagonal.  A cell outside the block re-fetches the block from that cell, which then lies inside.
#pragma once
#include "po_acc_rules.h"

#define PO_ALN_EQ 0
#define PO_ALN_X 1
#define PO_ALN_I 2
#define PO_ALN_D 3
#define PO_ALN_GAP 4                // the row / column of a gap in the confusion table
#define PO_ALN_SIDE 5
#define PO_ALN_CELLS (PO_ALN_SIDE * PO_ALN_SIDE)

static_assert(PO_EV_WAVE == 64 && PO_EV_MAX_SLOTS == 64, "the trace's geometry");

// ---- what the trace holds: the cell's direction in the kernel's orientation
#define PO_ALN_DIR_EQ 0u            // the diagonal, equal symbols
#define PO_ALN_DIR_X 1u             // the diagonal, unequal symbols
#define PO_ALN_DIR_UP 2u            // a symbol of the longer string (the rows)
#define PO_ALN_DIR_LEFT 3u          // a symbol of the shorter string (the lanes' columns)
#define PO_ALN_ODD 0x55555555u      // bit 0 of every column of a word
// A word of directions or comparisons is pinned after each column's share has gone into it: left to itself the device
// compiler holds all 64 columns' comparisons back until the words are put together, in scalar registers that it then
// spills and reads back inside the row loop.
#if defined(__HIP_DEVICE_COMPILE__)
#define PO_ALN_PIN(word) asm volatile("" : "+v"(word))
#else
#define PO_ALN_PIN(word) ((void)0)
#endif

// the op of a direction, and the step it takes
PO_EV_HD inline uint32_t po_aln_op(uint32_t dir, bool cols_hyp) {
    if (dir <= PO_ALN_DIR_X) return dir;
    return (dir == PO_ALN_DIR_LEFT) == cols_hyp ? PO_ALN_I : PO_ALN_D;     // the columns' symbol is a hypothesis symbol or not
}
PO_EV_HD inline void po_aln_step(uint32_t dir, int* i, int* j) {
    if (dir != PO_ALN_DIR_LEFT) --*i;
    if (dir != PO_ALN_DIR_UP) --*j;
}

// -1, 0, 1 for v below, at, above w (no difference of two values of the table overflows)
PO_EV_HD inline int32_t po_aln_cmp3(int32_t v, int32_t w) {
    const int32_t d = v - w;
    return d < -1 ? -1 : d > 1 ? 1 : d;
}
// 16 columns at once.  dirs: the direction that achieves the candidate t of each column; cmp: the candidate against a term
// that reaches the cell from the left, a digit a column (0 below, 1 at, 2 above).  Above: the cell is the left term's, LEFT.
// At: both achieve the cell, and LEFT takes it from UP where the columns are the hypothesis (tie_left all ones, else 0):
// the diagonal goes first either way, then the hypothesis step.
PO_EV_HD inline uint32_t po_aln_merge(uint32_t dirs, uint32_t cmp, uint32_t tie_left) {
    const uint32_t above = cmp & ~PO_ALN_ODD;
    return dirs | above | (above >> 1) | (cmp & (dirs >> 1) & PO_ALN_ODD & tie_left);
}

// ---- trace geometry of instantiation K (a power of two, 1 .. 64)
struct po_aln_geom {
    int ush, rsh;       // log2 of U = min(K, 16) columns a word and of R = 16 / U rows a word
    int gw;             // words of a group of R rows: 64 K / U
};
PO_EV_HD inline po_aln_geom po_aln_geometry(int K) {
    po_aln_geom g;
    g.ush = 0;
    while ((1 << g.ush) < K && g.ush < 4) ++g.ush;
    g.rsh = 4 - g.ush;
    g.gw = K < 16 ? PO_EV_WAVE : 4 * K;
    return g;
}
PO_EV_HD inline int64_t po_aln_words(int K, int64_t L) {
    const po_aln_geom g = po_aln_geometry(K);
    return ((L + (1 << g.rsh) - 1) >> g.rsh) * g.gw;
}
// the words of the trace of la against lb symbols; lengths past po_edit_stats' caps count as the caps, so the function is
// non-decreasing in both arguments and a bound on the lengths bounds the room of every pair that is answered
PO_EV_HD inline int64_t po_aln_trace_words(int64_t la, int64_t lb) {
    int64_t S = la <= lb ? la : lb, L = la <= lb ? lb : la;
    if (S < 0) return 0;
    if (S > PO_EDIT_MAX_SHORT) S = PO_EDIT_MAX_SHORT;
    if (L > PO_ACC_MAX_LONG) L = PO_ACC_MAX_LONG;
    return po_aln_words(po_ev_slot_class(po_ev_slots((int)S)), L);
}
PO_EV_HD inline int64_t po_aln_word(const po_aln_geom& g, int i, int j) { return (int64_t)((i - 1) >> g.rsh) * g.gw + (j >> g.ush); }
PO_EV_HD inline int po_aln_bit(const po_aln_geom& g, int i, int j) {
    return 2 * ((((i - 1) & ((1 << g.rsh) - 1)) << g.ush) + (j & ((1 << g.ush) - 1)));
}

// ---- forward.  po_acc_row_local with the directions: the values of row[] and the return are po_acc_row_local's.  st[] takes
// each column's direction as far as the lane alone knows it (the left term is the running minimum before the column).
template <int K>
PO_EV_HD inline int32_t po_aln_row_local(int32_t (&row)[K], uint32_t (&st)[(K + 15) / 16], const uint32_t (&sym)[(K + 3) / 4],
                                         int32_t diag, int x, int32_t i, uint32_t tie_left, int lane) {
    uint32_t cmp[(K + 15) / 16];
    PO_EV_UNROLL
    for (int q = 0; q < (K + 15) / 16; ++q) st[q] = 0, cmp[q] = PO_ALN_ODD;
    // every column's t' = t - 4096 j and the direction that achieves t: nothing here waits for a neighbour
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) {
        const int j = lane * K + k;
        const int32_t up = row[k];
        const int c = (int)((sym[k >> 2] >> (8 * (k & 3))) & 0xffu);
        const int32_t neq = c != x ? 1 : 0;
        const int32_t tu = up + PO_ACC_BASE, td = diag + neq * (PO_ACC_BASE + 1) - 1;
        const bool col0 = k == 0 && lane == 0;   // j == 0: D[i][0] = 4096 i, and only up achieves it
        const int32_t t = col0 ? i * PO_ACC_BASE : po_ev_min(tu, td);
        const uint32_t dir = col0 || tu < td ? PO_ALN_DIR_UP : (uint32_t)neq;
        diag = up;
        row[k] = t - j * PO_ACC_BASE;
        st[k >> 4] |= dir << (2 * (k & 15));
        PO_ALN_PIN(st[k >> 4]);
    }
    // the running minimum, and each t' against the minimum before it
    int32_t run = PO_EV_INF;
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) {
        const int32_t tp = row[k];
        cmp[k >> 4] += (uint32_t)po_aln_cmp3(tp, run) << (2 * (k & 15));
        PO_ALN_PIN(cmp[k >> 4]);
        run = po_ev_min(run, tp);
        row[k] = run;
    }
    PO_EV_UNROLL
    for (int q = 0; q < (K + 15) / 16; ++q) st[q] = po_aln_merge(st[q], cmp[q], tie_left);
    return run;
}

// po_acc_row_finish with the directions: row[] and the return are po_acc_row_finish's; code[] takes the final direction of each
// of the lane's columns (column k in bits 2 (k % 16) of word k / 16; K < 16: the bits above 2 K are no column's)
template <int K>
PO_EV_HD inline int32_t po_aln_row_finish(int32_t (&row)[K], uint32_t (&code)[(K + 15) / 16], const uint32_t (&st)[(K + 15) / 16],
                                          int32_t excl, uint32_t tie_left, int lane) {
    uint32_t cmp[(K + 15) / 16];
    PO_EV_UNROLL
    for (int q = 0; q < (K + 15) / 16; ++q) cmp[q] = PO_ALN_ODD;
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) {
        const int32_t r = row[k];
        cmp[k >> 4] += (uint32_t)po_aln_cmp3(r, excl) << (2 * (k & 15));
        PO_ALN_PIN(cmp[k >> 4]);
        row[k] = po_ev_min(r, excl) + (lane * K + k) * PO_ACC_BASE;
    }
    PO_EV_UNROLL
    for (int q = 0; q < (K + 15) / 16; ++q) code[q] = po_aln_merge(st[q], cmp[q], tie_left);
    return excl + (lane * K - 1) * PO_ACC_BASE;
}

// ---- the walk's block.  Anchored at the cell (i0, j0), i0 >= 1: relative group g = 0 .. 64 / R - 1
PO_EV_HD inline int po_aln_window(const po_aln_geom& g, int i0, int j0, int rel) {
    const int R = 1 << g.rsh;
    const int G = ((i0 - 1) >> g.rsh) - rel;
    const int top = i0 < (G + 1) * R ? i0 : (G + 1) * R;          // the first row of the group that the walk can reach
    const int e = j0 - (i0 - top) - 8 - (R - 1) / 2;               // 32 columns around the diagonal through (i0, j0)
    const int cw = e > 0 ? e >> g.ush : 0, last = g.gw - 2 * R;
    return cw < last ? cw : last;
}
// the first of the two adjacent words lane `lane` holds, or -1 where its group lies above row 1
PO_EV_HD inline int64_t po_aln_block_word(const po_aln_geom& g, int i0, int j0, int lane) {
    const int rel = lane >> g.rsh, sub = lane & ((1 << g.rsh) - 1);
    const int G = ((i0 - 1) >> g.rsh) - rel;
    if (G < 0) return -1;
    return (int64_t)G * g.gw + po_aln_window(g, i0, j0, rel) + 2 * sub;
}
// where the block anchored at (i0, j0) holds cell (i, j), 1 <= i <= i0: the lane, which of its two words, the bit; false
// where the block does not hold it
PO_EV_HD inline bool po_aln_block_find(const po_aln_geom& g, int i0, int j0, int i, int j, int* lane, int* which, int* bit) {
    const int rel = ((i0 - 1) >> g.rsh) - ((i - 1) >> g.rsh);
    if (rel < 0 || rel >= (PO_EV_WAVE >> g.rsh)) return false;
    const int cw = (j >> g.ush) - po_aln_window(g, i0, j0, rel);
    if (cw < 0 || cw >= (2 << g.rsh)) return false;
    *lane = (rel << g.rsh) + (cw >> 1);
    *which = cw & 1;
    *bit = po_aln_bit(g, i, j);
    return true;
}

// ---- confusion: the cell r * 5 + h (r the truth code or 4 for a gap, h the hypothesis code or 4) of an op that consumes
// hypothesis byte a and / or truth byte b; -1 where a consumed byte is above 3
PO_EV_HD inline int po_aln_cell(uint32_t code, int a, int b) {
    const bool ua = code != PO_ALN_D, ub = code != PO_ALN_I;
    if ((ua && a > 3) || (ub && b > 3)) return -1;
    return (ub ? b : PO_ALN_GAP) * PO_ALN_SIDE + (ua ? a : PO_ALN_GAP);
}
