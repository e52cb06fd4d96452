// The per-element rules of the held-out validation of `train`, once: the class of a frame, the place of
// a frame's code in its window's path, the cell of the edit distance and the way a wave of 64 lanes walks that table.  The
// kernels of po_eval.hip and the host use the same functions.  No HIP in this file: tools/eval_check.cpp compiles it alone
// under sanitizers and holds it against brute-force recursion and the plain row DP.
//   argmax   np.argmax over the 5 f32 probabilities of a frame: the first NaN if there is one, else the first maximum
//   path     train.validation_error: the frames in order, classes 0..3 kept as codes 0..3, class 4 dropped, repeats kept
//   cell     unit-cost Levenshtein on int32: D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (a[i-1] != b[j-1])),
//            D[i][0] = i, D[0][j] = j; the distance is D[la][lb] (an empty side gives the other side's length)
//   wave     one row i of the table at a time, the columns j = 0..S of the SHORTER string on the lanes: lane l holds the K
//            columns l·K .. l·K + K - 1 (K = the power of two >= ceil((S + 1) / 64)).  With t[j] = min(D[i-1][j] + 1,
//            D[i-1][j-1] + neq) and t[0] = i, the left neighbour's term unrolls to D[i][j] = j + min_{k <= j} (t[k] - k)
//            (accuracy.alignment_summary's running minimum): each lane takes the running minimum of its own columns, a
//            wave-wide exclusive prefix minimum of the lanes' totals supplies the columns to its left, and that prefix
//            plus l·K - 1 is also D[i][l·K - 1], the next row's diagonal for the lane's first column.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define PO_EV_HD __host__ __device__
#define PO_EV_UNROLL _Pragma("unroll")
#else
#define PO_EV_HD
#define PO_EV_UNROLL
#endif

#define PO_EV_CLASSES 5
#define PO_EV_BLANK 4
#define PO_EV_WAVE 64
#define PO_EDIT_MAX_SHORT 4095        // the shorter string of a pair: 64 lanes x 64 columns, column 0 included
#define PO_EV_MAX_SLOTS 64
#define PO_EV_INF 0x3fffffff          // the identity of the prefix minimum (no sum with a column index overflows)

// ---- argmax
PO_EV_HD inline int po_ev_argmax(const float* p) {
    int best = 0;
    float bv = p[0];
    for (int c = 1; c < PO_EV_CLASSES; ++c) {
        const float v = p[c];
        if (v > bv || (v != v && bv == bv)) { best = c; bv = v; }
    }
    return best;
}

// ---- path.  One frame of a block of up to 64 frames: keep has bit f set where frame f of the block is no blank, carry is
// the number of codes the window's earlier blocks kept.  Returns false for a dropped frame, else *pos = the frame's place.
PO_EV_HD inline int po_ev_popc(uint64_t x) { return __builtin_popcountll(x); }
PO_EV_HD inline bool po_ev_path_slot(uint64_t keep, int lane, int carry, int* pos) {
    const uint64_t bit = (uint64_t)1 << lane;
    if (!(keep & bit)) return false;
    *pos = carry + po_ev_popc(keep & (bit - 1));
    return true;
}

// ---- cell
PO_EV_HD inline int32_t po_ev_min(int32_t a, int32_t b) { return a < b ? a : b; }
PO_EV_HD inline int32_t po_ev_cell(int32_t up, int32_t left, int32_t diag, bool neq) {
    return po_ev_min(po_ev_min(up + 1, left + 1), diag + (neq ? 1 : 0));
}

// ---- wave.  Columns per lane for a shorter string of S symbols, and the instantiation that holds them
PO_EV_HD inline int po_ev_slots(int S) { return (S + 1 + PO_EV_WAVE - 1) / PO_EV_WAVE; }
PO_EV_HD inline int po_ev_slot_class(int slots) {
    int K = 1;
    while (K < slots) K <<= 1;
    return K;
}

// the symbol b[j - 1] of column j = lane·K + k sits in byte k of the lane's packed words (any value at j = 0 and j > S)
template <int K>
PO_EV_HD inline void po_ev_load_symbols(uint32_t (&sym)[(K + 3) / 4], const uint8_t* b, int S, int lane) {
    PO_EV_UNROLL
    for (int q = 0; q < (K + 3) / 4; ++q) sym[q] = 0;
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) {
        const int j = lane * K + k;
        const uint32_t c = (j >= 1 && j <= S) ? b[j - 1] : 0;
        sym[k >> 2] |= c << (8 * (k & 3));
    }
}

// row 0: D[0][j] = j
template <int K>
PO_EV_HD inline void po_ev_row_init(int32_t (&row)[K], int lane) {
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) row[k] = lane * K + k;
}

// Row i >= 1 for symbol x of the longer string, the lane's part.  In: row[] = D[i-1][lane·K ..], diag = D[i-1][lane·K - 1]
// (unused by lane 0).  Out: row[k] = the running minimum of t[j] - j over the lane's columns up to k; returns its last.
template <int K>
PO_EV_HD inline int32_t po_ev_row_local(int32_t (&row)[K], const uint32_t (&sym)[(K + 3) / 4], int32_t diag, int x, int32_t i,
                                        int lane) {
    int32_t run = PO_EV_INF;
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) {
        const int j = lane * K + k;
        const int32_t up = row[k];
        const int c = (int)((sym[k >> 2] >> (8 * (k & 3))) & 0xffu);
        const int32_t t = j == 0 ? i : po_ev_min(up + 1, diag + (c != x ? 1 : 0));
        diag = up;
        run = po_ev_min(run, t - j);
        row[k] = run;
    }
    return run;
}

// excl = the minimum of the totals of the lanes to the left (PO_EV_INF for lane 0): row[] becomes D[i][lane·K ..]; returns
// D[i][lane·K - 1], the lane's diagonal for row i + 1
template <int K>
PO_EV_HD inline int32_t po_ev_row_finish(int32_t (&row)[K], int32_t excl, int lane) {
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) row[k] = po_ev_min(row[k], excl) + (lane * K + k);
    return excl + lane * K - 1;
}

// D[i][S] out of the lane that holds column S (lane S / K)
template <int K>
PO_EV_HD inline int32_t po_ev_row_pick(const int32_t (&row)[K], int S) {
    int32_t v = 0;
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k)
        if (k == S % K) v = row[k];
    return v;
}

// The wave's exclusive prefix minimum as the kernel's moves make it, on an array of the 64 lanes' values (the host's
// restatement; the kernel does each step with one data-parallel move): Hillis-Steele inside each row of 16 lanes (shifts of
// 1, 2, 4, 8), lane 15 of rows 0 / 2 into every lane of rows 1 / 3, lane 31 into every lane of rows 2 and 3, then one
// lane to the right with PO_EV_INF into lane 0.
inline void po_ev_wave_excl_min(const int32_t* in, int32_t* out) {
    int32_t v[PO_EV_WAVE], u[PO_EV_WAVE];
    for (int l = 0; l < PO_EV_WAVE; ++l) v[l] = in[l];
    for (int d = 1; d < 16; d <<= 1) {
        for (int l = 0; l < PO_EV_WAVE; ++l) u[l] = (l & 15) >= d ? po_ev_min(v[l], v[l - d]) : v[l];
        for (int l = 0; l < PO_EV_WAVE; ++l) v[l] = u[l];
    }
    for (int l = 0; l < PO_EV_WAVE; ++l) u[l] = ((l >> 4) & 1) ? po_ev_min(v[l], v[(l & ~15) - 1]) : v[l];
    for (int l = 0; l < PO_EV_WAVE; ++l) v[l] = l >= 32 ? po_ev_min(u[l], u[31]) : u[l];
    out[0] = PO_EV_INF;
    for (int l = 1; l < PO_EV_WAVE; ++l) out[l] = v[l - 1];
}
