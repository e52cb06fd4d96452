// The per-element rules of tensors.accuracy, once: the class of a frame of raw values of four dtypes read
// through strides, the frames of a window that emit a base under either basecaller kind, the cell of the alignment that
// counts matches as well as edits, and the way a wave of 64 lanes walks that table.  The kernels of po_acc.hip and the host
// use the same functions.  No HIP in this file: tools/acc_check.cpp compiles it alone under sanitizers and holds it against an
// enumeration of every alignment, the plain lexicographic row DP and the emit rules written naively.  What po_eval_rules.h has
// already (the ballot's slot, the symbols of a lane, the pick, the prefix minimum) is used from there, not restated.
//   widen    f16 and bf16 to f32 by their bits (exact: every f16 and bf16 value is an f32 value); f64 is compared as double
//   argmax   po_ev_argmax's rule on the C = 5 raw values in canonical column order (source column perm[c] is canonical c):
//            a later value replaces the best only when it is strictly greater, or when it is NaN and the best is not
//   emit     poreover: a frame whose class is no blank emits, repeats kept; bonito: a frame emits when its class is no blank
//            and differs from the previous frame's class (frame 0 has none: prev = PO_ACC_NO_PREV).  In a block of 64 frames the
//            previous class of lane l is lane l - 1's; lane 0 takes the class carried from the last frame of the block before
//   cell     global alignment, unit costs, on the pair (d, -m) in lexicographic order: the edit distance d, and among the
//            alignments of that distance the most matches m.  The pair is additive along a path, so it packs into one int32
//            key = d * 4096 - m (m <= min(la, lb) <= 4095 < 4096): up, left and a diagonal mismatch cost +4096, a diagonal
//            match -1, and po_eval_rules.h's recurrence holds unchanged: D[i][0] = 4096 i, D[0][j] = 4096 j,
//            d = (key + 4095) >> 12, m = 4096 d - key
//   wave     po_eval_rules.h's, on the key: with t[j] = min(D[i-1][j] + 4096, D[i-1][j-1] + cost) and t[0] = 4096 i the left
//            term unrolls to D[i][j] = 4096 j + min_{k <= j} (t[k] - 4096 k)
//   bounds   a lane's columns run to 64 * 64 - 1 = 4095 whatever S is (the columns past S hold a padded string's cells, never
//            read), rows to L: every cell is at most 4096 * max(i, j) and at least -min(i, j), every t at most
//            4096 * (max(L, 4095) + 1), every t - 4096 k at least -4096 * 4095 - 4095.  PO_ACC_MAX_LONG is the largest L that
//            keeps t below PO_EV_INF, the identity of the prefix minimum; PO_EV_INF + 4096 * 4095 (the identity run through
//            po_acc_row_finish in lane 0's unused diagonal) stays an int32.
#pragma once
#include <climits>
#include <cstdint>

#include "po_eval_rules.h"

#define PO_ACC_CLASSES PO_EV_CLASSES
#define PO_ACC_BLANK PO_EV_BLANK
#define PO_ACC_NO_PREV (-1)
#define PO_ACC_SHIFT 12
#define PO_ACC_BASE (1 << PO_ACC_SHIFT)                     // 4096: one edit; a match is -1
#define PO_ACC_MAX_LONG (PO_EV_INF / PO_ACC_BASE - 1)       // 262142: the longer string of a pair
// PO_DTYPE_* and PO_KIND_* of include/poreover_hip.h (this file includes no project header but po_eval_rules.h)
#define PO_ACC_F32 0
#define PO_ACC_F16 1
#define PO_ACC_BF16 2
#define PO_ACC_F64 3
#define PO_ACC_POREOVER 0
#define PO_ACC_BONITO 1

static_assert(PO_EDIT_MAX_SHORT < PO_ACC_BASE, "the matches of a pair must fit under one edit");
static_assert(PO_EV_WAVE * PO_EV_MAX_SLOTS - 1 <= PO_EDIT_MAX_SHORT, "a lane's last column");
static_assert((int64_t)(PO_ACC_MAX_LONG + 1) * PO_ACC_BASE < (int64_t)PO_EV_INF, "a term of the last row reaches the identity");
static_assert((int64_t)(PO_EDIT_MAX_SHORT + 1) * PO_ACC_BASE < (int64_t)PO_EV_INF, "a term of the last column reaches the identity");
static_assert((int64_t)PO_EV_INF + (int64_t)PO_ACC_BASE * PO_EDIT_MAX_SHORT <= (int64_t)INT32_MAX, "the identity plus a column overflows");
static_assert(-(int64_t)PO_ACC_BASE * PO_EDIT_MAX_SHORT - PO_EDIT_MAX_SHORT - PO_ACC_BASE >= (int64_t)INT32_MIN, "t - 4096 k underflows");
static_assert(PO_ACC_MAX_LONG >= 131071, "the cap on the longer string");

// ---- widen
PO_EV_HD inline float po_acc_bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
PO_EV_HD inline float po_acc_bf16(uint16_t h) { return po_acc_bits_f32((uint32_t)h << 16); }
PO_EV_HD inline float po_acc_f16(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 31u) return po_acc_bits_f32(sign | 0x7f800000u | (m << 13));                    // infinity, NaN
    if (e != 0u) return po_acc_bits_f32(sign | ((e + 112u) << 23) | (m << 13));               // normal: bias 15 -> 127
    const float v = (float)(int)m * 5.9604644775390625e-8f;                                   // subnormal: m * 2^-24, exact
    return sign ? -v : v;
}
PO_EV_HD inline int po_acc_elem_bytes(int dtype) { return dtype == PO_ACC_F64 ? 8 : (dtype == PO_ACC_F32 ? 4 : 2); }
// one element of dtype f32 / f16 / bf16 as float
PO_EV_HD inline float po_acc_load_f32(const char* p, int dtype) {
    if (dtype == PO_ACC_F32) return *(const float*)p;
    const uint16_t h = *(const uint16_t*)p;
    return dtype == PO_ACC_F16 ? po_acc_f16(h) : po_acc_bf16(h);
}

// ---- argmax (po_ev_argmax's rule, on float or double)
template <class V>
PO_EV_HD inline int po_acc_argmax(const V* p) {
    int best = 0;
    V bv = p[0];
    PO_EV_UNROLL
    for (int c = 1; c < PO_ACC_CLASSES; ++c) {
        const V v = p[c];
        if (v > bv || (v != v && bv == bv)) { best = c; bv = v; }
    }
    return best;
}

// the class of frame t of an item: element (t, k) at base + (t * row_stride + k * col_stride) * sizeof(dtype), strides in
// elements (0 included); canonical class c reads source column perm[c]
PO_EV_HD inline int po_acc_frame_class(const void* base, int64_t row_stride, int64_t col_stride, int64_t t, int dtype, const int* perm) {
    const int eb = po_acc_elem_bytes(dtype);
    const char* p = (const char*)base + t * row_stride * eb;
    const int64_t cs = col_stride * eb;
    if (dtype == PO_ACC_F64) {
        double v[PO_ACC_CLASSES];
        PO_EV_UNROLL
        for (int c = 0; c < PO_ACC_CLASSES; ++c) v[c] = *(const double*)(p + perm[c] * cs);
        return po_acc_argmax(v);
    }
    float v[PO_ACC_CLASSES];
    PO_EV_UNROLL
    for (int c = 0; c < PO_ACC_CLASSES; ++c) v[c] = po_acc_load_f32(p + perm[c] * cs, dtype);
    return po_acc_argmax(v);
}

// ---- emit
PO_EV_HD inline bool po_acc_emit(int kind, int cls, int prev) {
    return cls != PO_ACC_BLANK && (kind == PO_ACC_POREOVER || cls != prev);
}

// ---- cell
PO_EV_HD inline int32_t po_acc_cell(int32_t up, int32_t left, int32_t diag, bool neq) {
    return po_ev_min(po_ev_min(up + PO_ACC_BASE, left + PO_ACC_BASE), diag + (neq ? PO_ACC_BASE : -1));
}
PO_EV_HD inline int32_t po_acc_distance(int32_t key) { return (key + PO_ACC_BASE - 1) >> PO_ACC_SHIFT; }
PO_EV_HD inline int32_t po_acc_matches(int32_t key) { return po_acc_distance(key) * PO_ACC_BASE - key; }

// ---- wave (po_ev_load_symbols, po_ev_row_pick, po_ev_slots and po_ev_slot_class serve as they are)
// row 0: D[0][j] = 4096 j
template <int K>
PO_EV_HD inline void po_acc_row_init(int32_t (&row)[K], int lane) {
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) row[k] = (lane * K + k) * PO_ACC_BASE;
}
// the diagonal of row 1 for the lane's first column: D[0][lane·K - 1] (unused by lane 0)
template <int K>
PO_EV_HD inline int32_t po_acc_diag_init(int lane) { return (lane * K - 1) * PO_ACC_BASE; }

// Row i >= 1 for symbol x of the longer string, the lane's part.  In: row[] = D[i-1][lane·K ..], diag = D[i-1][lane·K - 1]
// (unused by lane 0).  Out: row[k] = the running minimum of t[j] - 4096 j over the lane's columns up to k; returns its last.
template <int K>
PO_EV_HD inline int32_t po_acc_row_local(int32_t (&row)[K], const uint32_t (&sym)[(K + 3) / 4], int32_t diag, int x, int32_t i,
                                         int lane) {
    int32_t run = PO_EV_INF;
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) {
        const int j = lane * K + k;
        const int32_t up = row[k];
        const int c = (int)((sym[k >> 2] >> (8 * (k & 3))) & 0xffu);
        const int32_t t = j == 0 ? i * PO_ACC_BASE : po_ev_min(up + PO_ACC_BASE, diag + (c != x ? PO_ACC_BASE : -1));
        diag = up;
        run = po_ev_min(run, t - j * PO_ACC_BASE);
        row[k] = run;
    }
    return run;
}

// excl = the minimum of the totals of the lanes to the left (PO_EV_INF for lane 0): row[] becomes D[i][lane·K ..]; returns
// D[i][lane·K - 1], the lane's diagonal for row i + 1
template <int K>
PO_EV_HD inline int32_t po_acc_row_finish(int32_t (&row)[K], int32_t excl, int lane) {
    PO_EV_UNROLL
    for (int k = 0; k < K; ++k) row[k] = po_ev_min(row[k], excl) + (lane * K + k) * PO_ACC_BASE;
    return excl + (lane * K - 1) * PO_ACC_BASE;
}
