// Rules of po_ctc.hip that the host and the device share: the launch classes by lattice width S = 2L + 1, the LDS a class
// takes, and the label length the LDS form holds.  No HIP here: the host reads them to plan, the kernel to index.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/poreover_hip.h"

#ifdef __HIPCC__
#define PO_CTC_HD __host__ __device__
#else
#define PO_CTC_HD
#endif

// The longest label of po_ctc_loss: S = 2401 states, two rows of doubles, the state codes and the reduction slots in 48 KiB.
// (PO_CTC_MAX_LABEL is include/poreover_hip.h's)
constexpr int PO_CTC_MAX_STATES = 2 * PO_CTC_MAX_LABEL + 1;

// class c takes the items with PO_CTC_CLASS_HI[c - 1] < S <= PO_CTC_CLASS_HI[c] (class 0: from S = 1):
// (threads, states per thread) = (64, 2), (256, 2), (256, 10)
constexpr int PO_CTC_NCLASS = 3;
constexpr int PO_CTC_CLASS_HI[PO_CTC_NCLASS] = {128, 512, PO_CTC_MAX_STATES};
constexpr int PO_CTC_CLASS_THREADS[PO_CTC_NCLASS] = {64, 256, 256};
constexpr int PO_CTC_CLASS_PER[PO_CTC_NCLASS] = {2, 2, 10};
static_assert(PO_CTC_CLASS_THREADS[0] * PO_CTC_CLASS_PER[0] >= PO_CTC_CLASS_HI[0], "class 0 holds its states");
static_assert(PO_CTC_CLASS_THREADS[1] * PO_CTC_CLASS_PER[1] >= PO_CTC_CLASS_HI[1], "class 1 holds its states");
static_assert(PO_CTC_CLASS_THREADS[2] * PO_CTC_CLASS_PER[2] >= PO_CTC_CLASS_HI[2], "class 2 holds its states");

// A lattice row in LDS: two -inf cells below state 0 and two above state S - 1, so that s - 2 .. s + 2 need no bounds test.
PO_CTC_HD inline int po_ctc_row_stride(int S) { return (S + 4 + 1) & ~1; }
// dynamic LDS of a workgroup whose widest item has S states: two rows | the reduction slots (2 buffers x 4 waves x 8
// classes) | one code byte per state; every part a multiple of 16 bytes
PO_CTC_HD inline size_t po_ctc_lds_bytes(int S) {
    return (size_t)2 * po_ctc_row_stride(S) * 8 + (size_t)2 * 4 * 8 * 8 + (((size_t)S + 15) & ~(size_t)15);
}
static_assert(2 * ((PO_CTC_MAX_STATES + 5) & ~1) * 8 + 512 + ((PO_CTC_MAX_STATES + 15) & ~15) <= 48 * 1024, "the widest class fits 48 KiB");

// the frames a label needs at least: one per symbol, and in merge mode one blank between equal neighbours
PO_CTC_HD inline int64_t po_ctc_min_frames(int64_t L, int64_t adjacent_equal, int merge) { return L + (merge ? adjacent_equal : 0); }
