// Rules of po_falign.hip that the host and the device share.  The launch classes, the row stride in LDS, the label limit and
// the least number of frames are po_ctc_rules.h's: the lattice is po_ctc_loss's.  Here: the trace-back's bit rows and the LDS
// of a class without the loss's reduction slots.  No HIP here.
#pragma once
#include "po_ctc_rules.h"

// A frame's decisions: one 2-bit code per state (0 stay, 1 step, 2 skip), kept as two bit planes per 64 states.  A "word" is
// the pair (low plane, high plane) of 64 states, 16 bytes; frame t of an item with S states has po_falign_row_words(S) of them.
constexpr int PO_FALIGN_WORD_BYTES = 16;
PO_CTC_HD inline int64_t po_falign_row_words(int64_t S) { return (S + 63) / 64; }

// the trace-back walks this many frames per block: their candidate words are requested together, their states written together
constexpr int PO_FALIGN_BLOCK = 64;

// dynamic LDS of a workgroup whose widest item has S states: two rows | one code byte per state
PO_CTC_HD inline size_t po_falign_lds_bytes(int S) { return (size_t)2 * po_ctc_row_stride(S) * 8 + (((size_t)S + 15) & ~(size_t)15); }
static_assert(2 * ((PO_CTC_MAX_STATES + 5) & ~1) * 8 + ((PO_CTC_MAX_STATES + 15) & ~15) <= 48 * 1024, "the widest class fits 48 KiB");
