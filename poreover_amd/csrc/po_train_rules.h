// How `train` cuts the M = n·T rows of a weight-gradient reduction into splits, once.  Every split's
// partial sum goes to its own slice of the trainer's partial buffer and combine_kernel adds the slices in split order, so
// the cut is part of a step's bits: it depends on M alone.  No HIP in this file: tools/train_split_check.cpp compiles it
// alone under sanitizers.
//   f32 kernels (wgrad_kernel, colsum_kernel)   align = 4: the rows of one v_mfma_f32_16x16x4_f32
//   bf16 kernel (wgrad_bf16_kernel)             align = 32: the rows of one v_mfma_f32_16x16x32_bf16, so that a split
//                                               boundary never falls inside an MFMA's k block
#pragma once
#include <cstdint>

constexpr int PO_TRAIN_WG_ROWS = 1024;    // rows per split while that gives at most PO_TRAIN_MAX_SPLIT splits
constexpr int PO_TRAIN_MAX_SPLIT = 64;
constexpr int PO_TRAIN_BF16_ALIGN = 32;

// rows per split: M over the number of splits aimed for, rounded up to a multiple of `align`
inline int64_t po_train_split_rows(int64_t M, int align) {
    int64_t nz = (M + PO_TRAIN_WG_ROWS - 1) / PO_TRAIN_WG_ROWS;
    if (nz < 1) nz = 1;
    if (nz > PO_TRAIN_MAX_SPLIT) nz = PO_TRAIN_MAX_SPLIT;
    return ((M + nz - 1) / nz + align - 1) / align * align;
}

// the splits that hold a row: split z is rows [z·rows, min((z + 1)·rows, M))
inline int po_train_split_count(int64_t M, int64_t rows) { return (int)((M + rows - 1) / rows); }

// floats of partial buffer a K x N result needs
inline int64_t po_train_part_floats(int64_t M, int64_t rows, int64_t K, int64_t N) {
    return (int64_t)po_train_split_count(M, rows) * K * N;
}
