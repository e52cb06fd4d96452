// The split rule of `train`'s weight-gradient reductions (poreover_amd/csrc/po_train_rules.h), the part of
// `--gemm_precision bf16` that needs no device: the same source po_train.hip runs.  Plain C++, no HIP: built and run under
// -fsanitize=address,undefined by tests/test_train_bf16_cpu.py.  Exit status 0 and "ok" when every case holds.
//
// For M = 1 .. 5000 and M = 64 · 1024 - 33 .. 64 · 1024 + 33, and for both alignments (4: the f32 kernels; 32: the bf16
// kernel): the splits [z · rows, min((z + 1) · rows, M)) cover [0, M) exactly once (every row is marked in a heap array of
// exactly M entries), none is empty, every split start is a multiple of the alignment, there are at most PO_TRAIN_MAX_SPLIT
// of them, and the partial buffer a K x N result needs stays within PO_TRAIN_MAX_SPLIT · K · N floats, the bound the trainer
// allocates by.  For alignment 4 the rule is also held against the expression po_train.hip used before this header.
#include "../poreover_amd/csrc/po_train_rules.h"

#include <algorithm>
#include <cstdio>
#include <vector>

static int failures = 0;
static long checked = 0;

static void fail(const char* what, long M, long align, long a = 0, long b = 0) {
    if (failures < 20) std::printf("FAILED %s (M %ld, align %ld: %ld, %ld)\n", what, M, align, a, b);
    ++failures;
}

static void check(int64_t M, int align) {
    ++checked;
    const int64_t rows = po_train_split_rows(M, align);
    const int nz = po_train_split_count(M, rows);
    if (rows < 1 || rows % align != 0) fail("rows per split", M, align, rows);
    if (nz < 1 || nz > PO_TRAIN_MAX_SPLIT) fail("split count", M, align, nz);
    std::vector<unsigned char> seen((size_t)M, 0);
    for (int z = 0; z < nz; ++z) {
        const int64_t beg = (int64_t)z * rows, end = std::min<int64_t>(beg + rows, M);
        if (beg % align != 0) fail("split start", M, align, z, beg);
        if (beg >= end) fail("empty split", M, align, z, beg);
        for (int64_t m = beg; m < end; ++m) ++seen[(size_t)m];
    }
    for (int64_t m = 0; m < M; ++m)
        if (seen[(size_t)m] != 1) { fail("coverage", M, align, m, seen[(size_t)m]); break; }
    if ((int64_t)nz * rows < M) fail("rows left over", M, align, nz, rows);
    for (int64_t K : {1, 24, 128, 256})
        if (po_train_part_floats(M, rows, K, 384) > (int64_t)PO_TRAIN_MAX_SPLIT * K * 384) fail("partial buffer bound", M, align, K);
    if (align == 4) {
        const int64_t z0 = std::min<int64_t>(PO_TRAIN_MAX_SPLIT, std::max<int64_t>(1, (M + PO_TRAIN_WG_ROWS - 1) / PO_TRAIN_WG_ROWS));
        if (rows != ((M + z0 - 1) / z0 + 3) / 4 * 4) fail("the f32 rule changed", M, align, rows);
    }
}

int main() {
    for (int align : {4, PO_TRAIN_BF16_ALIGN}) {
        for (int64_t M = 1; M <= 5000; ++M) check(M, align);
        for (int64_t M = 64 * 1024 - 33; M <= 64 * 1024 + 33; ++M) check(M, align);
        check(512000, align);
    }
    // the shapes the device tests name: two splits with a tail, three splits with a tail that is no multiple of 32
    if (po_train_split_rows(1080, 32) != 544 || po_train_split_count(1080, 544) != 2) fail("M = 1080", 1080, 32);
    if (po_train_split_rows(2100, 32) != 704 || po_train_split_count(2100, 704) != 3) fail("M = 2100", 2100, 32);
    if (po_train_split_count(680, po_train_split_rows(680, 32)) != 1) fail("M = 680", 680, 32);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok (%ld cases)\n", checked);
    return 0;
}
