// The rules of data-parallel training, once: who owns which part of the gradient in the all-reduce between
// the replicas of a po_train_group, and in which order the replicas' accumulators are summed.  po_train_group.hip's kernels
// and its host code use the same functions.  No HIP in this file: tools/train_dp_check.cpp compiles it alone under
// sanitizers.
//   partition  An n-element vector is nvec = n / 4 whole 16-byte groups and a tail of n % 4 elements.  Replica r of R owns
//              slice r: the groups [po_dp_slice_begin(nvec, R, r), po_dp_slice_begin(nvec, R, r + 1)), nvec / R groups each
//              and one more in the first nvec % R slices; the tail belongs to the last slice.  A function of (n, R) alone.
//   sum        ga[e] = ((x_0[e] + x_1[e]) + x_2[e]) + ... over the contributing replicas in ascending order, plain f32
//              additions: no fmaf, no atomics, no order that depends on timing.  A replica that contributes nothing is
//              skipped, not added as zero (-0.0 + 0.0 would be +0.0).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define PO_DP_HD __host__ __device__
#else
#define PO_DP_HD
#endif

constexpr int PO_DP_MAX_REPLICAS = 16;      // the kernels take the replicas' pointers by value

// the first 16-byte group of slice r (r = R: nvec)
PO_DP_HD inline int64_t po_dp_slice_begin(int64_t nvec, int R, int r) {
    const int64_t q = nvec / R, rem = nvec % R;
    return q * r + (r < rem ? r : rem);
}

// the slice that holds 16-byte group i < nvec
PO_DP_HD inline int po_dp_slice_of(int64_t nvec, int R, int64_t i) {
    const int64_t q = nvec / R, rem = nvec % R;
    if (i < rem * (q + 1)) return (int)(i / (q + 1));
    return (int)(rem + (i - rem * (q + 1)) / q);      // (q > 0 here: with q = 0 every group is below rem)
}

// the elements [*e0, *e1) of slice r: its groups, and the tail in the last slice
PO_DP_HD inline void po_dp_slice_elems(int64_t n, int R, int r, int64_t* e0, int64_t* e1) {
    const int64_t nvec = n / 4;
    *e0 = 4 * po_dp_slice_begin(nvec, R, r);
    *e1 = r == R - 1 ? n : 4 * po_dp_slice_begin(nvec, R, r + 1);
}

// the sum's step: the running sum plus the next contributing replica's value (-ffp-contract=off: an addition stays one)
PO_DP_HD inline float po_dp_add(float acc, float x) { return acc + x; }
