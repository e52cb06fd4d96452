// The window plan of `basecall`, once: how many windows a read is cut into, which frames of a window are
// kept, and the checks of po_basecall_batch_h's window / overlap / offset arguments.  The device kernels of po_basecall.hip
// and the host entry use the same functions.  No HIP in this file: tools/basecall_check.cpp compiles it alone under
// sanitizers and holds it against the definition (frame t belongs to window clamp(floor((t - O/2) / S), 0, n - 1)).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"

#ifdef __HIPCC__
#define PO_BC_HD __host__ __device__
#else
#define PO_BC_HD
#endif

// windows of a read of L >= 1 samples: 1 if L <= W, else 1 + ceil((L - W) / S)
PO_BC_HD inline int64_t po_basecall_windows(int64_t L, int W, int S) { return L <= W ? 1 : 1 + (L - W + S - 1) / S; }

// the output frames [lo, hi) that window j of a read's n windows supplies: interior windows keep their middle
// [jS + O/2, (j + 1)S + O/2), the first keeps from 0, the last keeps to L
PO_BC_HD inline void po_basecall_keep(int64_t j, int64_t n, int64_t L, int S, int O, int64_t* lo, int64_t* hi) {
    *lo = j == 0 ? 0 : j * S + O / 2;
    *hi = j == n - 1 ? L : (j + 1) * S + O / 2;
}

struct PoBasecallPlan {
    int stride = 0;
    int64_t rows = 0;                // samples of all reads = output frames
    int64_t windows = 0;             // windows of all reads: the global window list, read after read
    int64_t max_rows = 0;            // the longest read
    std::vector<int64_t> win_off;    // [n_reads + 1] first global window of each read
    std::vector<int32_t> win_read;   // [windows] the read a global window belongs to
};

// Checks window, overlap, the signal offsets and (where given) the sequence capacities, then fills *p.  Returns PO_OK, or
// PO_E_ARG / PO_E_CAP with *err naming the value under the name of the entry that asks.  Touches no device.
inline int po_basecall_make_plan(const int64_t* sig_off_h, int n_reads, int window, int overlap, const int64_t* seq_off_h,
                                 PoBasecallPlan* p, std::string* err, const char* entry = "po_basecall_batch_h") {
    const std::string me = std::string(entry) + ": ";
    if (window < 1) { *err = me + "window " + std::to_string(window) + " (at least 1)"; return PO_E_ARG; }
    if (overlap < 0 || overlap >= window || (overlap & 1)) {
        *err = me + "overlap " + std::to_string(overlap) + " (even, 0 <= overlap < window " + std::to_string(window) + ")";
        return PO_E_ARG;
    }
    if (sig_off_h[0] != 0) { *err = me + "sig_off[0] is " + std::to_string(sig_off_h[0]) + " (must be 0)"; return PO_E_ARG; }
    if (seq_off_h && seq_off_h[0] != 0) { *err = me + "seq_off[0] is " + std::to_string(seq_off_h[0]) + " (must be 0)"; return PO_E_ARG; }
    const int S = window - overlap;
    int64_t windows = 0, max_rows = 0;
    for (int r = 0; r < n_reads; ++r) {
        const int64_t L = sig_off_h[r + 1] - sig_off_h[r];
        if (L < 1) { *err = me + "read " + std::to_string(r) + " has " + std::to_string(L) + " samples (at least 1)"; return PO_E_ARG; }
        if (seq_off_h && seq_off_h[r + 1] - seq_off_h[r] < L) {
            *err = me + "read " + std::to_string(r) + " has " + std::to_string(L) + " samples and room for " +
                   std::to_string(seq_off_h[r + 1] - seq_off_h[r]) + " characters";
            return PO_E_CAP;
        }
        windows += po_basecall_windows(L, window, S);
        max_rows = L > max_rows ? L : max_rows;
        if (windows > INT32_MAX) { *err = me + "more than 2^31 - 1 windows"; return PO_E_ARG; }
    }
    p->stride = S;
    p->rows = sig_off_h[n_reads];
    p->windows = windows;
    p->max_rows = max_rows;
    p->win_off.assign((size_t)n_reads + 1, 0);
    p->win_read.resize((size_t)windows);
    for (int r = 0; r < n_reads; ++r) {
        const int64_t n = po_basecall_windows(sig_off_h[r + 1] - sig_off_h[r], window, S);
        for (int64_t j = 0; j < n; ++j) p->win_read[(size_t)(p->win_off[r] + j)] = r;
        p->win_off[r + 1] = p->win_off[r] + n;
    }
    return PO_OK;
}
