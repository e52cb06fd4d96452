// The per-frame arithmetic of the trace ingest, once: ingest_kernel (po_ingest.hip, mode PO_INGEST_LOGITS_F32) and
// pair_table_kernel (po_pair_basecall.hip) call the same function, so a frame's log-probabilities are the same bits
// whichever kernel made them.
#pragma once
#include <hip/hip_runtime.h>

// v[c] = (double)(x[c] - logsumexp(x)) for the C <= 8 float32 logits of one frame, in float32 like the reference
// (decode.py:34-39) and only then widened (transducer.py:16).
// scipy.special.logsumexp as shipped in this image (1.15.3, _logsumexp.py): the maximal elements leave
// the sum (cnt of them), s = sum of exp(x - max) over the others in numpy's order (fewer than 8 elements are added
// sequentially, exactly 8 as ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)): the eight accumulators of numpy's pairwise
// sum; the maximal ones contribute exp(-inf) = +0), lse = log1p(s / cnt) + log(cnt) + max
__device__ __forceinline__ void po_ingest_log_softmax_f32(const float* x, int C, double* v) {
    float xv[8], ev[8], m = x[0];
    for (int c = 0; c < C; ++c) { xv[c] = x[c]; m = fmaxf(m, xv[c]); }
    const float shift = isfinite(m) ? m : 0.f;
    float sum = 0.f, cnt = 0.f;
    for (int c = 0; c < C; ++c) {
        const bool top = (xv[c] == m);
        if (top) cnt += 1.f;
        ev[c] = top ? 0.f : expf(xv[c] - shift);
    }
    if (C == 8) sum = ((ev[0] + ev[1]) + (ev[2] + ev[3])) + ((ev[4] + ev[5]) + (ev[6] + ev[7]));
    else for (int c = 0; c < C; ++c) sum += ev[c];
    if (sum != 0.f) sum = sum / cnt;
    const float lse = (log1pf(sum) + logf(cnt)) + m;
    for (int c = 0; c < C; ++c) v[c] = (double)(xv[c] - lse);
}
