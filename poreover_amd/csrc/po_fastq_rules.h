// The per-element rules of `basecall --fastq`, once: the band guide of a frame, the consumed count of a
// called base, the Phred value of a base.  The kernels of po_fastq.hip and the host use the same functions.  No HIP in
// this file: tools/fastq_check.cpp compiles it alone under sanitizers and holds it against brute-force loops and, for
// Phred, against quality.phred.
//   guide     make_labeled_data.guide_from_alignment: c[t] = consumed[j(t)], j(t) the last called base with map[j] <= t, 0
//             before the first; a diagonal read gets floor((t + 1) * L / T)
//   consumed  make_labeled_data.consumed_from_columns + the clip of quality.call_guides: per called base, the scored
//             string's bases up to and including its column, at most L
//   phred     quality.phred: the alternatives' share of the odds, in log space, float64
//   pair      quality.combine and pair_decode._attach_fastq's rule for a consensus scored on two reads' tables: the
//             element-wise sum where both lattices stand, one read's odds alone where the other's is lost, Q 0 for neither
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define PO_FQ_HD __host__ __device__
#else
#define PO_FQ_HD
#endif

#define PO_FQ_QMAX 60
#define PO_FQ_GAP '-'

// how a read's guide is made (one int32 per read)
#define PO_FQ_IDENTITY 0   // the scored string is the Viterbi call: consumed[j] = j + 1
#define PO_FQ_CONSUMED 1   // consumed[] comes from an alignment of the two
#define PO_FQ_DIAGONAL 2   // no Viterbi call, an empty string or a failed alignment: the straight diagonal
#define PO_FQ_ALIGN 3      // (between the stages) the strings differ: the pair goes to the aligner

// the number of entries of the increasing map[0..n) that are <= t
PO_FQ_HD inline int po_fq_bases_upto(const int32_t* map, int n, int64_t t) {
    int lo = 0, hi = n;   // map[lo - 1] <= t < map[hi]
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)map[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// c[t] of a read of T frames whose Viterbi call has Lc bases at frames map[], scored on a string of L bases
PO_FQ_HD inline int32_t po_fq_guide(const int32_t* map, int Lc, const int32_t* consumed, int mode, int64_t t, int64_t T, int L) {
    if (mode == PO_FQ_DIAGONAL) return (int32_t)(((t + 1) * (int64_t)L) / (T > 0 ? T : 1));
    const int j = po_fq_bases_upto(map, Lc, t) - 1;
    if (j < 0) return 0;
    return (mode == PO_FQ_CONSUMED && consumed) ? consumed[j] : j + 1;
}

PO_FQ_HD inline int po_fq_popc(uint64_t x) { return __builtin_popcountll(x); }

// One column of a block of up to 64 alignment columns.  m1 / m2: bit c set where column c of row 1 / row 2 holds a base;
// carry1 / carry2: the bases of the two rows before the block.  Returns false where column `lane` of row 1 is a gap;
// otherwise *j = the called base of that column and *value = consumed[j].
PO_FQ_HD inline bool po_fq_consumed_column(uint64_t m1, uint64_t m2, int lane, int carry1, int carry2, int L, int* j, int32_t* value) {
    const uint64_t bit = (uint64_t)1 << lane;
    if (!(m1 & bit)) return false;
    const uint64_t below = bit - 1;
    *j = carry1 + po_fq_popc(m1 & below);
    const int c = carry2 + po_fq_popc(m2 & (below | bit));
    *value = c < L ? c : L;
    return true;
}

// Q of one base from its five log-odds (quality.phred): own is the column of the called base, the other four are the
// alternatives.  NaN among them gives 0.
PO_FQ_HD inline int po_fq_phred(const double* odds, int own) {
    if (own < 0 || own > 4) return 0;
    const double INF = HUGE_VAL;
    double m = -INF;
    for (int b = 0; b < 5; ++b) {
        if (b == own) continue;
        const double v = odds[b];
        if (v != v) return 0;
        m = v > m ? v : m;
    }
    if (m == INF) return 0;
    if (m == -INF) return PO_FQ_QMAX;
    double sum = 0.0;
    for (int b = 0; b < 5; ++b)
        if (b != own) sum += exp(odds[b] - m);
    const double la = log(sum) + m;                                       // log of the alternatives' odds
    const double lae = la > 0.0 ? la + log1p(exp(-la)) : log1p(exp(la));  // logaddexp(la, 0)
    const double log_e = la - lae;
    const double q = -10.0 * log_e / 2.302585092994046;                   // ln 10
    const double r = floor(q + 0.5);
    return r < 0.0 ? 0 : r > (double)PO_FQ_QMAX ? PO_FQ_QMAX : (int)r;
}

// Q of one consensus base from the five log-odds it has on each read's table; ok1 / ok2: that table's lattice stands
// (quality status 0).  The sum is a float64 add per value: there is no product next to it to contract with.
PO_FQ_HD inline int po_fq_pair_phred(const double* odds1, const double* odds2, bool ok1, bool ok2, int own) {
    if (!ok1 && !ok2) return 0;
    double o[5];
    for (int b = 0; b < 5; ++b) o[b] = (ok1 && ok2) ? odds1[b] + odds2[b] : ok1 ? odds1[b] : odds2[b];
    return po_fq_phred(o, own);
}

// the alphabet index of a base (4 symbols), or -1
PO_FQ_HD inline int po_fq_code(const char* alphabet, char c) {
    for (int b = 0; b < 4; ++b)
        if (alphabet[b] == c) return b;
    return -1;
}
