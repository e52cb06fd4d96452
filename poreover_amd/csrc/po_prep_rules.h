// Signal preparation, once: the abasic filter and the five scalings of network.parse_fast5 as a rule on
// exact integers, used by the kernels of po_prep.hip, by po_signal_prep_h's host side and by tools/prep_check.cpp, which
// compiles this file alone (no HIP) under sanitizers.  tests/_prep_oracle.py states the same rule in Python.
//
// A raw sample x (int16) is kept when lo < x < hi, so a read's statistics are functions of its histogram over the
// bins x - (lo + 1) = 0 .. hi - lo - 2, PO_PREP_MAX_BINS of them at most.  From the histogram, as exact integers:
//   n = the kept samples, S = sum x, Q = sum x^2, min, max, and the order statistics (n - 1) / 2 and n / 2 (0-based).
// Every output is f32((f64(x) - a) / b): one rounding in the subtraction, one in the division, one in the cast
// (numpy's operation order), with f64 a and b per read:
//   standard  a = f64(S) / f64(n), b = sqrt(f64(N) / (f64(n) * f64(n))), N = n Q - S^2
//   current   a = -offset, b = alpha                       (both given per read; alpha = digitisation / range)
//   median    a = 0, b = f64(med_lo + med_hi) / 2
//   rescale   a = f64(S) / f64(n), b = f64(max - min)
//   raw       a = 0, b = 1
// N is computed in 128-bit unsigned integers (PoU128 below: two 64-bit words, products from 32-bit halves) on the
// coordinates y = x - (lo + 1) >= 0, in which it has the same value (the variance numerator does not depend on a shift),
// and converted to f64 with one rounding to nearest even.  n = 0: S / n = 0 / 0 = NaN, and b is NaN for standard, median
// and rescale (numpy's mean, std and median of an empty array; its max refuses); min = max = med_lo = med_hi = 0.  b = 0
// divides as IEEE does.  A read is shorter than 2^31 samples, so a bin count fits 32 bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"

#ifdef __HIPCC__
#define PO_PREP_HD __host__ __device__
#else
#define PO_PREP_HD
#endif

constexpr int PO_PREP_MAX_BINS = 4096;    // hi - lo - 1 at most
constexpr int PO_PREP_SLAB = 4096;        // raw samples per slab: a read is cut into slabs from its own first sample on
constexpr int PO_PREP_TPB = 256;          // threads per workgroup of every kernel of po_prep.hip
constexpr int PO_PREP_VEC = 8;            // int16 per load: 16 bytes

// ---- 128-bit unsigned integers: what n Q - S^2 needs from about 3.8 M kept samples on
struct PoU128 { uint64_t hi, lo; };

PO_PREP_HD inline PoU128 po_u128_mul(uint64_t a, uint64_t b) {
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);   // < 3 * 2^32
    PoU128 r;
    r.lo = (p00 & 0xffffffffu) | (mid << 32);
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}

// a - b for a >= b
PO_PREP_HD inline PoU128 po_u128_sub(PoU128 a, PoU128 b) {
    PoU128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
    return r;
}

// the nearest f64, ties to even: the top 64 bits with every lower bit folded into the lowest of them (it lies 11 places
// below the rounding point, so the rounding of the 64-bit conversion sees what the 128 bits would show it), then an exact
// scaling by a power of two
PO_PREP_HD inline double po_u128_to_f64(PoU128 v) {
    if (v.hi == 0) return (double)v.lo;
    int s = 0;
    while (!((v.hi << s) >> 63)) ++s;
    uint64_t m = s ? (v.hi << s) | (v.lo >> (64 - s)) : v.hi;
    if (s ? (v.lo << s) != 0 : v.lo != 0) m |= 1u;
    return ldexp((double)m, 64 - s);
}

// ---- a read's statistics
// po_prep_stats (include/poreover_hip.h): n, S, Q; min, max, med_lo, med_hi; a, b
struct PoPrepSums {          // of a histogram, in the coordinates y = bin index
    uint64_t n, sy, qy;      // kept samples, sum y, sum y^2
    int32_t ymin, ymax;      // the first and the last occupied bin (0 when n = 0)
    int32_t ylo, yhi;        // the bins of the order statistics (n - 1) / 2 and n / 2 (0 when n = 0)
};

// The scaling's a and b, and the statistics in the coordinates x = y + lo + 1.
PO_PREP_HD inline void po_prep_finish(const PoPrepSums& h, int scaling, int lo, double offset, double alpha, po_prep_stats* st) {
    const int64_t c = (int64_t)lo + 1;
    const int64_t n = (int64_t)h.n;
    st->n = n;
    st->S = c * n + (int64_t)h.sy;
    st->Q = c * c * n + 2 * c * (int64_t)h.sy + (int64_t)h.qy;
    st->min = n ? (int32_t)(h.ymin + c) : 0;
    st->max = n ? (int32_t)(h.ymax + c) : 0;
    st->med_lo = n ? (int32_t)(h.ylo + c) : 0;
    st->med_hi = n ? (int32_t)(h.yhi + c) : 0;
    const double nan = (double)NAN;
    const double mean = (double)st->S / (double)n;    // 0 / 0 = NaN for n = 0
    double a = 0.0, b = 1.0;
    if (scaling == PO_SCALE_STANDARD) {
        const PoU128 N = po_u128_sub(po_u128_mul(h.n, h.qy), po_u128_mul(h.sy, h.sy));
        a = mean;
        b = sqrt(po_u128_to_f64(N) / ((double)n * (double)n));
    } else if (scaling == PO_SCALE_CURRENT) {
        a = -offset;
        b = alpha;
    } else if (scaling == PO_SCALE_MEDIAN) {
        b = n ? (double)((int64_t)st->med_lo + st->med_hi) / 2.0 : nan;
    } else if (scaling == PO_SCALE_RESCALE) {
        a = mean;
        b = n ? (double)((int64_t)st->max - st->min) : nan;
    }
    st->a = a;
    st->b = b;
}

PO_PREP_HD inline bool po_prep_keep(int x, int lo, int hi) { return x > lo && x < hi; }
PO_PREP_HD inline float po_prep_scale(int x, double a, double b) { return (float)(((double)x - a) / b); }

// ---- host only: the argument checks that need no device, and the slab list
struct PoPrepPlan {
    int bins = 0;
    int64_t total = 0;                 // raw samples of all reads
    std::vector<int64_t> slab_off;     // [n_reads + 1] first slab of each read
    std::vector<int32_t> slab_read;    // [slabs] the read a slab belongs to
};

// Checks scaling, lo / hi and the offsets (from 0, non-decreasing, a read shorter than 2^31), then fills *p.  Returns
// PO_OK or PO_E_ARG with *err naming the value under the name of the entry that asks.  Touches no device.
inline int po_prep_make_plan(const int64_t* raw_off_h, int n_reads, int scaling, int lo, int hi, PoPrepPlan* p, std::string* err,
                             const char* entry = "po_signal_prep_h") {
    const std::string me = std::string(entry) + ": ";
    if (scaling < PO_SCALE_STANDARD || scaling > PO_SCALE_RAW) { *err = me + "scaling " + std::to_string(scaling); return PO_E_ARG; }
    if (lo < -32769 || hi > 32768 || hi <= lo) {
        *err = me + "lo " + std::to_string(lo) + ", hi " + std::to_string(hi) + " (-32769 <= lo < hi <= 32768)";
        return PO_E_ARG;
    }
    if ((int64_t)hi - lo - 1 > PO_PREP_MAX_BINS) {
        *err = me + "lo " + std::to_string(lo) + ", hi " + std::to_string(hi) + ": " + std::to_string((int64_t)hi - lo - 1) +
               " bins (at most " + std::to_string(PO_PREP_MAX_BINS) + ")";
        return PO_E_ARG;
    }
    if (raw_off_h[0] != 0) { *err = me + "raw_off[0] is " + std::to_string(raw_off_h[0]) + " (must be 0)"; return PO_E_ARG; }
    int64_t slabs = 0;
    for (int r = 0; r < n_reads; ++r) {
        const int64_t L = raw_off_h[r + 1] - raw_off_h[r];
        if (L < 0 || L > INT32_MAX) {
            *err = me + "read " + std::to_string(r) + " has " + std::to_string(L) + " samples (0 to 2^31 - 1)";
            return PO_E_ARG;
        }
        slabs += (L + PO_PREP_SLAB - 1) / PO_PREP_SLAB;
        if (slabs > INT32_MAX) { *err = me + "more than 2^31 - 1 slabs"; return PO_E_ARG; }
    }
    p->bins = hi - lo - 1;
    p->total = raw_off_h[n_reads];
    p->slab_off.assign((size_t)n_reads + 1, 0);
    p->slab_read.resize((size_t)slabs);
    for (int r = 0; r < n_reads; ++r) {
        const int64_t k = (raw_off_h[r + 1] - raw_off_h[r] + PO_PREP_SLAB - 1) / PO_PREP_SLAB;
        for (int64_t j = 0; j < k; ++j) p->slab_read[(size_t)(p->slab_off[r] + j)] = r;
        p->slab_off[r + 1] = p->slab_off[r] + k;
    }
    return PO_OK;
}

// The whole rule on the host, read by read: what the kernels must give bit for bit (tools/prep_check.cpp).  signal gets the
// kept samples back to back, sig_off[n_reads + 1] their offsets from 0.
inline void po_prep_host(const int16_t* raw, const int64_t* raw_off, int n_reads, int scaling, int lo, int hi, const double* offset,
                         const double* alpha, std::vector<float>* signal, std::vector<int64_t>* sig_off,
                         std::vector<po_prep_stats>* stats) {
    const int bins = hi - lo - 1;
    signal->clear();
    sig_off->assign(1, 0);
    stats->resize((size_t)n_reads);
    std::vector<uint32_t> hist((size_t)bins);
    for (int r = 0; r < n_reads; ++r) {
        std::fill(hist.begin(), hist.end(), 0u);
        for (int64_t i = raw_off[r]; i < raw_off[r + 1]; ++i)
            if (po_prep_keep(raw[i], lo, hi)) ++hist[(size_t)(raw[i] - lo - 1)];
        PoPrepSums h = {0, 0, 0, 0, 0, 0, 0};
        for (int y = 0; y < bins; ++y) {
            if (!hist[(size_t)y]) continue;
            if (!h.n) h.ymin = y;
            h.ymax = y;
            h.n += hist[(size_t)y];
            h.sy += (uint64_t)y * hist[(size_t)y];
            h.qy += (uint64_t)y * y * hist[(size_t)y];
        }
        if (h.n) {
            const uint64_t klo = (h.n - 1) / 2, khi = h.n / 2;
            uint64_t run = 0;
            for (int y = 0; y < bins; ++y) {
                const uint64_t next = run + hist[(size_t)y];
                if (klo >= run && klo < next) h.ylo = y;
                if (khi >= run && khi < next) h.yhi = y;
                run = next;
            }
        }
        po_prep_stats& st = (*stats)[(size_t)r];
        po_prep_finish(h, scaling, lo, offset ? offset[r] : 0.0, alpha ? alpha[r] : 1.0, &st);
        for (int64_t i = raw_off[r]; i < raw_off[r + 1]; ++i)
            if (po_prep_keep(raw[i], lo, hi)) signal->push_back(po_prep_scale(raw[i], st.a, st.b));
        sig_off->push_back((int64_t)signal->size());
    }
}
