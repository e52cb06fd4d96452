// The signal preparation rule (poreover_amd/csrc/po_prep_rules.h), the part of po_signal_prep_h that needs no device.  Plain
// C++, no HIP: built and run under -fsanitize=address,undefined by tests/test_prep_cpu.py.  Exit status 0 and "ok" when
// every case holds.
//   - the 128-bit product, difference and conversion to f64 against the compiler's unsigned __int128;
//   - a read's integer statistics against a sort of its kept samples, its a and b against the definitions, every scaling;
//   - the filter's edges, an even count with unlike middle values, n = 0 and b = 0, the variance numerator past 64 bits;
//   - the slab tables of a ragged batch, each in a heap block of exactly its size, and every refusal with its message.
#include "../poreover_amd/csrc/po_prep_rules.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

static int failures = 0;

static void fail(const char* what, long a = 0, long b = 0) {
    std::printf("FAILED %s (%ld, %ld)\n", what, a, b);
    ++failures;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (std::isnan(a) && std::isnan(b)); }

static void check_u128() {
    typedef unsigned __int128 u128;
    const uint64_t edge[] = {0, 1, 2, 0xffffffffull, 0x100000000ull, 0x1fffffffffffffull, 0x20000000000001ull, ~0ull, ~0ull - 1, 1ull << 63};
    for (int i = 0; i < 20000; ++i) {
        uint64_t a = rnd() >> (rnd() % 64), b = rnd() >> (rnd() % 64);
        if (i < 100) { a = edge[i / 10]; b = edge[i % 10]; }
        const PoU128 p = po_u128_mul(a, b);
        const u128 want = (u128)a * b;
        if (p.hi != (uint64_t)(want >> 64) || p.lo != (uint64_t)want) fail("128-bit product", i);
        if (!same(po_u128_to_f64(p), (double)want)) fail("128-bit value to f64", i);
        // every bit pattern below the rounding point: a value just under, at and just over a tie
        for (int d = -1; d <= 1; ++d) {
            const u128 t = (((u128)(a | (1ull << 63)) << 64) >> (rnd() % 64)) + (u128)(int64_t)d + ((u128)1 << (rnd() % 70));
            const PoU128 v = {(uint64_t)(t >> 64), (uint64_t)t};
            if (!same(po_u128_to_f64(v), (double)t)) fail("rounding to nearest even", i, d);
        }
        const uint64_t c = rnd() >> (rnd() % 64), e = rnd() >> (rnd() % 64);
        u128 x = (u128)a * b, y = (u128)c * e;
        PoU128 px = p, py = po_u128_mul(c, e);
        if (x < y) { std::swap(x, y); std::swap(px, py); }
        const PoU128 dif = po_u128_sub(px, py);
        if (dif.hi != (uint64_t)((x - y) >> 64) || dif.lo != (uint64_t)(x - y)) fail("128-bit difference", i);
    }
}

struct Out {
    std::vector<float> sig;
    std::vector<int64_t> off;
    std::vector<po_prep_stats> st;
};

static Out run(const std::vector<std::vector<int16_t>>& reads, int scaling, int lo, int hi, const std::vector<double>* offset = nullptr,
               const std::vector<double>* alpha = nullptr) {
    std::vector<int16_t> raw;   // exact heap blocks: a read past an end is a sanitizer report
    std::vector<int64_t> off(1, 0);
    for (const auto& r : reads) {
        raw.insert(raw.end(), r.begin(), r.end());
        off.push_back((int64_t)raw.size());
    }
    raw.shrink_to_fit();
    Out o;
    po_prep_host(raw.data(), off.data(), (int)reads.size(), scaling, lo, hi, offset ? offset->data() : nullptr,
                 alpha ? alpha->data() : nullptr, &o.sig, &o.off, &o.st);
    return o;
}

// one read against the definitions, computed another way: a sort for the order statistics, long double sums
static void check_read(const std::vector<int16_t>& read, int lo, int hi, int tag) {
    std::vector<int64_t> kept;
    for (int16_t x : read)
        if (x > lo && x < hi) kept.push_back(x);
    std::vector<int64_t> sorted(kept);
    std::sort(sorted.begin(), sorted.end());
    const int64_t n = (int64_t)kept.size();
    int64_t S = 0, Q = 0;
    for (int64_t x : kept) { S += x; Q += x * x; }
    const std::vector<double> offset = {12.5}, alpha = {8192.0 / 1425.42};
    for (int scaling = PO_SCALE_STANDARD; scaling <= PO_SCALE_RAW; ++scaling) {
        const Out o = run({read}, scaling, lo, hi, &offset, &alpha);
        const po_prep_stats& st = o.st[0];
        if (st.n != n || st.S != S || st.Q != Q) fail("n, S, Q", tag, scaling);
        if (o.off.size() != 2 || o.off[1] != n || (int64_t)o.sig.size() != n) fail("offsets", tag, scaling);
        if (n) {
            if (st.min != sorted.front() || st.max != sorted.back()) fail("min, max", tag, scaling);
            if (st.med_lo != sorted[(size_t)((n - 1) / 2)] || st.med_hi != sorted[(size_t)(n / 2)]) fail("middle order statistics", tag, scaling);
        } else if (st.min || st.max || st.med_lo || st.med_hi) {
            fail("an empty read's integers are 0", tag, scaling);
        }
        double a = 0, b = 1;
        if (scaling == PO_SCALE_STANDARD) {
            a = (double)S / (double)n;
            const unsigned __int128 N = (unsigned __int128)n * Q - (unsigned __int128)S * S;
            b = std::sqrt((double)N / ((double)n * (double)n));
        } else if (scaling == PO_SCALE_CURRENT) {
            a = -offset[0];
            b = alpha[0];
        } else if (scaling == PO_SCALE_MEDIAN) {
            b = n ? (double)(sorted[(size_t)((n - 1) / 2)] + sorted[(size_t)(n / 2)]) / 2.0 : (double)NAN;
        } else if (scaling == PO_SCALE_RESCALE) {
            a = (double)S / (double)n;
            b = n ? (double)(sorted.back() - sorted.front()) : (double)NAN;
        }
        if (!same(st.a, a) || !same(st.b, b)) fail("a, b", tag, scaling);
        for (int64_t i = 0; i < n; ++i) {
            const float want = (float)(((double)kept[(size_t)i] - a) / b);
            if (std::memcmp(&want, &o.sig[(size_t)i], 4) != 0 && !(std::isnan(want) && std::isnan(o.sig[(size_t)i]))) {
                fail("a sample", tag, scaling);
                break;
            }
        }
    }
}

static void refused(const char* name, const std::vector<int64_t>& off, int scaling, int lo, int hi, const char* needle) {
    std::vector<int64_t> a(off);
    PoPrepPlan p;
    std::string err;
    const int rc = po_prep_make_plan(a.data(), (int)a.size() - 1, scaling, lo, hi, &p, &err);
    if (rc != PO_E_ARG || err.find(needle) == std::string::npos || err.find("po_signal_prep_h: ") != 0) {
        std::printf("FAILED refusal %s: code %d, message \"%s\"\n", name, rc, err.c_str());
        ++failures;
    }
}

int main() {
    check_u128();

    check_read({200, 201, 799, 800, 500, -5, 32767, -32768, 201}, 200, 800, 1);   // the filter's edges
    check_read({300, 700, 301, 699}, 200, 800, 2);                                // even n, middle values 301 and 699
    check_read({300, 700, 301}, 200, 800, 3);
    check_read({}, 200, 800, 4);                                                  // n = 0
    check_read({100, 900, 200, 800}, 200, 800, 5);                                // nothing kept
    check_read({444, 444, 444}, 200, 800, 6);                                     // b = 0 for standard and rescale
    check_read({-3, -2, -1, 0, 1, 2, 3}, -3, 3, 7);                               // another range, negative values
    check_read({5}, 4, 6, 8);                                                     // one bin
    {
        std::vector<int16_t> r(5000);
        for (auto& x : r) x = (int16_t)(150 + rnd() % 700);
        check_read(r, 200, 800, 9);
        check_read(r, -32769, -32769 + PO_PREP_MAX_BINS + 1, 10);                 // the widest range, nothing in it
        for (auto& x : r) x = (int16_t)(rnd() % 4096 - 100);
        check_read(r, -101, 3996, 11);                                            // the widest range, everything in it
    }
    {   // two reads, the first empty: offsets 0, 0, 2
        const Out o = run({{100}, {300, 301}}, PO_SCALE_RAW, 200, 800);
        if (o.off != std::vector<int64_t>({0, 0, 2}) || o.sig != std::vector<float>({300.f, 301.f})) fail("a batch's offsets");
    }
    {   // the variance numerator past 64 bits, from sums alone: 2^33 samples, half in bin 0 and half in bin 4095
        PoPrepSums h = {1ull << 33, (1ull << 32) * 4095, (1ull << 32) * 4095 * 4095, 0, 4095, 0, 4095};
        po_prep_stats st;
        po_prep_finish(h, PO_SCALE_STANDARD, 200, 0.0, 1.0, &st);
        if (!same(st.a, 201.0 + 2047.5) || !same(st.b, 2047.5)) fail("variance numerator past 64 bits");
    }

    {   // reads of 0, 1, 4096, 4097 and 9000 samples: 0, 1, 1, 2 and 3 slabs
        const std::vector<int64_t> off = {0, 0, 1, 4097, 8194, 17194};
        std::vector<int64_t> a(off);
        PoPrepPlan p;
        std::string err;
        if (po_prep_make_plan(a.data(), 5, PO_SCALE_MEDIAN, 200, 800, &p, &err) != PO_OK) fail("ragged plan accepted");
        if (p.slab_off != std::vector<int64_t>({0, 0, 1, 2, 4, 7}) || p.slab_read != std::vector<int32_t>({1, 2, 3, 3, 4, 4, 4}) ||
            p.bins != 599 || p.total != 17194)
            fail("ragged plan tables");
        std::vector<int64_t> none = {0};
        if (po_prep_make_plan(none.data(), 0, PO_SCALE_RAW, 200, 800, &p, &err) != PO_OK || !p.slab_read.empty() || p.slab_off.size() != 1)
            fail("empty batch");
    }
    const std::vector<int64_t> two = {0, 5, 9};
    refused("scaling 5", two, 5, 200, 800, "scaling 5");
    refused("scaling -1", two, -1, 200, 800, "scaling -1");
    refused("hi = lo", two, 0, 200, 200, "lo 200, hi 200");
    refused("hi < lo", two, 0, 800, 200, "lo 800, hi 200");
    refused("lo out of range", two, 0, -40000, -39000, "lo -40000");
    refused("hi out of range", two, 0, 30000, 32769, "hi 32769");
    refused("one bin over the cap", two, 0, 0, PO_PREP_MAX_BINS + 2, "4097 bins (at most 4096)");
    refused("offsets not from 0", {3, 8}, 0, 200, 800, "raw_off[0] is 3");
    refused("decreasing offsets", {0, 5, 3}, 0, 200, 800, "read 1 has -2 samples");
    refused("a read of 2^31 samples", {0, (int64_t)1 << 31}, 0, 200, 800, "read 0 has 2147483648 samples");
    {
        std::vector<int64_t> a = {0, 1};
        PoPrepPlan p;
        std::string err;
        if (po_prep_make_plan(a.data(), 1, 0, 0, PO_PREP_MAX_BINS + 1, &p, &err) != PO_OK || p.bins != PO_PREP_MAX_BINS) fail("the cap itself is accepted");
    }
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
