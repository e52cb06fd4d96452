// The rounding rule of `--precision bf16` (poreover_amd/csrc/po_bf16_rules.h), the part of the feature that needs no device:
// the same source w_to_bf16_kernel runs.  Plain C++, no HIP: built and run under -fsanitize=address,undefined by
// tests/test_call_bf16_cpu.py.  Exit status 0 and "ok" when every case holds.
//
// The rule is held against a brute-force statement of it: the two bf16 neighbours of a finite f32 (its upper 16 bits, and
// those plus one in the magnitude — past the largest finite bf16 that is the pattern of inf, which stands for 2^128 as IEEE
// rounding has it) are compared with the value in double, where f32 values and their differences are exact; the nearer one
// wins, a tie goes to the neighbour whose last kept bit is 0.
//   every exponent 0..254 (subnormals included) x the tie patterns and their neighbours in the discarded half x kept parts of
//   both parities x both signs; NaN payloads (quiet and signalling, both signs); +-inf, +-0, +-FLT_MAX; 2^22 pseudo-random
//   patterns; every array in a heap block of exactly its size
//
// The split of `--recurrence bf16x3` (po_bf16_split) is held against its own statement on the same patterns: hi is the rule's
// rounding of f; f - hi is exact (the f32 difference equals the difference in double); lo is the rule's rounding of that
// difference; hi + lo is within 2^-16 of f, relatively, wherever the remainder is zero or a normal bf16 value (|r| >= 2^-126);
// NaN, +-inf, an overflowing rounding and +-0 behave as the rule's comment promises.
#include "../poreover_amd/csrc/po_bf16_rules.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
static long checked = 0;

static void fail(const char* what, unsigned long a = 0, unsigned long b = 0, unsigned long c = 0) {
    if (failures < 20) std::printf("FAILED %s (%#lx, %#lx, %#lx)\n", what, a, b, c);
    ++failures;
}

static double value_of(uint32_t bits) {   // the f32 of these bits; the pattern of inf stands for 2^128 (sign kept)
    if ((bits & 0x7fffffffu) == 0x7f800000u) return (bits >> 31) ? -std::ldexp(1.0, 128) : std::ldexp(1.0, 128);
    float f;
    std::memcpy(&f, &bits, 4);
    return (double)f;
}

static uint16_t brute(uint32_t u) {   // u finite
    const uint32_t lo = u & 0xffff0000u, hi = lo + 0x10000u;   // towards zero, away from zero
    const double d = value_of(u), dl = std::fabs(d - value_of(lo)), dh = std::fabs(value_of(hi) - d);
    if (dl < dh) return (uint16_t)(lo >> 16);
    if (dh < dl) return (uint16_t)(hi >> 16);
    return (uint16_t)(((lo >> 16) & 1u) ? hi >> 16 : lo >> 16);
}

static void check_finite(uint32_t u) {
    const uint16_t want = brute(u), got = po_bf16_bits_from_f32_bits(u);
    ++checked;
    if (got != want) fail("rule vs brute force", u, got, want);
    float f;
    std::memcpy(&f, &u, 4);
    if (po_bf16_from_f32(f) != got) fail("po_bf16_from_f32 vs the bit form", u);
    // rounding is idempotent, and the float form carries exactly the bf16
    const float r = po_round_bf16(f);
    uint32_t rb;
    std::memcpy(&rb, &r, 4);
    if (rb != (uint32_t)got << 16) fail("po_round_bf16", u, rb, got);
    if (po_bf16_from_f32(r) != got) fail("idempotence", u);
}

static void check_split(uint32_t u) {   // any pattern
    float f;
    std::memcpy(&f, &u, 4);
    uint16_t hi = 0xdead, lo = 0xdead;
    po_bf16_split(f, &hi, &lo);
    ++checked;
    if (hi != po_bf16_bits_from_f32_bits(u)) fail("split: hi is not the rule's rounding", u, hi);
    if ((hi & 0x7f80) == 0x7f80) {   // NaN, inf, or a finite value that overflows: no remainder
        if (lo != 0) fail("split: lo of a non-finite hi is not +0", u, hi, lo);
        if ((u & 0x7fffffffu) > 0x7f800000u && (hi & 0x007f) == 0) fail("split: NaN became inf", u, hi);
        return;
    }
    const double d = (double)f, dh = (double)po_f32_from_bf16(hi);
    const float rf = f - po_f32_from_bf16(hi);
    if ((double)rf != d - dh) fail("split: f - hi is not exact in f32", u, hi);
    uint32_t rb;
    std::memcpy(&rb, &rf, 4);
    if (lo != brute(rb)) fail("split: lo is not the brute-force rounding of the remainder", u, lo, brute(rb));
    if ((u & 0x7fffffffu) == 0) {   // +-0: hi keeps the sign, lo is +0
        if (hi != (uint16_t)(u >> 16) || lo != 0) fail("split: zero", u, hi, lo);
        return;
    }
    if (rf == 0.0f || std::fabs(rf) >= 0x1p-126f) {
        const double sum = dh + (double)po_f32_from_bf16(lo);
        if (std::fabs(sum - d) > std::ldexp(std::fabs(d), -16)) fail("split: hi + lo is further than 2^-16 from f", u, hi, lo);
    }
}

int main() {
    // ---- every exponent x patterns of the discarded half x kept parts of both parities x both signs
    const std::vector<uint32_t> low = {0x0000, 0x0001, 0x7ffe, 0x7fff, 0x8000, 0x8001, 0x8002, 0xfffe, 0xffff, 0x4000, 0xc000};
    const std::vector<uint32_t> kept = {0x00, 0x01, 0x02, 0x03, 0x3e, 0x3f, 0x40, 0x41, 0x7c, 0x7d, 0x7e, 0x7f};
    for (uint32_t e = 0; e <= 254; ++e)
        for (uint32_t k : kept)
            for (uint32_t l : low)
                for (uint32_t s = 0; s < 2; ++s) check_finite((s << 31) | (e << 23) | (k << 16) | l);
    for (uint32_t e = 0; e <= 255; ++e)   // (255: inf and NaN patterns)
        for (uint32_t k : kept)
            for (uint32_t l : low)
                for (uint32_t s = 0; s < 2; ++s) check_split((s << 31) | (e << 23) | (k << 16) | l);
    // ---- the split by hand: 1 + 2^-8 is a tie for hi (down to 1, remainder 2^-8 exactly); 1 + 2^-9 + 2^-17 rounds down to 1 and
    // its remainder 2^-9 (1 + 2^-8) is a tie for lo (down to 2^-9); 1 + 2^-9 + 3 2^-17 leaves 2^-9 (1 + 3 2^-8): a tie that goes up;
    // 1 + 3 2^-8 goes up to 1 + 2^-6 and leaves -2^-8
    struct { float in, hi, lo; } split[] = {
        {1.0f + 0x1p-8f, 1.0f, 0x1p-8f}, {1.0f + 0x1p-9f + 0x1p-17f, 1.0f, 0x1p-9f},
        {1.0f + 0x1p-9f + 3 * 0x1p-17f, 1.0f, 0x1p-9f * (1.0f + 0x1p-6f)}, {1.0f + 3 * 0x1p-8f, 1.0f + 0x1p-6f, -0x1p-8f},
        {-(1.0f + 0x1p-9f + 0x1p-17f), -1.0f, -0x1p-9f}, {1.5f, 1.5f, 0.0f}, {0.0f, 0.0f, 0.0f}, {-0.0f, -0.0f, 0.0f},
        {INFINITY, INFINITY, 0.0f}, {-INFINITY, -INFINITY, 0.0f}, {FLT_MAX, INFINITY, 0.0f}, {-FLT_MAX, -INFINITY, 0.0f}};
    for (const auto& h : split) {
        uint16_t hi, lo;
        po_bf16_split(h.in, &hi, &lo);
        const float fh = po_f32_from_bf16(hi), fl = po_f32_from_bf16(lo);
        if (std::memcmp(&fh, &h.hi, 4) != 0 || std::memcmp(&fl, &h.lo, 4) != 0) {
            uint32_t a;
            std::memcpy(&a, &h.in, 4);
            fail("split hand vector", a, hi, lo);
        }
    }
    // ---- hand vectors
    struct { float in, out; } hand[] = {
        {1.0f + 0x1p-8f, 1.0f}, {1.0f + 3 * 0x1p-8f, 1.0f + 0x1p-6f}, {-(1.0f + 0x1p-8f), -1.0f},
        {1.0f + 0x1p-8f + 0x1p-23f, 1.0f + 0x1p-7f}, {FLT_MAX, INFINITY}, {-FLT_MAX, -INFINITY}, {INFINITY, INFINITY},
        {-INFINITY, -INFINITY}, {0.0f, 0.0f}, {-0.0f, -0.0f}, {1.5f, 1.5f}, {-3.0f, -3.0f}};
    for (const auto& h : hand) {
        const float r = po_round_bf16(h.in);
        if (std::memcmp(&r, &h.out, 4) != 0) {
            uint32_t a, b;
            std::memcpy(&a, &h.in, 4);
            std::memcpy(&b, &r, 4);
            fail("hand vector", a, b);
        }
    }
    // the largest f32 that still rounds to the largest finite bf16, and the first that overflows (the tie goes to even = inf)
    if (po_bf16_bits_from_f32_bits(0x7f7f7fffu) != 0x7f7f) fail("below the overflow tie");
    if (po_bf16_bits_from_f32_bits(0x7f7f8000u) != 0x7f80) fail("the overflow tie");
    if (po_bf16_bits_from_f32_bits(0xff7f8000u) != 0xff80) fail("the overflow tie, negative");
    // ---- NaN stays NaN: quiet and signalling payloads, payloads that live only in the discarded half, both signs
    const std::vector<uint32_t> payload = {0x400000, 0x400001, 0x000001, 0x00ffff, 0x010000, 0x3fffff, 0x7fffff, 0x7f0000, 0x008000};
    for (uint32_t p : payload)
        for (uint32_t s = 0; s < 2; ++s) {
            const uint32_t u = (s << 31) | 0x7f800000u | p;
            const uint16_t b = po_bf16_bits_from_f32_bits(u);
            ++checked;
            if ((b & 0x7f80) != 0x7f80 || (b & 0x007f) == 0) fail("NaN became a number or inf", u, b);
            if ((uint32_t)(b >> 15) != s) fail("NaN lost its sign", u, b);
            const float r = po_f32_from_bf16(b);
            if (!std::isnan(r)) fail("po_f32_from_bf16 of a NaN", u, b);
        }
    // ---- pseudo-random patterns (an LCG), in a heap block of exactly their size and results in another
    const size_t N = (size_t)1 << 22;
    std::vector<float> in(N);
    std::vector<uint16_t> out(N);
    uint32_t x = 0x2545f491u;
    for (size_t i = 0; i < N; ++i) {
        x = x * 1664525u + 1013904223u;
        uint32_t u = x ^ (x >> 15);
        if ((u & 0x7f800000u) == 0x7f800000u) u &= 0xff7fffffu;   // keep it finite (NaN and inf have their cases above)
        std::memcpy(&in[i], &u, 4);
    }
    for (size_t i = 0; i < N; ++i) out[i] = po_bf16_from_f32(in[i]);
    for (size_t i = 0; i < N; ++i) {
        uint32_t u;
        std::memcpy(&u, &in[i], 4);
        ++checked;
        if (out[i] != brute(u)) fail("random pattern", u, out[i], brute(u));
        if ((i & 3) == 0) check_split(u);
    }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok (%ld values)\n", checked);
    return 0;
}
