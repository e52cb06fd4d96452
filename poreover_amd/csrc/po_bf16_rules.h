// The rounding of `--precision bf16`, once: f32 -> bf16 by round-to-nearest-even on the upper 16 bits.
// The weight conversion kernel of po_call_bf16.h and the host use this function; the projection kernel rounds x with the
// hardware's packed conversion, which the device test holds against this rule at exact ties.  No HIP in this file:
// tools/bf16_check.cpp compiles it alone under sanitizers and holds it against a brute-force statement of the rule.
// po_bf16_split (below) is the operand split of `--recurrence bf16x3`, for the host and the device.
//   NaN stays a NaN (quiet, sign kept); +-inf and +-0 are kept; a finite value whose rounding overflows becomes +-inf
#pragma once
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define PO_BF_HD __host__ __device__
#else
#define PO_BF_HD
#endif

// the bf16 bit pattern nearest the f32 bit pattern u, ties to the even pattern
PO_BF_HD inline uint16_t po_bf16_bits_from_f32_bits(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);   // NaN: keep the top payload, set quiet
    // add half an ulp of the kept part, less one where the kept part is even: a tie goes to the even neighbour.  The carry
    // runs into the exponent, so 0x7f7f.... with its upper discarded half rounds to 0x7f80 = inf, and inf itself stays.
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

PO_BF_HD inline uint16_t po_bf16_from_f32(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return po_bf16_bits_from_f32_bits(u);
}

PO_BF_HD inline float po_f32_from_bf16(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// f rounded to bf16, as an f32
PO_BF_HD inline float po_round_bf16(float f) { return po_f32_from_bf16(po_bf16_from_f32(f)); }

// The split of `--recurrence bf16x3`: f as two bf16 values, hi = bf16(f) and lo = bf16(f - hi).  For a
// finite f whose hi is finite, f - hi is exact in f32 (at most 16 significant bits, a multiple of f's own last place), so
// hi + lo is f rounded ONCE more: within 2^-16 of f, relatively, wherever the remainder is a normal bf16 value.
//   NaN: hi is the NaN of the rule above, lo is +0.  +-inf, and a finite f whose hi overflows to +-inf: hi is that inf and
//   lo is +0 (no remainder of an infinite value: hi + lo stays hi).  +-0: hi keeps the sign, lo is +0.
PO_BF_HD inline void po_bf16_split(float f, uint16_t* hi, uint16_t* lo) {
    const uint16_t h = po_bf16_from_f32(f);
    *hi = h;
    const uint16_t l = po_bf16_from_f32(f - po_f32_from_bf16(h));   // (inf - inf: a NaN, not kept)
    *lo = (h & 0x7f80u) == 0x7f80u ? (uint16_t)0 : l;
}
