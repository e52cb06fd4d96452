// The per-element rules of tensors.accuracy (poreover_amd/csrc/po_acc_rules.h), the part of the feature that needs no device:
// the same source the kernels of po_acc.hip run.  Plain C++, no HIP: built and run under -fsanitize=address,undefined by
// tests/test_tensors_accuracy_cpu.py.  Exit status 0 and "ok" when every case holds.
//   widen    every f16 bit pattern against the value built from its fields with ldexp, every bf16 pattern against its shift
//   argmax   po_acc_frame_class on frames of the four dtypes, read through a row stride, a column stride (0 included) and a
//            column order, against a restatement of the rule on the widened values in canonical order: every frame whose five
//            values come from {-1, 0, 0.5, 0.5 again, NaN}, infinities, all-NaN
//   emit     the kernel's loop (blocks of 64 frames, one ballot, the left neighbour's class, the class carried over the edge,
//            one carried count) against a frame-by-frame filter of either kind: every class pattern of up to 7 frames over
//            {0, 3, 4}, windows of 1 .. 200 frames, a repeat and a blank-separated repeat across frames 63 | 64 | 65
//   align    the packed key's wave walk (64 lanes, K columns each, the local pass, the exclusive prefix minimum as the kernel's
//            moves make it, the second pass, the pick, the decode) in every instantiation that can hold the pair, both ways
//            round: against the enumeration of EVERY alignment for la, lb <= 4 over 3 symbols (the lexicographic row DP and the
//            packed-key row DP on every such pair too), against the plain lexicographic row DP on random strings up to a few
//            hundred symbols, and at the widths' edges (63, 64, 127, 128 .. 4095 columns)
// Every array sits in a heap block of exactly its size.
#include "../poreover_amd/csrc/po_acc_rules.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

static int failures = 0;

static void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    if (failures < 20) std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
    ++failures;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

// ---- widen
static void widen() {
    for (uint32_t h = 0; h < 65536u; ++h) {
        const int e = (int)((h >> 10) & 31u), m = (int)(h & 1023u);
        const float got = po_acc_f16((uint16_t)h);
        if (e == 31) {
            if (m ? !std::isnan(got) : !(std::isinf(got) && (got < 0) == (bool)(h >> 15))) fail("f16 infinity / NaN", (long)h);
            continue;
        }
        float want = e ? std::ldexp((float)(1024 + m), e - 25) : std::ldexp((float)m, -24);
        if (h >> 15) want = -want;
        if (bits_of(got) != bits_of(want)) fail("f16", (long)h);
        const float b = po_acc_bf16((uint16_t)h);
        if (bits_of(b) != h << 16) fail("bf16", (long)h);
    }
}

// ---- argmax
static int rule_argmax(const std::vector<double>& p) {   // the issue's words, on the widened values in canonical order
    size_t best = 0;
    for (size_t c = 1; c < p.size(); ++c)
        if (p[c] > p[best] || (std::isnan(p[c]) && !std::isnan(p[best]))) best = c;
    return (int)best;
}

static int numpy_argmax(const std::vector<double>& p) {
    for (size_t c = 0; c < p.size(); ++c)
        if (std::isnan(p[c])) return (int)c;
    size_t best = 0;
    for (size_t c = 1; c < p.size(); ++c)
        if (p[c] > p[best]) best = c;
    return (int)best;
}

static uint16_t f16_of(float v) {   // of the few values used here, all exact in f16
    if (std::isnan(v)) return 0x7e00;
    if (std::isinf(v)) return v < 0 ? 0xfc00 : 0x7c00;
    if (v == 0.f) return 0;
    int e;
    const float f = std::frexp(std::fabs(v), &e);   // |v| = f * 2^e, f in [0.5, 1): a normal f16 where 1 <= e + 14 <= 30
    const uint16_t h = (uint16_t)((v < 0 ? 0x8000 : 0) | ((e + 14) << 10) | (int)((f * 2.f - 1.f) * 1024.f));
    if (e + 14 < 1 || e + 14 > 30 || po_acc_f16(h) != v) fail("a test value is no f16");
    return h;
}

// the frame `canon` (canonical order) stored at row t of a block of `dtype` with the given strides and column order, read back
static int stored_class(const std::vector<float>& canon, int dtype, int64_t row_stride, int64_t col_stride, int64_t t, const int* perm) {
    const size_t eb = (size_t)po_acc_elem_bytes(dtype);
    const size_t elems = (size_t)(t * row_stride + 4 * col_stride + 1);
    std::vector<char> buf(elems * eb, (char)0x5a);
    for (int c = 0; c < PO_ACC_CLASSES; ++c) {
        char* p = buf.data() + (size_t)(t * row_stride + perm[c] * col_stride) * eb;
        const float v = canon[(size_t)c];
        if (dtype == PO_ACC_F64) { const double d = v; std::memcpy(p, &d, 8); }
        else if (dtype == PO_ACC_F32) std::memcpy(p, &v, 4);
        else if (dtype == PO_ACC_BF16) { const uint16_t h = (uint16_t)(bits_of(v) >> 16); std::memcpy(p, &h, 2); }
        else { const uint16_t h = f16_of(v); std::memcpy(p, &h, 2); }
    }
    return po_acc_frame_class(buf.data(), row_stride, col_stride, t, dtype, perm);
}

static void argmax() {
    const float vals[5] = {-1.f, 0.f, 0.5f, 0.5f, NAN};
    const int ident[5] = {0, 1, 2, 3, 4}, bonito[5] = {1, 2, 3, 4, 0}, mixed[5] = {3, 0, 4, 2, 1};
    for (int code = 0; code < 5 * 5 * 5 * 5 * 5; ++code) {
        std::vector<float> p(PO_ACC_CLASSES);
        std::vector<double> d(PO_ACC_CLASSES);
        for (int c = 0, k = code; c < PO_ACC_CLASSES; ++c, k /= 5) d[(size_t)c] = p[(size_t)c] = vals[k % 5];
        const int want = rule_argmax(d);
        if (want != numpy_argmax(d)) fail("the rule is np.argmax", code);
        if (po_acc_argmax(p.data()) != want || po_acc_argmax(d.data()) != want) fail("argmax", code);
        const int dtype = code % 4;
        const int* perm = code % 3 == 0 ? ident : code % 3 == 1 ? bonito : mixed;
        if (stored_class(p, dtype, 5, 1, code % 4, perm) != want) fail("frame class, dense", code, dtype);
        if (stored_class(p, (dtype + 1) % 4, 13, 2, 3, perm) != want) fail("frame class, strided", code, dtype);
        if (stored_class(p, (dtype + 2) % 4, 0, 1, 7, perm) != want) fail("frame class, row stride 0", code, dtype);
    }
    for (int dtype = 0; dtype < 4; ++dtype) {
        const std::vector<float> inf = {0.25f, HUGE_VALF, 0.25f, HUGE_VALF, -HUGE_VALF};
        if (stored_class(inf, dtype, 5, 1, 1, ident) != 1) fail("the first of two infinities", dtype);
        const std::vector<float> ninf(5, -HUGE_VALF), nan(5, NAN), same(5, 0.5f);
        if (stored_class(ninf, dtype, 5, 1, 0, bonito) != 0 || stored_class(nan, dtype, 5, 1, 0, bonito) != 0) fail("all -inf / all NaN", dtype);
        if (stored_class(same, dtype, 0, 0, 9, mixed) != 0) fail("column stride 0: a tie of five", dtype);
    }
}

// ---- emit
static void check_path(const std::vector<uint8_t>& cls, int kind) {
    const int T = (int)cls.size();
    std::vector<uint8_t> want;
    for (int t = 0; t < T; ++t) {   // the rule, naively
        const uint8_t c = cls[(size_t)t];
        if (c == PO_ACC_BLANK) continue;
        if (kind == PO_ACC_BONITO && t > 0 && cls[(size_t)(t - 1)] == c) continue;
        want.push_back(c);
    }
    std::vector<uint8_t> got(want.size(), 0xff);
    int carry = 0, edge = PO_ACC_NO_PREV;
    for (int t0 = 0; t0 < T; t0 += PO_EV_WAVE) {
        int c[PO_EV_WAVE];
        for (int lane = 0; lane < PO_EV_WAVE; ++lane) c[lane] = t0 + lane < T ? cls[(size_t)(t0 + lane)] : PO_ACC_BLANK;
        uint64_t keep = 0;
        for (int lane = 0; lane < PO_EV_WAVE; ++lane)
            if (po_acc_emit(kind, c[lane], lane == 0 ? edge : c[lane - 1])) keep |= (uint64_t)1 << lane;
        for (int lane = 0; lane < PO_EV_WAVE; ++lane) {
            int pos;
            if (!po_ev_path_slot(keep, lane, carry, &pos)) continue;
            if (pos < 0 || pos >= (int)got.size() || got[(size_t)pos] != 0xff) { fail("path: one writer per code", T, pos); continue; }
            got[(size_t)pos] = (uint8_t)c[lane];
        }
        carry += po_ev_popc(keep);
        edge = c[PO_EV_WAVE - 1];
    }
    if (carry != (int)want.size() || got != want) fail("path", T, kind);
}

static void paths() {
    const uint8_t pick[3] = {0, 3, PO_ACC_BLANK};
    for (int kind = 0; kind < 2; ++kind) {
        for (int T = 0; T <= 7; ++T) {
            int count = 1;
            for (int t = 0; t < T; ++t) count *= 3;
            for (int code = 0; code < count; ++code) {
                std::vector<uint8_t> cls((size_t)T);
                for (int t = 0, k = code; t < T; ++t, k /= 3) cls[(size_t)t] = pick[k % 3];
                check_path(cls, kind);
            }
        }
        const int sizes[7] = {1, 63, 64, 65, 128, 129, 200};
        for (int T : sizes)
            for (int variant = 0; variant < 5; ++variant) {
                std::vector<uint8_t> cls((size_t)T);
                for (int t = 0; t < T; ++t)
                    cls[(size_t)t] = variant == 0 ? PO_ACC_BLANK : variant == 1 ? (uint8_t)(t % 4) : variant == 2 ? (uint8_t)2
                                   : (uint8_t)(rnd() % (variant == 3 ? 5 : 20) % 5);
                check_path(cls, kind);
            }
        // frames 62 .. 66 over {1, blank}, everything else blank: a repeat and a blank-separated repeat across the block's edge
        for (int code = 0; code < 32; ++code) {
            std::vector<uint8_t> cls(130, PO_ACC_BLANK);
            for (int k = 0; k < 5; ++k) if ((code >> k) & 1) cls[(size_t)(62 + k)] = 1;
            check_path(cls, kind);
        }
    }
    if (!po_acc_emit(PO_ACC_BONITO, 2, PO_ACC_NO_PREV) || po_acc_emit(PO_ACC_BONITO, 2, 2) || !po_acc_emit(PO_ACC_POREOVER, 2, 2) ||
        po_acc_emit(PO_ACC_POREOVER, PO_ACC_BLANK, 0) || po_acc_emit(PO_ACC_BONITO, PO_ACC_BLANK, 0))
        fail("emit");
}

// ---- alignment
typedef std::pair<int, int> DM;   // (d, -m): smaller is better, lexicographically

// every alignment of a[i..) against b[j..), one after the other: the best (d, -m) of the rest, no table
static DM enumerate(const std::vector<uint8_t>& a, size_t i, const std::vector<uint8_t>& b, size_t j) {
    if (i == a.size() && j == b.size()) return DM(0, 0);
    DM best(1 << 20, 0);
    if (i < a.size()) { DM r = enumerate(a, i + 1, b, j); r.first += 1; best = std::min(best, r); }
    if (j < b.size()) { DM r = enumerate(a, i, b, j + 1); r.first += 1; best = std::min(best, r); }
    if (i < a.size() && j < b.size()) {
        DM r = enumerate(a, i + 1, b, j + 1);
        if (a[i] == b[j]) r.second -= 1; else r.first += 1;
        best = std::min(best, r);
    }
    return best;
}

static DM lex_row_dp(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    std::vector<DM> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = DM((int)j, 0);
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = DM((int)i, 0);
        for (size_t j = 1; j <= b.size(); ++j) {
            const DM up(prev[j].first + 1, prev[j].second), left(cur[j - 1].first + 1, cur[j - 1].second);
            const DM diag = a[i - 1] == b[j - 1] ? DM(prev[j - 1].first, prev[j - 1].second - 1) : DM(prev[j - 1].first + 1, prev[j - 1].second);
            cur[j] = std::min(std::min(up, left), diag);
        }
        prev.swap(cur);
    }
    return prev[b.size()];
}

static DM decode(int32_t key) { return DM(po_acc_distance(key), -po_acc_matches(key)); }

static DM key_row_dp(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    std::vector<int32_t> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int32_t)j * PO_ACC_BASE;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int32_t)i * PO_ACC_BASE;
        for (size_t j = 1; j <= b.size(); ++j) cur[j] = po_acc_cell(prev[j], cur[j - 1], prev[j - 1], a[i - 1] != b[j - 1]);
        prev.swap(cur);
    }
    return decode(prev[b.size()]);
}

// the kernel's stats_wave<K>, the 64 lanes one after the other
template <int K>
static int32_t wave_walk(const std::vector<uint8_t>& lo, const std::vector<uint8_t>& sh) {
    const int S = (int)sh.size(), L = (int)lo.size();
    struct Lane { int32_t row[K]; uint32_t sym[(K + 3) / 4]; int32_t diag; };
    std::vector<Lane> lanes(PO_EV_WAVE);
    std::vector<int32_t> total(PO_EV_WAVE), excl(PO_EV_WAVE);
    for (int l = 0; l < PO_EV_WAVE; ++l) {
        po_ev_load_symbols<K>(lanes[(size_t)l].sym, sh.data(), S, l);
        po_acc_row_init<K>(lanes[(size_t)l].row, l);
        lanes[(size_t)l].diag = po_acc_diag_init<K>(l);
    }
    for (int i = 1; i <= L; ++i) {
        for (int l = 0; l < PO_EV_WAVE; ++l)
            total[(size_t)l] = po_acc_row_local<K>(lanes[(size_t)l].row, lanes[(size_t)l].sym, lanes[(size_t)l].diag, lo[(size_t)(i - 1)], i, l);
        po_ev_wave_excl_min(total.data(), excl.data());
        for (int l = 0; l < PO_EV_WAVE; ++l) lanes[(size_t)l].diag = po_acc_row_finish<K>(lanes[(size_t)l].row, excl[(size_t)l], l);
    }
    return po_ev_row_pick<K>(lanes[(size_t)(S / K)].row, S);
}

// (d, -m) as the kernel takes it: the shorter string on the lanes, in instantiation K (0: the one the kernel chooses)
static DM wave_stats(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int K) {
    const bool a_short = a.size() <= b.size();
    const std::vector<uint8_t>& sh = a_short ? a : b;
    const std::vector<uint8_t>& lo = a_short ? b : a;
    if (K == 0) K = po_ev_slot_class(po_ev_slots((int)sh.size()));
    switch (K) {
        case 1: return decode(wave_walk<1>(lo, sh));
        case 2: return decode(wave_walk<2>(lo, sh));
        case 4: return decode(wave_walk<4>(lo, sh));
        case 8: return decode(wave_walk<8>(lo, sh));
        case 16: return decode(wave_walk<16>(lo, sh));
        case 32: return decode(wave_walk<32>(lo, sh));
        default: return decode(wave_walk<PO_EV_MAX_SLOTS>(lo, sh));
    }
}

static std::vector<uint8_t> random_string(int n, int alphabet) {
    std::vector<uint8_t> s((size_t)n);
    for (auto& c : s) c = (uint8_t)(rnd() % (uint32_t)alphabet);
    return s;
}

static void align() {
    // every pair over 3 symbols up to 4 symbols a side
    int pairs = 0;
    for (int la = 0; la <= 4; ++la)
        for (int lb = 0; lb <= 4; ++lb) {
            int na = 1, nb = 1;
            for (int i = 0; i < la; ++i) na *= 3;
            for (int j = 0; j < lb; ++j) nb *= 3;
            for (int ca = 0; ca < na; ++ca)
                for (int cb = 0; cb < nb; ++cb, ++pairs) {
                    std::vector<uint8_t> a((size_t)la), b((size_t)lb);
                    for (int i = 0, k = ca; i < la; ++i, k /= 3) a[(size_t)i] = (uint8_t)("ACG"[k % 3]);
                    for (int j = 0, k = cb; j < lb; ++j, k /= 3) b[(size_t)j] = (uint8_t)("ACG"[k % 3]);
                    const DM want = enumerate(a, 0, b, 0);
                    if (lex_row_dp(a, b) != want) fail("lexicographic row DP against the enumeration", la, lb, ca);
                    if (key_row_dp(a, b) != want) fail("packed-key row DP against the enumeration", la, lb, ca);
                    if (wave_stats(a, b, 0) != want) fail("wave against the enumeration", la, lb, ca);
                    // (a wider instantiation on one pair in 16: all of them on all pairs would take minutes under the sanitizers)
                    if ((ca * 7 + cb) % 16 == 0 && wave_stats(a, b, 2 << ((ca + cb + lb) % 6)) != want) fail("wide wave against the enumeration", la, lb, ca);
                }
        }
    if (pairs != 121 * 121) fail("the enumeration's pairs", pairs);
    {   // "AB" / "BA": two edits either way, and the alignment with a match is taken
        const std::vector<uint8_t> ab = {'A', 'B'}, ba = {'B', 'A'};
        if (wave_stats(ab, ba, 0) != DM(2, -1) || enumerate(ab, 0, ba, 0) != DM(2, -1)) fail("AB / BA");
    }
    // random strings up to a few hundred symbols: 4 symbols (reads), 2 (long runs of matches), 250 (nothing in common)
    for (int it = 0; it < 60; ++it) {
        const int alphabet = it % 3 == 0 ? 4 : it % 3 == 1 ? 2 : 250;
        const std::vector<uint8_t> a = random_string((int)(rnd() % 400), alphabet), b = random_string((int)(rnd() % 400), alphabet);
        const DM want = lex_row_dp(a, b);
        if (wave_stats(a, b, 0) != want || wave_stats(b, a, 0) != want) fail("wave against the row DP", (long)a.size(), (long)b.size());
        if (key_row_dp(a, b) != want) fail("packed-key row DP against the lexicographic one", (long)a.size(), (long)b.size());
        if (wave_stats(a, a, 0) != DM(0, -(int)a.size())) fail("equal strings", (long)a.size());
    }
    // noisy copies: reads against their truth
    for (int it = 0; it < 20; ++it) {
        const std::vector<uint8_t> b = random_string(20 + (int)(rnd() % 300), 4);
        std::vector<uint8_t> a;
        for (uint8_t c : b) {
            const uint32_t r = rnd() % 20;
            if (r == 0) continue;
            if (r == 1) a.push_back((uint8_t)(rnd() % 4));
            a.push_back(r == 2 ? (uint8_t)(rnd() % 4) : c);
        }
        if (wave_stats(a, b, 0) != lex_row_dp(a, b)) fail("wave on a noisy copy", (long)a.size(), (long)b.size());
    }
    // the widths' edges: S + 1 columns fill K lanes' worth exactly, one less, one more
    const int edges[] = {62, 63, 64, 65, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, PO_EDIT_MAX_SHORT};
    for (int S : edges) {
        const std::vector<uint8_t> sh = random_string(S, 4), lo = random_string(S > 1000 ? 70 : 300, 4);
        const DM want = lex_row_dp(lo, sh);
        if (wave_stats(lo, sh, 0) != want) fail("wave at a width's edge", S);
        if (S <= 512 && wave_stats(lo, sh, PO_EV_MAX_SLOTS) != want) fail("widest instantiation", S);
    }
    {   // nothing in common, and an empty side
        const std::vector<uint8_t> a(100, 'A'), b(37, 'C'), none;
        if (wave_stats(a, b, 0) != DM(100, 0) || wave_stats(b, a, 0) != DM(100, 0)) fail("no symbol in common");
        if (wave_stats(a, none, 0) != DM(100, 0) || wave_stats(none, b, 0) != DM(37, 0) || wave_stats(none, none, 0) != DM(0, 0)) fail("empty side");
    }
    // the decode at the key's ends: the most matches at no distance, the longest pair with nothing in common
    if (decode(-PO_EDIT_MAX_SHORT) != DM(0, -PO_EDIT_MAX_SHORT) || decode(PO_ACC_BASE - PO_EDIT_MAX_SHORT) != DM(1, -PO_EDIT_MAX_SHORT)) fail("decode");
    if (decode(PO_ACC_MAX_LONG * PO_ACC_BASE) != DM(PO_ACC_MAX_LONG, 0) || (int64_t)(PO_ACC_MAX_LONG + 1) * PO_ACC_BASE >= PO_EV_INF) fail("cap");
}

int main() {
    widen();
    argmax();
    paths();
    align();
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
