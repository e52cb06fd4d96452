// The per-element rules of `train`'s held-out validation (poreover_amd/csrc/po_eval_rules.h), the part of the feature that
// needs no device: the same source the kernels of po_eval.hip run.  Plain C++, no HIP: built and run under
// -fsanitize=address,undefined by tests/test_train_eval_cpu.py.  Exit status 0 and "ok" when every case holds.
//   argmax   against a restatement of np.argmax (NaN is the largest value, the first of equals wins) on every frame whose
//            five values come from {-1, 0, 0.5, 0.5 again, NaN}: ties of two to five classes, NaN before and after the maximum
//   path     the kernel's loop (blocks of 64 frames, one ballot, one carried count) against a frame-by-frame filter, for
//            every class pattern of up to 7 frames over {0, 3, 4} and for windows of 1, 63, 64, 65 and 200 frames
//   edit     the wave's walk (64 lanes, K columns each, the local pass, the exclusive prefix minimum as the kernel's moves
//            make it, the second pass, the pick) in every instantiation that can hold the pair, both ways round: against
//            the recursion on the cell rule for pairs over {A, C} up to 8 symbols (the row DP on every such pair), and
//            against the plain row DP for random strings up to a few hundred symbols and at the widths' edges (63, 64, 127, 128, ... 4095 columns)
// Every array sits in a heap block of exactly its size.
#include "../poreover_amd/csrc/po_eval_rules.h"

#include <cmath>
#include <cstdio>
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

// ---- argmax
static int numpy_argmax(const std::vector<float>& p) {
    for (size_t c = 0; c < p.size(); ++c)
        if (std::isnan(p[c])) return (int)c;
    size_t best = 0;
    for (size_t c = 1; c < p.size(); ++c)
        if (p[c] > p[best]) best = c;
    return (int)best;
}

static void argmax() {
    const float vals[5] = {-1.f, 0.f, 0.5f, 0.5f, NAN};
    for (int code = 0; code < 5 * 5 * 5 * 5 * 5; ++code) {
        std::vector<float> p(PO_EV_CLASSES);
        for (int c = 0, k = code; c < PO_EV_CLASSES; ++c, k /= 5) p[(size_t)c] = vals[k % 5];
        if (po_ev_argmax(p.data()) != numpy_argmax(p)) fail("argmax", code);
    }
    const std::vector<float> inf = {0.25f, HUGE_VALF, 0.25f, HUGE_VALF, -HUGE_VALF};
    if (po_ev_argmax(inf.data()) != 1) fail("argmax: the first of two infinities");
}

// ---- path
static void check_path(const std::vector<uint8_t>& cls) {
    const int T = (int)cls.size();
    std::vector<uint8_t> want;
    for (int t = 0; t < T; ++t)
        if (cls[(size_t)t] != PO_EV_BLANK) want.push_back(cls[(size_t)t]);
    std::vector<uint8_t> got(want.size(), 0xff);
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += PO_EV_WAVE) {
        uint64_t keep = 0;
        for (int lane = 0; lane < PO_EV_WAVE && t0 + lane < T; ++lane)
            if (cls[(size_t)(t0 + lane)] != PO_EV_BLANK) keep |= (uint64_t)1 << lane;
        for (int lane = 0; lane < PO_EV_WAVE; ++lane) {
            int pos;
            if (!po_ev_path_slot(keep, lane, carry, &pos)) continue;
            if (pos < 0 || pos >= (int)got.size() || got[(size_t)pos] != 0xff) { fail("path: one writer per code", T, pos); continue; }
            got[(size_t)pos] = cls[(size_t)(t0 + lane)];
        }
        carry += po_ev_popc(keep);
    }
    if (carry != (int)want.size() || got != want) fail("path", T);
}

static void paths() {
    const uint8_t pick[3] = {0, 3, PO_EV_BLANK};
    for (int T = 1; T <= 7; ++T) {
        int count = 1;
        for (int t = 0; t < T; ++t) count *= 3;
        for (int code = 0; code < count; ++code) {
            std::vector<uint8_t> cls((size_t)T);
            for (int t = 0, k = code; t < T; ++t, k /= 3) cls[(size_t)t] = pick[k % 3];
            check_path(cls);
        }
    }
    const int sizes[5] = {1, 63, 64, 65, 200};
    for (int T : sizes)
        for (int variant = 0; variant < 4; ++variant) {
            std::vector<uint8_t> cls((size_t)T);
            for (int t = 0; t < T; ++t)
                cls[(size_t)t] = variant == 0 ? PO_EV_BLANK : variant == 1 ? (uint8_t)(t % 4) : (uint8_t)(rnd() % (variant == 2 ? 5 : 20) % 5);
            check_path(cls);
        }
}

// ---- edit distance
// the definition, top down (each cell remembered: the bare recursion takes 10^6 calls for one pair of 8 and 8 symbols)
static int32_t recurse(const std::vector<uint8_t>& a, size_t i, const std::vector<uint8_t>& b, size_t j, std::vector<int32_t>& memo) {
    if (i == 0) return (int32_t)j;
    if (j == 0) return (int32_t)i;
    int32_t& m = memo[i * (b.size() + 1) + j];
    if (m < 0)
        m = po_ev_cell(recurse(a, i - 1, b, j, memo), recurse(a, i, b, j - 1, memo), recurse(a, i - 1, b, j - 1, memo), a[i - 1] != b[j - 1]);
    return m;
}

static int32_t row_dp(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    std::vector<int32_t> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int32_t)j;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int32_t)i;
        for (size_t j = 1; j <= b.size(); ++j) cur[j] = po_ev_cell(prev[j], cur[j - 1], prev[j - 1], a[i - 1] != b[j - 1]);
        prev.swap(cur);
    }
    return prev[b.size()];
}

// the kernel's edit_wave<K>, the 64 lanes one after the other
template <int K>
static int32_t wave_walk(const std::vector<uint8_t>& lo, const std::vector<uint8_t>& sh) {
    const int S = (int)sh.size(), L = (int)lo.size();
    struct Lane { int32_t row[K]; uint32_t sym[(K + 3) / 4]; int32_t diag; };
    std::vector<Lane> lanes(PO_EV_WAVE);
    std::vector<int32_t> total(PO_EV_WAVE), excl(PO_EV_WAVE);
    for (int l = 0; l < PO_EV_WAVE; ++l) {
        po_ev_load_symbols<K>(lanes[(size_t)l].sym, sh.data(), S, l);
        po_ev_row_init<K>(lanes[(size_t)l].row, l);
        lanes[(size_t)l].diag = l * K - 1;
    }
    for (int i = 1; i <= L; ++i) {
        for (int l = 0; l < PO_EV_WAVE; ++l)
            total[(size_t)l] = po_ev_row_local<K>(lanes[(size_t)l].row, lanes[(size_t)l].sym, lanes[(size_t)l].diag, lo[(size_t)(i - 1)], i, l);
        po_ev_wave_excl_min(total.data(), excl.data());
        for (int l = 0; l < PO_EV_WAVE; ++l) lanes[(size_t)l].diag = po_ev_row_finish<K>(lanes[(size_t)l].row, excl[(size_t)l], l);
    }
    return po_ev_row_pick<K>(lanes[(size_t)(S / K)].row, S);
}

// the distance as the kernel takes it: the shorter string on the lanes, in instantiation K (0: the one the kernel chooses)
static int32_t wave_distance(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int K) {
    const bool a_short = a.size() <= b.size();
    const std::vector<uint8_t>& sh = a_short ? a : b;
    const std::vector<uint8_t>& lo = a_short ? b : a;
    if (K == 0) K = po_ev_slot_class(po_ev_slots((int)sh.size()));
    switch (K) {
        case 1: return wave_walk<1>(lo, sh);
        case 2: return wave_walk<2>(lo, sh);
        case 4: return wave_walk<4>(lo, sh);
        case 8: return wave_walk<8>(lo, sh);
        case 16: return wave_walk<16>(lo, sh);
        case 32: return wave_walk<32>(lo, sh);
        default: return wave_walk<PO_EV_MAX_SLOTS>(lo, sh);
    }
}

static std::vector<uint8_t> random_string(int n, int alphabet) {
    std::vector<uint8_t> s((size_t)n);
    for (auto& c : s) c = (uint8_t)(rnd() % (uint32_t)alphabet);
    return s;
}

static void edit() {
    // every pair over {A, C} up to 8 symbols (la <= lb: the walk is tried both ways round)
    for (int la = 0; la <= 8; ++la)
        for (int lb = la; lb <= 8; ++lb)
            for (unsigned ca = 0; ca < (1u << la); ++ca)
                for (unsigned cb = 0; cb < (1u << lb); ++cb) {
                    std::vector<uint8_t> a((size_t)la), b((size_t)lb);
                    for (int i = 0; i < la; ++i) a[(size_t)i] = (ca >> i) & 1 ? 'C' : 'A';
                    for (int j = 0; j < lb; ++j) b[(size_t)j] = (cb >> j) & 1 ? 'C' : 'A';
                    std::vector<int32_t> memo((size_t)(la + 1) * (size_t)(lb + 1), -1);
                    const int32_t want = recurse(a, a.size(), b, b.size(), memo);
                    if (row_dp(a, b) != want || row_dp(b, a) != want) fail("row DP against the recursion", la, lb, (long)ca);
                    // (the wave's walk on every pair up to 6 symbols and on one longer pair in 16, there in a wider instantiation
                    // too: all of them on all pairs would take minutes under the sanitizers)
                    if (lb > 6 && (ca * 7 + cb) % 16 != 0) continue;
                    if (wave_distance(a, b, 0) != want || wave_distance(b, a, 0) != want) fail("wave against the recursion", la, lb, 0);
                    const int K = 2 << ((ca + cb + (unsigned)lb) % 6);
                    if (lb > 6 && wave_distance(a, b, K) != want) fail("wave against the recursion", la, lb, K);
                }
    if (po_ev_slots(0) != 1 || po_ev_slots(63) != 1 || po_ev_slots(64) != 2 || po_ev_slots(PO_EDIT_MAX_SHORT) != PO_EV_MAX_SLOTS)
        fail("slots");
    if (po_ev_slot_class(1) != 1 || po_ev_slot_class(3) != 4 || po_ev_slot_class(33) != 64 || po_ev_slot_class(64) != 64) fail("slot class");
    // random strings up to a few hundred symbols: 4 symbols (reads), 2 (long runs of matches), 250 (nothing in common)
    for (int it = 0; it < 60; ++it) {
        const int alphabet = it % 3 == 0 ? 4 : it % 3 == 1 ? 2 : 250;
        const std::vector<uint8_t> a = random_string((int)(rnd() % 400), alphabet), b = random_string((int)(rnd() % 400), alphabet);
        const int32_t want = row_dp(a, b);
        if (wave_distance(a, b, 0) != want || wave_distance(b, a, 0) != want) fail("wave against the row DP", (long)a.size(), (long)b.size());
        if (wave_distance(a, a, 0) != 0) fail("equal strings", (long)a.size());
    }
    // the widths' edges: S + 1 columns fill K lanes' worth exactly, one less, one more
    const int edges[] = {62, 63, 64, 65, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, PO_EDIT_MAX_SHORT};
    for (int S : edges) {
        const std::vector<uint8_t> sh = random_string(S, 4), lo = random_string(S > 1000 ? 70 : 300, 4);
        const int32_t want = row_dp(lo, sh);
        if (wave_distance(lo, sh, 0) != want) fail("wave at a width's edge", S);
        if (S <= 512 && wave_distance(lo, sh, PO_EV_MAX_SLOTS) != want) fail("widest instantiation", S);
    }
    {   // nothing in common, and an empty side
        const std::vector<uint8_t> a(100, 'A'), b(37, 'C'), none;
        if (wave_distance(a, b, 0) != 100 || wave_distance(b, a, 0) != 100) fail("no symbol in common");
        if (wave_distance(a, none, 0) != 100 || wave_distance(none, b, 0) != 37 || wave_distance(none, none, 0) != 0) fail("empty side");
    }
}

int main() {
    argmax();
    paths();
    edit();
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
