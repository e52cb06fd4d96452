// The per-element rules of tensors.edit_alignment (poreover_amd/csrc/po_aln_rules.h), the part of the feature that needs no
// device: the same source the kernels of po_aln.hip run.  Plain C++, no HIP: built and run under -fsanitize=address,undefined
// by tests/test_tensors_alignment_cpu.py.  Exit status 0 and "ok" when every case holds.
//   naive    the full key table D (rows the hypothesis, columns the truth) and the walk by the three rules, as the header states
//            them; its ops replayed against the two strings
//   wave     edit_align_kernel and edit_walk_kernel restated lane by lane: po_aln_row_local, the exclusive prefix minimum as the
//            kernel's moves make it, po_aln_row_finish, the packing of each row's ops into the trace as the kernel stores them,
//            then the walk over blocks of two words a lane, re-fetched where a cell lies outside.  Every pair with la, lb <= 4
//            over 3 symbols in every instantiation K = 1 .. 64 and with either string on the lanes: ops == the naive walk's,
//            count(=) == m and length == m + d of po_acc_rules.h's key.  (A lane's values depend on the lanes to its left
//            alone, so these small cases compute the lanes up to the one past column S; the cases below compute all 64 and
//            check that every word of the trace is stored exactly once.)
//   random   random and noisy pairs up to 400 symbols in the kernel's own instantiation and a wider one, both ways round, and
//            strings at the slot classes' edges
//   packing  word and bit of every cell of a few shapes per K: inside po_aln_words, no two cells on the same bits, lane and
//            word edges as the kernel's stores place them
//   room     po_aln_trace_words non-decreasing in both arguments on a grid that crosses every slot-class edge and the caps
//   cells    the confusion cell of each op, bytes above 3 included
// Every array sits in a heap block of exactly its size.
#include "../poreover_amd/csrc/po_aln_rules.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Str;

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

// ---- naive: the header's words
static Str naive_ops(const Str& a, const Str& b, int32_t* key) {
    const size_t la = a.size(), lb = b.size();
    std::vector<int64_t> D((la + 1) * (lb + 1));
    auto at = [&](size_t i, size_t j) -> int64_t& { return D[i * (lb + 1) + j]; };
    for (size_t j = 0; j <= lb; ++j) at(0, j) = 4096 * (int64_t)j;
    for (size_t i = 1; i <= la; ++i) {
        at(i, 0) = 4096 * (int64_t)i;
        for (size_t j = 1; j <= lb; ++j)
            at(i, j) = std::min(std::min(at(i - 1, j) + 4096, at(i, j - 1) + 4096), at(i - 1, j - 1) + (a[i - 1] != b[j - 1] ? 4096 : -1));
    }
    Str ops;
    size_t i = la, j = lb;
    while (i || j) {
        if (i && j && at(i, j) == at(i - 1, j - 1) + (a[i - 1] != b[j - 1] ? 4096 : -1)) { ops.push_back(a[i - 1] != b[j - 1] ? PO_ALN_X : PO_ALN_EQ); --i; --j; }
        else if (i && at(i, j) == at(i - 1, j) + 4096) { ops.push_back(PO_ALN_I); --i; }
        else {
            if (!j || at(i, j) != at(i, j - 1) + 4096) fail("naive walk: no predecessor achieves the cell", (long)i, (long)j);
            ops.push_back(PO_ALN_D);
            --j;
        }
    }
    std::reverse(ops.begin(), ops.end());
    *key = (int32_t)at(la, lb);
    return ops;
}

static bool replay(const Str& ops, const Str& a, const Str& b) {
    size_t i = 0, j = 0;
    for (uint8_t c : ops) {
        if (c <= PO_ALN_X) {
            if (i >= a.size() || j >= b.size() || (a[i] == b[j]) != (c == PO_ALN_EQ)) return false;
            ++i; ++j;
        } else if (c == PO_ALN_I) { if (i++ >= a.size()) return false; }
        else if (c == PO_ALN_D) { if (j++ >= b.size()) return false; }
        else return false;
    }
    return i == a.size() && j == b.size();
}

// ---- the two kernels, the lanes one after the other.  lanes: how many of the 64 are computed (those to the right feed nothing
// to the left); refetches: how often the walk fetched its block
template <int K>
static Str wave_ops(const Str& hyp, const Str& truth, bool cols_hyp, int lanes, int32_t* key, int* refetches) {
    constexpr int W = (K + 15) / 16, R = K < 16 ? 16 / K : 1;
    const Str& sh = cols_hyp ? hyp : truth;
    const Str& lo = cols_hyp ? truth : hyp;
    const int S = (int)sh.size(), L = (int)lo.size();
    const uint32_t tie_left = cols_hyp ? ~0u : 0u;
    struct Lane { int32_t row[K]; uint32_t sym[(K + 3) / 4]; uint32_t st[W], code[W]; int32_t diag; uint32_t acc; };
    std::vector<Lane> ln((size_t)lanes);
    std::vector<int32_t> total(PO_EV_WAVE, PO_EV_INF), excl(PO_EV_WAVE);
    std::vector<uint32_t> tr((size_t)po_aln_words(K, L), 0u);
    std::vector<uint8_t> stored(tr.size(), 0);
    auto store = [&](int64_t at, uint32_t v) {
        if (at < 0 || at >= (int64_t)tr.size()) { fail("a store outside the trace", K, (long)at, (long)tr.size()); return; }
        if (stored[(size_t)at]++) fail("a word stored twice", K, (long)at);
        tr[(size_t)at] = v;
    };
    for (int l = 0; l < lanes; ++l) {
        po_ev_load_symbols<K>(ln[(size_t)l].sym, sh.data(), S, l);
        po_acc_row_init<K>(ln[(size_t)l].row, l);
        ln[(size_t)l].diag = po_acc_diag_init<K>(l);
        ln[(size_t)l].acc = 0;
    }
    for (int i = 1; i <= L; ++i) {
        const int x = lo[(size_t)(i - 1)];
        for (int l = 0; l < lanes; ++l) total[(size_t)l] = po_aln_row_local<K>(ln[(size_t)l].row, ln[(size_t)l].st, ln[(size_t)l].sym, ln[(size_t)l].diag, x, i, tie_left, l);
        po_ev_wave_excl_min(total.data(), excl.data());
        for (int l = 0; l < lanes; ++l) {
            Lane& n = ln[(size_t)l];
            n.diag = po_aln_row_finish<K>(n.row, n.code, n.st, excl[(size_t)l], tie_left, l);
            if (K >= 16) {
                for (int q = 0; q < W; ++q) store(((int64_t)(i - 1) * PO_EV_WAVE + l) * W + q, n.code[q]);
            } else {
                const int sub = (i - 1) & (R - 1);
                n.acc |= (n.code[0] & (uint32_t)((1ull << (2 * K)) - 1)) << (sub * 2 * K);
                if (sub == R - 1 || i == L) { store((int64_t)((i - 1) / R) * PO_EV_WAVE + l, n.acc); n.acc = 0; }
            }
        }
    }
    if (lanes == PO_EV_WAVE)
        for (size_t q = 0; q < stored.size(); ++q)
            if (stored[q] != 1) { fail("a word of the trace is not stored", K, (long)q); break; }
    if (S / K >= lanes) { fail("the lane of column S is not computed", K, S, lanes); return Str(); }
    *key = po_ev_row_pick<K>(ln[(size_t)(S / K)].row, S);
    // edit_walk_kernel
    const po_aln_geom gm = po_aln_geometry(K);
    int pos = po_acc_matches(*key) + po_acc_distance(*key);
    Str ops((size_t)pos, 0xee);
    int i = L, j = S, i0 = 0, j0 = 0;
    std::vector<uint32_t> w0(PO_EV_WAVE, 0), w1(PO_EV_WAVE, 0);
    *refetches = 0;
    while (pos > 0) {
        const int cnt = pos < PO_EV_WAVE ? pos : PO_EV_WAVE;
        for (int q = 0; q < cnt; ++q) {
            uint32_t code;
            if (i <= 0) code = PO_ALN_DIR_LEFT;
            else if (j <= 0) code = PO_ALN_DIR_UP;
            else {
                int lane = 0, which = 0, bit = 0;
                if (i0 == 0 || !po_aln_block_find(gm, i0, j0, i, j, &lane, &which, &bit)) {
                    i0 = i; j0 = j;
                    ++*refetches;
                    for (int l = 0; l < PO_EV_WAVE; ++l) {
                        const int64_t at = po_aln_block_word(gm, i0, j0, l);
                        if (at >= 0 && at + 1 >= (int64_t)tr.size()) { fail("a block word outside the trace", K, (long)at, (long)tr.size()); return Str(); }
                        w0[(size_t)l] = at >= 0 ? tr[(size_t)at] : 0;
                        w1[(size_t)l] = at >= 0 ? tr[(size_t)at + 1] : 0;
                    }
                    if (!po_aln_block_find(gm, i0, j0, i, j, &lane, &which, &bit)) { fail("the anchor lies outside its block", K, i, j); return Str(); }
                }
                if (lane < 0 || lane >= PO_EV_WAVE || bit < 0 || bit > 30) { fail("lane or bit", K, lane, bit); return Str(); }
                code = ((which ? w1[(size_t)lane] : w0[(size_t)lane]) >> bit) & 3u;
                const int64_t direct = po_aln_word(gm, i, j);
                if (((tr[(size_t)direct] >> bit) & 3u) != code) fail("the block's word is not the cell's", K, i, j);
            }
            po_aln_step(code, &i, &j);
            ops[(size_t)(pos - 1 - q)] = (uint8_t)po_aln_op(code, cols_hyp);
        }
        pos -= cnt;
    }
    if (i != 0 || j != 0) fail("the walk does not end at (0, 0)", K, i, j);
    return ops;
}

static Str wave_any(int K, const Str& hyp, const Str& truth, bool cols_hyp, int lanes, int32_t* key, int* refetches) {
    switch (K) {
        case 1: return wave_ops<1>(hyp, truth, cols_hyp, lanes, key, refetches);
        case 2: return wave_ops<2>(hyp, truth, cols_hyp, lanes, key, refetches);
        case 4: return wave_ops<4>(hyp, truth, cols_hyp, lanes, key, refetches);
        case 8: return wave_ops<8>(hyp, truth, cols_hyp, lanes, key, refetches);
        case 16: return wave_ops<16>(hyp, truth, cols_hyp, lanes, key, refetches);
        case 32: return wave_ops<32>(hyp, truth, cols_hyp, lanes, key, refetches);
        default: return wave_ops<PO_EV_MAX_SLOTS>(hyp, truth, cols_hyp, lanes, key, refetches);
    }
}

// the packed-key row DP of po_acc_rules.h's cell
static int32_t key_row_dp(const Str& a, const Str& b) {
    std::vector<int32_t> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int32_t)j * PO_ACC_BASE;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int32_t)i * PO_ACC_BASE;
        for (size_t j = 1; j <= b.size(); ++j) cur[j] = po_acc_cell(prev[j], cur[j - 1], prev[j - 1], a[i - 1] != b[j - 1]);
        prev.swap(cur);
    }
    return prev[b.size()];
}

static long total_refetches = 0, total_columns = 0;

// one pair in instantiation K with the given string on the lanes, against the naive walk
static void check(const Str& a, const Str& b, int K, bool cols_hyp, int lanes, const Str& want, int32_t want_key) {
    int32_t key = 0;
    int refetches = 0;
    const Str got = wave_any(K, a, b, cols_hyp, lanes, &key, &refetches);
    total_refetches += refetches;
    total_columns += (long)got.size();
    if (key != want_key) fail("the wave's key", K, (long)a.size(), (long)b.size());
    if (got != want) fail("the wave's ops", K, (long)a.size(), (long)b.size());
}

static void verify_naive(const Str& a, const Str& b, const Str& ops, int32_t key) {
    const int d = po_acc_distance(key), m = po_acc_matches(key);
    if (key != key_row_dp(a, b)) fail("the naive table's key is po_acc_cell's", (long)a.size(), (long)b.size());
    if (!replay(ops, a, b)) fail("replay", (long)a.size(), (long)b.size());
    if ((int)std::count(ops.begin(), ops.end(), (uint8_t)PO_ALN_EQ) != m) fail("count(=) == m", (long)a.size(), (long)b.size(), m);
    if ((int)ops.size() != m + d) fail("length == m + d", (long)a.size(), (long)b.size(), m + d);
}

static Str random_string(int n, int alphabet) {
    Str s((size_t)n);
    for (auto& c : s) c = (uint8_t)(rnd() % (uint32_t)alphabet);
    return s;
}

static Str noisy_copy(const Str& b) {
    Str a;
    for (uint8_t c : b) {
        const uint32_t r = rnd() % 10;
        if (r == 0) continue;
        if (r == 1) a.push_back((uint8_t)(rnd() % 4));
        a.push_back(r == 2 ? (uint8_t)(rnd() % 4) : c);
    }
    return a;
}

static Str text(const char* s) {
    Str v;
    for (; *s; ++s) v.push_back((uint8_t)*s);
    return v;
}

static void named(const char* a, const char* b, const char* want) {
    int32_t key = 0;
    const Str ops = naive_ops(text(a), text(b), &key);
    std::string got;
    for (uint8_t c : ops) got.push_back("=XID"[c]);
    if (got != want) fail(want, (long)got.size());
}

static int natural_k(size_t S) { return po_ev_slot_class(po_ev_slots((int)S)); }

static void small() {
    const int Ks[7] = {1, 2, 4, 8, 16, 32, 64};
    int pairs = 0;
    for (int la = 0; la <= 4; ++la)
        for (int lb = 0; lb <= 4; ++lb) {
            int na = 1, nb = 1;
            for (int i = 0; i < la; ++i) na *= 3;
            for (int j = 0; j < lb; ++j) nb *= 3;
            for (int ca = 0; ca < na; ++ca)
                for (int cb = 0; cb < nb; ++cb, ++pairs) {
                    Str a((size_t)la), b((size_t)lb);
                    for (int i = 0, k = ca; i < la; ++i, k /= 3) a[(size_t)i] = (uint8_t)(k % 3);
                    for (int j = 0, k = cb; j < lb; ++j, k /= 3) b[(size_t)j] = (uint8_t)(k % 3);
                    int32_t key = 0;
                    const Str want = naive_ops(a, b, &key);
                    verify_naive(a, b, want, key);
                    for (int K : Ks)
                        for (int cols_hyp = 0; cols_hyp < 2; ++cols_hyp) {
                            const int S = cols_hyp ? la : lb;
                            check(a, b, K, cols_hyp != 0, S / K + 2, want, key);
                        }
                }
        }
    if (pairs != 121 * 121) fail("the enumeration's pairs", pairs);
    named("AB", "BA", "D=I");
    named("AAAA", "AAA", "I===");
    named("AAA", "AAAA", "D===");
    named("ACGT", "AGT", "=I==");
    named("", "AC", "DD");
    named("AC", "", "II");
}

static void both_ways(const Str& a, const Str& b, bool wider) {
    int32_t key = 0;
    const Str want = naive_ops(a, b, &key);
    verify_naive(a, b, want, key);
    const bool cols_hyp = a.size() <= b.size();           // the kernel's choice
    const int K = natural_k(std::min(a.size(), b.size()));
    check(a, b, K, cols_hyp, PO_EV_WAVE, want, key);
    if (wider) {
        if (K < 64) check(a, b, 2 * K, cols_hyp, PO_EV_WAVE, want, key);
        check(a, b, natural_k(std::max(a.size(), b.size())), !cols_hyp, PO_EV_WAVE, want, key);   // the longer string on the lanes
    }
}

static void random_pairs() {
    for (int it = 0; it < 36; ++it) {
        const int alphabet = it % 3 == 0 ? 4 : it % 3 == 1 ? 2 : 250;
        const Str a = random_string((int)(rnd() % 400), alphabet), b = random_string((int)(rnd() % 400), alphabet);
        both_ways(a, b, it % 4 == 0);
        both_ways(b, a, false);
    }
    for (int it = 0; it < 24; ++it) {
        const Str b = random_string(20 + (int)(rnd() % 380), 4), a = noisy_copy(b);
        both_ways(a, b, it % 4 == 0);
        both_ways(b, a, false);
    }
    {   // equal strings, nothing in common, an empty side, homopolymers
        const Str a = random_string(130, 4), ac(100, 0), gt(37, 2), none, run(90, 1), shorter(83, 1);
        both_ways(a, a, true);
        both_ways(ac, gt, true);
        both_ways(gt, ac, false);
        both_ways(ac, none, false);
        both_ways(none, gt, false);
        both_ways(none, none, false);
        both_ways(run, shorter, true);
        both_ways(shorter, run, true);
    }
    // the slot classes' edges: S + 1 columns fill K lanes' worth exactly, or need the next instantiation
    const int edges[] = {62, 63, 64, 65, 127, 128, 255, 256, 511, 512, 1023, 1024};
    for (int S : edges) {
        const Str sh = random_string(S, 4);
        Str lo = noisy_copy(sh);
        if (S > 300) lo.resize(70);
        both_ways(sh, lo, false);
        both_ways(lo, sh, false);
    }
}

static void packing() {
    const int Ks[7] = {1, 2, 4, 8, 16, 32, 64};
    for (int K : Ks) {
        const po_aln_geom g = po_aln_geometry(K);
        const int U = K < 16 ? K : 16, R = 16 / U;
        if ((1 << g.ush) != U || (1 << g.rsh) != R || g.gw != PO_EV_WAVE * K / U) fail("geometry", K);
        const int Ls[5] = {1, 15, 16, 17, 33};
        for (int L : Ls) {
            const int64_t words = po_aln_words(K, L);
            if (words != (int64_t)((L + R - 1) / R) * g.gw) fail("po_aln_words", K, L);
            std::vector<uint32_t> seen((size_t)words, 0u);
            for (int i = 1; i <= L; ++i)
                for (int j = 0; j < PO_EV_WAVE * K; ++j) {
                    const int64_t w = po_aln_word(g, i, j);
                    const int bit = po_aln_bit(g, i, j);
                    if (w < 0 || w >= words || bit < 0 || bit > 30 || (bit & 1)) { fail("word or bit outside", K, i, j); continue; }
                    if (seen[(size_t)w] & (3u << bit)) fail("two cells on the same bits", K, i, j);
                    seen[(size_t)w] |= 3u << bit;
                    // as the kernel stores it: lane j / K, column k = j % K of the lane
                    const int lane = j / K, k = j % K;
                    const int64_t kw = K >= 16 ? ((int64_t)(i - 1) * PO_EV_WAVE + lane) * (K / 16) + k / 16 : (int64_t)((i - 1) / R) * PO_EV_WAVE + lane;
                    const int kb = K >= 16 ? 2 * (k % 16) : ((i - 1) % R) * 2 * K + 2 * k;
                    if (kw != w || kb != bit) fail("the kernel's store is not the walk's word", K, i, j);
                }
            if (L % R == 0)
                for (uint32_t s : seen)
                    if (s != 0xffffffffu) { fail("a word with unused bits", K, L); break; }
        }
    }
}

static void room() {
    std::vector<int64_t> grid = {0, 1, 2, 15, 16, 17, 62, 63, 64, 65, 126, 127, 128, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024, 2046, 2047,
                                 2048, 4094, 4095, 4096, 4097, 5000, PO_ACC_MAX_LONG - 1, PO_ACC_MAX_LONG, PO_ACC_MAX_LONG + 1, 1000000};
    for (size_t x = 0; x < grid.size(); ++x)
        for (size_t y = 0; y < grid.size(); ++y) {
            const int64_t w = po_aln_trace_words(grid[x], grid[y]);
            if (w != po_aln_trace_words(grid[y], grid[x])) fail("the room is symmetric", (long)grid[x], (long)grid[y]);
            if (x + 1 < grid.size() && po_aln_trace_words(grid[x + 1], grid[y]) < w) fail("the room decreases in la", (long)grid[x], (long)grid[y]);
            if (y + 1 < grid.size() && po_aln_trace_words(grid[x], grid[y + 1]) < w) fail("the room decreases in lb", (long)grid[x], (long)grid[y]);
            const int64_t S = std::min(grid[x], grid[y]), L = std::max(grid[x], grid[y]);
            if (S <= PO_EDIT_MAX_SHORT && L <= PO_ACC_MAX_LONG && w != po_aln_words(natural_k((size_t)S), L)) fail("the room is the kernel's", (long)S, (long)L);
        }
    if (po_aln_trace_words(4095, 4095) != 4095 * 256 || po_aln_trace_words(0, 0) != 0 || po_aln_trace_words(-1, 5) != 0) fail("room values");
    if (po_aln_trace_words(63, 100) != 7 * 64 || po_aln_trace_words(64, 100) != 13 * 64) fail("room at the first edge");
}

static void cells() {
    if (po_aln_cell(PO_ALN_EQ, 2, 2) != 12 || po_aln_cell(PO_ALN_X, 1, 3) != 16 || po_aln_cell(PO_ALN_I, 1, 0xff) != 21 ||
        po_aln_cell(PO_ALN_D, 0xff, 3) != 19)
        fail("confusion cells");
    for (uint32_t code = 0; code < 4; ++code)
        for (int a = 0; a < 9; ++a)
            for (int b = 0; b < 9; ++b) {
                if (code == PO_ALN_EQ && a != b) continue;
                const bool ua = code != PO_ALN_D, ub = code != PO_ALN_I;
                const int got = po_aln_cell(code, a, b);
                if ((ua && a > 3) || (ub && b > 3)) { if (got != -1) fail("a byte above 3 is counted", (long)code, a, b); continue; }
                const int want = code == PO_ALN_EQ ? a * 5 + a : code == PO_ALN_X ? b * 5 + a : code == PO_ALN_I ? 20 + a : b * 5 + 4;
                if (got != want || got == 24) fail("confusion cell", (long)code, a, b);
            }
    int i = 5, j = 7;
    po_aln_step(PO_ALN_DIR_LEFT, &i, &j);
    po_aln_step(PO_ALN_DIR_UP, &i, &j);
    po_aln_step(PO_ALN_DIR_X, &i, &j);
    po_aln_step(PO_ALN_DIR_EQ, &i, &j);
    if (i != 2 || j != 4) fail("step");
    if (po_aln_op(PO_ALN_DIR_EQ, true) != PO_ALN_EQ || po_aln_op(PO_ALN_DIR_X, false) != PO_ALN_X || po_aln_op(PO_ALN_DIR_LEFT, true) != PO_ALN_I ||
        po_aln_op(PO_ALN_DIR_UP, true) != PO_ALN_D || po_aln_op(PO_ALN_DIR_LEFT, false) != PO_ALN_D || po_aln_op(PO_ALN_DIR_UP, false) != PO_ALN_I)
        fail("the op of a direction");
    // the word operation against its words, column by column
    for (int it = 0; it < 2000; ++it) {
        const uint32_t dirs = (rnd() << 8) ^ rnd();
        uint32_t cmp = 0;
        for (int k = 0; k < 16; ++k) cmp |= (rnd() % 3) << (2 * k);
        for (uint32_t tie_left = 0; tie_left < 2; ++tie_left) {
            const uint32_t got = po_aln_merge(dirs, cmp, tie_left ? ~0u : 0u);
            for (int k = 0; k < 16; ++k) {
                const uint32_t d = (dirs >> (2 * k)) & 3u, c = (cmp >> (2 * k)) & 3u;
                const uint32_t want = c == 2 ? PO_ALN_DIR_LEFT : c == 1 && tie_left && d == PO_ALN_DIR_UP ? PO_ALN_DIR_LEFT : d;
                if (((got >> (2 * k)) & 3u) != want) fail("merge", (long)d, (long)c, (long)tie_left);
            }
        }
    }
    if (po_aln_cmp3(5, 9) != -1 || po_aln_cmp3(9, 9) != 0 || po_aln_cmp3(10, 9) != 1 || po_aln_cmp3(-17000000, PO_EV_INF) != -1 ||
        po_aln_cmp3(PO_EV_INF, -17000000) != 1 || po_aln_cmp3(8, 9) != -1)
        fail("cmp3");
}

int main(int argc, char**) {
    small();
    random_pairs();
    packing();
    room();
    cells();
    if (argc > 1) std::printf("columns %ld, block fetches %ld\n", total_columns, total_refetches);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
