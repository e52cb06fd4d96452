// The rule of csrc/po_skip_rules.h (pair-decode --skip_matches: anchors, a2s, boxes) against hand-written tables, compiled alone
// (no HIP) under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_skip_cpu.py.
//   skip_check            the tables below; prints "ok"
//   skip_check --anchors  stdin: lines "matches indels row1 row2"; stdout: per line the anchors "cs:ce:type ..." of the
//                         serial form, after checking that the wave form (what the kernel computes) gives the same anchors
//                         and the a2s values of a direct count
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../poreover_amd/csrc/po_skip_rules.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)

struct Anc { int cs, ce, type; };

// serial and wave forms on one alignment; both must agree, the wave form's a2s values with a direct count
static std::vector<Anc> anchors_of(const std::string& r1, const std::string& r2, int matches, int indels,
                                   std::vector<int32_t>* a2s4 = nullptr) {
    const int ncol = (int)r1.size();
    const int cap = ncol + 1;
    std::vector<PoSkipAnchor> s((size_t)cap), w((size_t)cap);
    std::vector<int32_t> q(4 * (size_t)cap);
    const int ns = po_skip_anchors_serial(r1.data(), r2.data(), ncol, matches, indels, s.data(), cap);
    const int nw = po_skip_anchors_wave(r1.data(), r2.data(), ncol, matches, indels, w.data(), q.data(), cap);
    CHECK(ns == nw && ns <= cap);
    std::vector<int> c0((size_t)ncol + 1), c1((size_t)ncol + 1);
    int x0 = 0, x1 = 0;
    for (int c = 0; c < ncol; ++c) { x0 += r1[c] != '-'; x1 += r2[c] != '-'; c0[c] = x0; c1[c] = x1; }
    std::vector<Anc> out;
    for (int k = 0; k < ns && k < nw; ++k) {
        CHECK(s[k].cs == w[k].cs && s[k].ce == w[k].ce && s[k].type == w[k].type);
        CHECK(s[k].ce < ncol && s[k].cs < s[k].ce);
        CHECK(q[4 * k] == c0[s[k].cs] && q[4 * k + 1] == c1[s[k].cs] && q[4 * k + 2] == c0[s[k].ce] && q[4 * k + 3] == c1[s[k].ce]);
        out.push_back(Anc{s[k].cs, s[k].ce, s[k].type});
    }
    if (a2s4) *a2s4 = q;
    return out;
}

static bool same(const std::vector<Anc>& a, std::initializer_list<Anc> b) {
    if (a.size() != b.size()) return false;
    size_t i = 0;
    for (const Anc& x : b) { if (a[i].cs != x.cs || a[i].ce != x.ce || a[i].type != x.type) return false; ++i; }
    return true;
}

static void tables() {
    CHECK(po_skip_state('A', 'A') == PO_SKIP_MAT && po_skip_state('-', 'A') == PO_SKIP_INS);
    CHECK(po_skip_state('A', '-') == PO_SKIP_DEL && po_skip_state('A', 'C') == PO_SKIP_MIS);
    // a match run ended by a mismatch; the open run at the end is not reported
    CHECK(same(anchors_of("AAAACAAAA", "AAAAGAAAA", 3, 3), {{0, 4, PO_SKIP_MAT}}));
    CHECK(same(anchors_of("AAAACAAAA", "AAAAGAAAA", 5, 3), {}));
    CHECK(same(anchors_of("AAAA", "AAAA", 1, 1), {}));                      // all matching: nothing closes the run
    CHECK(same(anchors_of("AAAA", "CCCC", 1, 1), {}));                      // all mismatching
    CHECK(same(anchors_of("A", "C", 1, 1), {}));
    // gap runs of both kinds, thresholds met exactly
    CHECK(same(anchors_of("AA---CC", "AAGGGCC", 2, 3), {{0, 2, PO_SKIP_MAT}, {2, 5, PO_SKIP_INS}}));
    CHECK(same(anchors_of("AAGGGCC", "AA---CC", 2, 3), {{0, 2, PO_SKIP_MAT}, {2, 5, PO_SKIP_DEL}}));
    CHECK(same(anchors_of("AAGGGCC", "AA---CC", 2, 4), {{0, 2, PO_SKIP_MAT}}));
    CHECK(same(anchors_of("AAGGGCC", "AA---CC", 3, 4), {}));
    // mismatch columns between two runs: each a run of its own, never reported, even at thresholds of 1
    CHECK(same(anchors_of("AACGAA", "AAGCAT", 1, 1), {{0, 2, PO_SKIP_MAT}, {4, 5, PO_SKIP_MAT}}));
    // a run across the chunk edge 63 | 64 and one across 127 | 128
    {
        std::string a(200, 'A'), b(200, 'A');
        b[10] = 'C'; b[100] = 'C'; b[150] = 'C';
        CHECK(same(anchors_of(a, b, 10, 100), {{0, 10, PO_SKIP_MAT}, {11, 100, PO_SKIP_MAT}, {101, 150, PO_SKIP_MAT}}));
        CHECK(same(anchors_of(a, b, 50, 100), {{11, 100, PO_SKIP_MAT}}));
    }
    // the box rule: 2 anchors -> 3 boxes
    {
        // columns:        0123456789
        const std::string a = "AAACAAAGAA", b = "AAAGAAACAA";
        std::vector<int32_t> q;
        const std::vector<Anc> an = anchors_of(a, b, 3, 100, &q);
        CHECK(same(an, {{0, 3, PO_SKIP_MAT}, {4, 7, PO_SKIP_MAT}}));
        const int32_t map1[10] = {0, 2, 4, 6, 8, 10, 12, 14, 16, 18}, map2[10] = {1, 3, 5, 7, 9, 11, 13, 15, 17, 19};
        int32_t env[40];
        for (int u = 0; u < 20; ++u) { env[2 * u] = u > 3 ? u - 3 : 0; env[2 * u + 1] = u + 4 < 21 ? u + 4 : 21; }
        PoSkipBox bx;
        int pos;
        CHECK(po_skip_box(0, 2, 0, 0, q[0], q[1], map1, 10, map2, 10, 20, 21, env, &bx, &pos) == PO_OK);
        CHECK(bx.b0 == 0 && bx.b1 == 2 && pos == 2 && bx.lo == 0 && bx.hi == 5);       // a2s[0][0] = 1 -> map1[1] = 2
        CHECK(po_skip_box(1, 2, q[2], q[3], q[4], q[5], map1, 10, map2, 10, 20, 21, env, &bx, &pos) == PO_OK);
        CHECK(bx.b0 == 8 && bx.b1 == 10 && pos == 10 && bx.lo == 5 && bx.hi == 13);     // a2s[0][3] = 4, a2s[0][4] = 5
        CHECK(po_skip_box(2, 2, q[6], q[7], 0, 0, map1, 10, map2, 10, 20, 21, env, &bx, &pos) == PO_OK);
        CHECK(bx.b0 == 16 && bx.b1 == 20 && bx.lo == 13 && bx.hi == 21);               // a2s[0][7] = 8 -> map1[8] = 16
        // a map index equal to the basecall's length, on either read
        CHECK(po_skip_box(2, 2, 10, 3, 0, 0, map1, 10, map2, 10, 20, 21, env, &bx, &pos) == PO_E_BOX);
        CHECK(po_skip_box(1, 2, 3, 3, 4, 10, map1, 10, map2, 10, 20, 21, env, &bx, &pos) == PO_E_BOX);
        // an empty box
        CHECK(po_skip_box(1, 2, 4, 4, 4, 4, map1, 10, map2, 10, 20, 21, env, &bx, &pos) == PO_E_BOX);
    }
    CHECK(po_skip_table_row(100, 0, 3, 10, 100) == 13 && po_skip_table_row(100, 40, 0, 100, 6) == 10);
    CHECK(po_skip_text_less("AC", 2, "AG", 2) && !po_skip_text_less("AG", 2, "AC", 2) && po_skip_text_less("A", 1, "AC", 2));
    CHECK(!po_skip_text_less("AC", 2, "AC", 2) && po_skip_text_less("", 0, "A", 1));
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--anchors") == 0) {
        std::string line;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            int matches, indels;
            std::string r1, r2;
            if (!(in >> matches >> indels >> r1 >> r2) || r1.size() != r2.size()) { std::printf("bad line\n"); return 2; }
            std::string out;
            for (const Anc& a : anchors_of(r1, r2, matches, indels))
                out += (out.empty() ? "" : " ") + std::to_string(a.cs) + ":" + std::to_string(a.ce) + ":" + std::to_string(a.type);
            std::printf("%s\n", out.c_str());
        }
        return fails ? 1 : 0;
    }
    tables();
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
