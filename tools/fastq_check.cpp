// The per-element rules of `basecall --fastq` (poreover_amd/csrc/po_fastq_rules.h), the part of the feature that needs no
// device: the same source the kernels of po_fastq.hip run.  Plain C++, no HIP: built and run under
// -fsanitize=address,undefined by tests/test_basecall_fastq_cpu.py.  Exit status 0 and "ok" when every case holds.
//   fastq_check                 the guide rule against a linear scan for every frame map of T <= 6 frames (every subset of the
//                               frames), with consumed[j] = j + 1, with every non-decreasing consumed[] up to 3, and on the
//                               diagonal; the consumed rule against a column-by-column count for every pair of gapped rows of
//                               up to 6 columns, unclipped and clipped, and for rows of 200 columns (blocks of 64 with
//                               carries); every array in a heap block of exactly its size
//   fastq_check TABLE OUT       TABLE: int32 n, n x 5 float64 log-odds, n int32 own columns.  OUT: n bytes, Q of every row
#include "../poreover_amd/csrc/po_fastq_rules.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

static void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    if (failures < 20) std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
    ++failures;
}

// ---- guide
static void check_guide(int T, const std::vector<int32_t>& map, const std::vector<int32_t>* consumed, int L) {
    const int Lc = (int)map.size();
    const int mode = consumed ? PO_FQ_CONSUMED : PO_FQ_IDENTITY;
    for (int t = 0; t < T; ++t) {
        int j = -1;
        for (int k = 0; k < Lc; ++k)
            if (map[(size_t)k] <= t) j = k;
        const int want = j < 0 ? 0 : consumed ? (*consumed)[(size_t)j] : j + 1;
        const int got = po_fq_guide(map.data(), Lc, consumed ? consumed->data() : nullptr, mode, t, T, L);
        if (got != want) fail("guide", T, t, got);
    }
}

static void consumed_tables(int Lc, int top, std::vector<int32_t>& cur, int T, const std::vector<int32_t>& map) {
    if ((int)cur.size() == Lc) {
        std::vector<int32_t> exact(cur);   // (a fresh block of exactly Lc values)
        check_guide(T, map, &exact, top);
        return;
    }
    for (int v = cur.empty() ? 0 : cur.back(); v <= top; ++v) {
        cur.push_back(v);
        consumed_tables(Lc, top, cur, T, map);
        cur.pop_back();
    }
}

static void guides() {
    for (int T = 1; T <= 6; ++T) {
        for (unsigned frames = 0; frames < (1u << T); ++frames) {
            std::vector<int32_t> map;
            for (int t = 0; t < T; ++t)
                if (frames & (1u << t)) map.push_back(t);
            check_guide(T, map, nullptr, (int)map.size());
            for (int top = 0; top <= 3; ++top) {
                std::vector<int32_t> cur;
                consumed_tables((int)map.size(), top, cur, T, map);
            }
        }
        for (int L = 0; L <= T + 2; ++L)
            for (int t = 0; t < T; ++t)
                if (po_fq_guide(nullptr, 0, nullptr, PO_FQ_DIAGONAL, t, T, L) != ((t + 1) * L) / T) fail("diagonal", T, L, t);
    }
    if (po_fq_guide(nullptr, 0, nullptr, PO_FQ_DIAGONAL, 2999999999LL, 3000000000LL, 1 << 25) != (1 << 25)) fail("diagonal in 64 bits");
}

// ---- consumed: the kernel's loop (blocks of 64 columns, two masks, two carries) against a count column by column
static void check_consumed(const std::vector<char>& r1, const std::vector<char>& r2, int L) {
    const int64_t nc = (int64_t)r1.size();
    std::vector<int32_t> want;
    int seen2 = 0;
    for (int64_t c = 0; c < nc; ++c) {
        if (r2[(size_t)c] != PO_FQ_GAP) ++seen2;
        if (r1[(size_t)c] != PO_FQ_GAP) want.push_back(seen2 < L ? seen2 : L);
    }
    std::vector<int32_t> got(want.size(), -1);
    int carry1 = 0, carry2 = 0;
    for (int64_t c0 = 0; c0 < nc; c0 += 64) {
        uint64_t m1 = 0, m2 = 0;
        for (int lane = 0; lane < 64 && c0 + lane < nc; ++lane) {
            if (r1[(size_t)(c0 + lane)] != PO_FQ_GAP) m1 |= (uint64_t)1 << lane;
            if (r2[(size_t)(c0 + lane)] != PO_FQ_GAP) m2 |= (uint64_t)1 << lane;
        }
        for (int lane = 0; lane < 64; ++lane) {
            int j;
            int32_t v;
            if (!po_fq_consumed_column(m1, m2, lane, carry1, carry2, L, &j, &v)) continue;
            if (j < 0 || j >= (int)got.size() || got[(size_t)j] != -1) { fail("consumed: one writer per called base", (long)nc, j); continue; }
            got[(size_t)j] = v;
        }
        carry1 += po_fq_popc(m1);
        carry2 += po_fq_popc(m2);
    }
    if (carry1 != (int)want.size() || got != want) fail("consumed", (long)nc, L);
}

static void consumed() {
    const char cell[4][2] = {{'A', 'A'}, {'A', PO_FQ_GAP}, {PO_FQ_GAP, 'C'}, {PO_FQ_GAP, PO_FQ_GAP}};
    for (int nc = 0; nc <= 6; ++nc) {
        for (unsigned code = 0; code < (1u << (2 * nc)); ++code) {
            std::vector<char> r1((size_t)nc), r2((size_t)nc);
            int n2 = 0;
            for (int c = 0; c < nc; ++c) {
                const int k = (code >> (2 * c)) & 3;
                r1[(size_t)c] = cell[k][0];
                r2[(size_t)c] = cell[k][1];
                n2 += cell[k][1] != PO_FQ_GAP;
            }
            check_consumed(r1, r2, n2);
            if (n2 > 0) check_consumed(r1, r2, n2 - 1);   // the clip
        }
    }
    for (int variant = 0; variant < 4; ++variant) {   // 200 columns: three full blocks and a part
        std::vector<char> r1(200), r2(200);
        int n2 = 0;
        uint32_t x = 12345u + (uint32_t)variant;
        for (int c = 0; c < 200; ++c) {
            x = x * 1664525u + 1013904223u;
            int k = (int)((x >> 24) % 3);
            if (variant == 1) k = c < 70 ? 1 : (c < 140 ? 2 : 0);   // runs longer than a block
            if (variant == 2) k = 0;
            r1[(size_t)c] = cell[k][0];
            r2[(size_t)c] = cell[k][1];
            n2 += cell[k][1] != PO_FQ_GAP;
        }
        check_consumed(r1, r2, n2);
        check_consumed(r1, r2, n2 / 2);
    }
}

// ---- Phred of a table
static int phred_table(const char* in_path, const char* out_path) {
    std::FILE* f = std::fopen(in_path, "rb");
    if (!f) { std::printf("FAILED cannot read %s\n", in_path); return 1; }
    int32_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0) { std::fclose(f); std::printf("FAILED table header\n"); return 1; }
    std::vector<double> odds((size_t)n * 5);
    std::vector<int32_t> own((size_t)n);
    const bool ok = std::fread(odds.data(), sizeof(double), odds.size(), f) == odds.size() &&
                    std::fread(own.data(), sizeof(int32_t), own.size(), f) == own.size();
    std::fclose(f);
    if (!ok) { std::printf("FAILED table body\n"); return 1; }
    std::vector<unsigned char> q((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        std::vector<double> row(odds.begin() + (size_t)i * 5, odds.begin() + (size_t)i * 5 + 5);   // exactly five
        q[(size_t)i] = (unsigned char)po_fq_phred(row.data(), own[(size_t)i]);
    }
    std::FILE* g = std::fopen(out_path, "wb");
    if (!g || std::fwrite(q.data(), 1, q.size(), g) != q.size()) { if (g) std::fclose(g); std::printf("FAILED cannot write %s\n", out_path); return 1; }
    std::fclose(g);
    std::printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return phred_table(argv[1], argv[2]);
    guides();
    consumed();
    {   // Phred's edges: +inf, all alternatives -inf, NaN, a column that is no column, and the alphabet
        const double inf = HUGE_VAL;
        const double a[5] = {0.0, inf, -3.0, -4.0, -5.0}, b[5] = {-inf, 0.0, -inf, -inf, -inf}, c[5] = {0.0, -1.0, NAN, -2.0, -3.0};
        const double d[5] = {0.0, 700.0, -700.0, 700.0, -700.0}, e[5] = {-700.0, -700.0, -700.0, 0.0, -700.0};
        if (po_fq_phred(a, 0) != 0) fail("phred: +inf is Q 0");
        if (po_fq_phred(b, 1) != PO_FQ_QMAX) fail("phred: no alternative is Q 60");
        if (po_fq_phred(c, 0) != 0) fail("phred: NaN is Q 0");
        if (po_fq_phred(d, 0) != 0 || po_fq_phred(e, 3) != PO_FQ_QMAX) fail("phred: +-700");
        if (po_fq_phred(a, -1) != 0 || po_fq_phred(a, 5) != 0) fail("phred: own column outside the row");
        if (po_fq_code("ACGT", 'G') != 2 || po_fq_code("ACGT", 'N') != -1) fail("alphabet code");
    }
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
