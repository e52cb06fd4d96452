// The host-side rules of the pair quality stages (poreover_amd/csrc/po_pair_fastq_plan.h) and the consensus Phred rule
// (po_fastq_rules.h: po_fq_pair_phred), the part of po_pair_basecall_fastq_batch_h / po_pair_qual_h that needs no device.
// Plain C++, no HIP: built and run under -fsanitize=address,undefined by tests/test_pair_basecall_fastq_cpu.py.  Exit
// status 0 and "ok" when every case holds.
//   - the per-side dense offset tables from the interleaved seq1d_off, against the interleaved entries;
//   - an item's length and class (empty, banded, unbanded) against the rule spelled out per item;
//   - the two dense layouts, against loops: every base of every item has exactly one row in the combined buffer, inside
//     the part of the call that owns the item, and the rows of an item are consecutive; an item has L = 0 in the call
//     that does not own it;
//   - the merged status: the owner's entry, 0 for an empty item;
//   - the guide blocks: four blocks back to back, each with its side's rows;
//   - the combine rule: both standing -> the Phred of the value-by-value sum, one standing -> its own, none -> 0.
// Every table lives in a heap block of exactly its size: a read past its end is a sanitizer report.
#include "../poreover_amd/csrc/po_fastq_rules.h"
#include "../poreover_amd/csrc/po_pair_fastq_plan.h"

#include <cstdio>

static int failures = 0;

static void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    if (failures < 20) std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
    ++failures;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static void check_plan(const std::vector<int64_t>& room1d, const std::vector<int32_t>& status, const std::vector<int32_t>& len1,
                       const std::vector<int32_t>& len2, const std::vector<int32_t>& len, int band, const std::vector<int32_t>* flags) {
    const int n = (int)status.size();
    std::vector<int64_t> s1o(1, 0);
    for (int64_t r : room1d) s1o.push_back(s1o.back() + r);
    const std::vector<int64_t> seq1d_off(s1o);   // exactly 2 n + 1 entries
    PoPairFastqPlan p;
    po_pair_fastq_make_plan(seq1d_off.data(), n, status.data(), len1.data(), len2.data(), len.data(), band, flags ? flags->data() : nullptr, &p);
    for (int s = 0; s < 2; ++s) {
        if (p.off1d[s].size() != (size_t)n + 1) { fail("off1d size", s); return; }
        for (int i = 0; i < n; ++i)
            if (p.off1d[s][(size_t)i] != seq1d_off[2 * (size_t)i + s]) fail("off1d", s, i);
        if (p.off1d[s][(size_t)n] != seq1d_off[2 * (size_t)n]) fail("off1d end", s);
    }
    int64_t cons = 0;
    for (int k = 0; k < PO_PQ_ITEMS; ++k) {
        // ---- length and class, item by item
        int64_t nb = 0, nu = 0;
        for (int i = 0; i < n; ++i) {
            const int32_t raw = k == 0 ? len1[(size_t)i] : k == 1 ? len2[(size_t)i] : len[(size_t)i];
            int32_t L = raw;
            if (status[(size_t)i] != 0 || raw < 0) L = 0;
            int want = PO_PQ_BANDED;
            if (band <= 0) want = PO_PQ_UNBANDED;
            if (flags && (*flags)[4 * (size_t)i + k]) want = PO_PQ_UNBANDED;
            if (L == 0) want = PO_PQ_NONE;
            if (p.len[k][(size_t)i] != L || p.cls[k][(size_t)i] != want) fail("length / class", k, i);
            if (p.len_b[k][(size_t)i] != (want == PO_PQ_BANDED ? L : 0)) fail("banded length", k, i);
            const int64_t Lb = p.off_b[k][(size_t)i + 1] - p.off_b[k][(size_t)i], Lu = p.off_u[k][(size_t)i + 1] - p.off_u[k][(size_t)i];
            if (Lb != (want == PO_PQ_BANDED ? L : 0) || Lu != (want == PO_PQ_UNBANDED ? L : 0)) fail("L in the two calls", k, i);
            nb += Lb;
            nu += Lu;
        }
        if (p.off_b[k][0] != 0 || p.off_u[k][0] != 0 || p.total_b[k] != nb || p.total_u[k] != nu || p.total(k) != nb + nu) fail("totals", k);
        // ---- one row per base in the combined buffer, inside the owner's part
        std::vector<int> hits((size_t)(nb + nu), 0);
        for (int i = 0; i < n; ++i) {
            const int c = p.cls[k][(size_t)i];
            for (int64_t j = 0; j < p.len[k][(size_t)i]; ++j) {
                const int64_t row = p.pos[k][(size_t)i] + j;
                if (row < 0 || row >= nb + nu) { fail("row inside the buffer", k, i, (long)row); continue; }
                if ((c == PO_PQ_BANDED) != (row < nb)) fail("row in the owner's part", k, i, (long)row);
                const int64_t local = c == PO_PQ_BANDED ? row : row - nb;
                const std::vector<int64_t>& off = c == PO_PQ_BANDED ? p.off_b[k] : p.off_u[k];
                if (local < off[(size_t)i] || local >= off[(size_t)i + 1]) fail("row inside the item of its call", k, i, (long)row);
                ++hits[(size_t)row];
            }
        }
        for (size_t r = 0; r < hits.size(); ++r)
            if (hits[r] != 1) fail("one item per row", k, (long)r, hits[r]);
        // ---- the merged status
        std::vector<int32_t> st(2 * (size_t)n);
        for (size_t x = 0; x < st.size(); ++x) st[x] = (int32_t)(100 + x);
        for (int i = 0; i < n; ++i) {
            const int c = p.cls[k][(size_t)i];
            const int32_t want = c == PO_PQ_NONE ? 0 : c == PO_PQ_BANDED ? 100 + i : 100 + n + i;
            if (po_pair_fastq_status(p, k, i, st.data()) != want) fail("merged status", k, i);
        }
        if (k == 2)
            for (int i = 0; i < n; ++i) {
                if (p.cons_off[(size_t)i] != cons) fail("consensus offsets", i);
                cons += p.len[2][(size_t)i];
            }
    }
    if (p.cons_off.size() != (size_t)n + 1 || p.cons_off[(size_t)n] != cons) fail("consensus total");
    for (int i = 0; i < n; ++i)
        if (p.len[2][(size_t)i] != p.len[3][(size_t)i]) fail("one consensus on both tables", i);
}

static void plans() {
    for (int round = 0; round < 400; ++round) {
        const int n = (int)(rnd() % 7);
        std::vector<int64_t> room;
        std::vector<int32_t> st, l1, l2, ln, flags;
        for (int i = 0; i < n; ++i) {
            const int32_t a = (int32_t)(rnd() % 9), b = (int32_t)(rnd() % 9), c = (int32_t)(rnd() % 12);
            room.push_back(a + (int64_t)(rnd() % 3));
            room.push_back(b + (int64_t)(rnd() % 3));
            const uint32_t r = rnd() % 6;
            st.push_back(r == 0 ? 1 : r == 1 ? 2 : r == 2 ? -3 : 0);
            l1.push_back(round % 5 == 4 ? 0 : a);      // (the diagonal envelope: no 1-D calls)
            l2.push_back(round % 5 == 4 ? 0 : b);
            ln.push_back(rnd() % 11 == 0 ? -1 : c);
            for (int k = 0; k < 4; ++k) flags.push_back(rnd() % 3 == 0 ? (int32_t)(1 + rnd() % 2) : 0);
        }
        const int band = round % 3 == 0 ? 0 : round % 3 == 1 ? 16 : -1;
        check_plan(room, st, l1, l2, ln, band, round % 2 ? &flags : nullptr);
        check_plan(room, st, l1, l2, ln, 16, &flags);
    }
    if (po_pair_fastq_guide_base(0, 7, 11) != 0 || po_pair_fastq_guide_base(1, 7, 11) != 7 || po_pair_fastq_guide_base(2, 7, 11) != 18 ||
        po_pair_fastq_guide_base(3, 7, 11) != 25)
        fail("guide blocks");
    if (po_pq_side(0) != 0 || po_pq_side(1) != 1 || po_pq_side(2) != 0 || po_pq_side(3) != 1) fail("an item's side");
}

static void combine() {
    const double inf = HUGE_VAL;
    for (int round = 0; round < 2000; ++round) {
        std::vector<double> a(5), b(5), sum(5);   // exactly five each
        for (int c = 0; c < 5; ++c) {
            a[(size_t)c] = rnd() % 17 == 0 ? -inf : -(double)(rnd() % 20000) / 1000.0 + 2.0;
            b[(size_t)c] = rnd() % 17 == 0 ? -inf : -(double)(rnd() % 20000) / 1000.0 + 2.0;
            sum[(size_t)c] = a[(size_t)c] + b[(size_t)c];
        }
        const int own = (int)(rnd() % 4);
        if (po_fq_pair_phred(a.data(), b.data(), true, true, own) != po_fq_phred(sum.data(), own)) fail("combine: both", round);
        if (po_fq_pair_phred(a.data(), b.data(), true, false, own) != po_fq_phred(a.data(), own)) fail("combine: first alone", round);
        if (po_fq_pair_phred(a.data(), b.data(), false, true, own) != po_fq_phred(b.data(), own)) fail("combine: second alone", round);
        if (po_fq_pair_phred(a.data(), b.data(), false, false, own) != 0) fail("combine: neither", round);
    }
    const double hi[5] = {0.0, -30.0, -30.0, -30.0, -30.0};   // two reads of Q ~ 124 together: the clip at 60
    if (po_fq_pair_phred(hi, hi, true, true, 0) != PO_FQ_QMAX) fail("combine: the clip");
    const double none[5] = {0.0, -inf, -inf, -inf, -inf};
    if (po_fq_pair_phred(none, hi, true, true, 0) != PO_FQ_QMAX) fail("combine: -inf alternatives stay -inf");
}

int main() {
    plans();
    combine();
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
