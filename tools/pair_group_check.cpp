// The group rule of csrc/po_pair_basecall_group_rules.h (po_pair_basecaller's planner) against a brute-force
// restatement with sets, compiled alone (no HIP) under AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_pair_basecall_stream_cpu.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../poreover_amd/csrc/po_pair_basecall_group_rules.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)

struct Group { int first, count; };

// a stand-in for the size queries: grows with the pairs, the rows and the longest read
static int64_t extra(int n, const int64_t* t, const int64_t* m) { return 1000 * (int64_t)n + 3 * (t[0] + t[1]) + 7 * (m[0] + m[1]); }

// pair_basecall.engine_group_plan, line for line
static std::vector<Group> brute(const std::vector<int64_t>& len, const std::vector<int32_t>& idx, int64_t budget, int64_t share) {
    std::vector<Group> out;
    const int P = (int)idx.size() / 2;
    int first = 0;
    std::set<int> reads;
    int64_t samples = 0, tr[2] = {0, 0}, mr[2] = {0, 0};
    for (int k = 0; k < P; ++k) {
        const int a = idx[2 * k], b = idx[2 * k + 1];
        std::set<int> both = {a, b};
        int64_t s = samples;
        for (int r : both) if (!reads.count(r)) s += len[r];
        int64_t t[2] = {tr[0] + len[a], tr[1] + len[b]}, m[2] = {std::max(mr[0], len[a]), std::max(mr[1], len[b])};
        if (k > first && (t[0] + t[1] > share || s * 24 + (t[0] + t[1]) * 40 + extra(k - first + 1, t, m) > budget)) {
            out.push_back(Group{first, k - first});
            first = k;
            reads.clear();
            s = 0;
            for (int r : both) s += len[r];
            t[0] = m[0] = len[a]; t[1] = m[1] = len[b];
        }
        reads.insert(a); reads.insert(b);
        samples = s; tr[0] = t[0]; tr[1] = t[1]; mr[0] = m[0]; mr[1] = m[1];
    }
    if (P > first) out.push_back(Group{first, P - first});
    return out;
}

static void one(const std::vector<int64_t>& len, const std::vector<int32_t>& idx, int64_t budget, int ndev, int cap) {
    const int P = (int)idx.size() / 2;
    int64_t frames = 0;
    for (int32_t r : idx) frames += len[r];
    const int64_t share = po_pair_group_share(frames, ndev);
    const std::vector<Group> want = brute(len, idx, budget, share);
    std::vector<int32_t> first((size_t)cap, -1), count((size_t)cap, -1);   // exactly cap entries: a write past them is the sanitizer's
    const int g = po_pair_group_plan(len.data(), (int)len.size(), idx.data(), P, budget, share, extra, first.data(), count.data(), cap);
    CHECK(g == (int)want.size());
    int at = 0;
    for (int k = 0; k < g && k < cap && k < (int)want.size(); ++k) {
        CHECK(first[k] == want[k].first && count[k] == want[k].count);
        CHECK(first[k] == at && count[k] >= 1);
        at += count[k];
    }
    if (cap >= g) CHECK(at == P);
}

int main() {
    CHECK(po_pair_group_share(100, 1) == INT64_MAX && po_pair_group_share(100, 2) == 25 && po_pair_group_share(101, 2) == 26);
    CHECK(po_pair_group_share(0, 8) == 1);
    unsigned seed = 12345;
    auto rnd = [&](unsigned n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
    for (int round = 0; round < 400; ++round) {
        const int R = 1 + (int)rnd(12), P = (int)rnd(40);
        std::vector<int64_t> len((size_t)R);
        for (auto& L : len) L = 1 + (int64_t)rnd(rnd(8) == 0 ? 60000 : 400);
        std::vector<int32_t> idx(2 * (size_t)P);
        for (auto& r : idx) r = (int32_t)rnd((unsigned)R);
        const int64_t budgets[] = {1, 30000, 200000, 5000000, (int64_t)1 << 60};
        for (int64_t budget : budgets)
            for (int ndev : {1, 2, 8, 16})
                for (int cap : {0, 1, P}) one(len, idx, budget, ndev, cap);
    }
    one({}, {}, 1000, 2, 0);       // no reads, no pairs
    one({5}, {0, 0}, 1, 1, 1);     // one pair of a read with itself, over the budget: alone
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
