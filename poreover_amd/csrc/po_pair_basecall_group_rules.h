// The group rule of po_pair_basecaller, once: contiguous runs of pairs in input order.  No HIP in this
// file: tools/pair_group_check.cpp compiles it alone under sanitizers and holds it against a brute-force restatement.
//
// A pair joins the run while the run's resident bytes with it stay within `budget` — 24 per sample of the run's distinct
// reads, 40 per frame of every pair side and extra(n_pairs, rows, longest): the pair chain's workspace and, for a fastq
// engine, the quality stages' bytes — and its pair-side frames within `share` (INT64_MAX: no cap); a pair that does not
// fit alone goes alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// the frame cap of a run over ndev devices: ceil(all pair-side frames / (2 ndev)), 1 at least; none on one device, where a
// second group is a second full recurrence
inline int64_t po_pair_group_share(int64_t frames, int ndev) {
    if (ndev <= 1) return INT64_MAX;
    return std::max<int64_t>(1, (frames + 2 * (int64_t)ndev - 1) / (2 * (int64_t)ndev));
}

// len[r]: samples of read r (n_reads of them); pair_idx: 2 n_pairs indices in [0, n_reads), checked by the caller.
// extra(int n, const int64_t t[2], const int64_t m[2]) -> int64_t.  Writes first[g], count[g] for g < min(groups, cap);
// returns the number of groups.
template <class Extra>
int po_pair_group_plan(const int64_t* len, int n_reads, const int32_t* pair_idx, int n_pairs, int64_t budget, int64_t share,
                       Extra extra, int32_t* first, int32_t* count, int cap) {
    std::vector<int> in_group((size_t)std::max(n_reads, 0), -1);   // the group that last took the read
    int g = 0, i = 0;
    while (i < n_pairs) {
        const int f = i;
        int64_t samples = 0, t[2] = {0, 0}, m[2] = {0, 0};
        for (; i < n_pairs; ++i) {
            const int a = pair_idx[2 * (size_t)i], b = pair_idx[2 * (size_t)i + 1];
            const int64_t s = samples + (in_group[a] != g ? len[a] : 0) + (b != a && in_group[b] != g ? len[b] : 0);
            const int64_t t2[2] = {t[0] + len[a], t[1] + len[b]}, m2[2] = {std::max(m[0], len[a]), std::max(m[1], len[b])};
            if (i > f && (t2[0] + t2[1] > share || s * 24 + (t2[0] + t2[1]) * 40 + extra(i - f + 1, t2, m2) > budget)) break;
            in_group[a] = in_group[b] = g;
            samples = s; t[0] = t2[0]; t[1] = t2[1]; m[0] = m2[0]; m[1] = m2[1];
        }
        if (g < cap) { first[g] = f; count[g] = i - f; }
        ++g;
    }
    return g;
}
