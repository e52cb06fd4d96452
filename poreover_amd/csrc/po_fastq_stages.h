// What the quality stages of `basecall --fastq` (po_basecall.hip) and of the pair pass
// (po_pair_basecall.hip) share on the host: the alignment of the (Viterbi call, scored string) pairs whose
// strings differ, as quality.call_guides does it — one band for the call's pairs, 500 + the largest length difference —
// with the aligner's workspace bounded by ~4 GiB a launch.  The caller lists the pairs, gathers their strings into
// pair_seq with a gather kernel of its own and reads the columns with po_launch_fastq_consumed.  Host only, hidden.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "po_hostbuf.h"

#pragma GCC visibility push(hidden)

struct PoFqAligner {
    PoDev pair_read, pair_seq, pair_off, aln1, aln2, aln_off, ncol, ast, wsa;
    std::vector<int32_t> reads;              // the item (read, or pair of reads) of aligned pair p
    std::vector<int64_t> so{0}, ao{0};       // string offsets (2 m + 1: called, scored), alignment offsets (m + 1)
    int64_t slack = 0, m1 = 0, m2 = 0;
    int band = 0, step = 0;
    size_t wab = 0;

    int m() const { return (int)reads.size(); }
    void reset() {   // before the pairs of another call are listed (an engine's resident state)
        reads.clear();
        so.assign(1, 0);
        ao.assign(1, 0);
        slack = m1 = m2 = 0;
    }
    // pair = (called, scored), as quality.call_guides aligns them
    void add(int read, int64_t Lc, int64_t L) {
        reads.push_back(read);
        so.push_back(so.back() + Lc);
        so.push_back(so.back() + L);
        ao.push_back(ao.back() + Lc + L + 8);
        slack = std::max(slack, Lc > L ? Lc - L : L - Lc);
        m1 = std::max(m1, Lc);
        m2 = std::max(m2, L);
    }
    // the band, the buffers and the tables of the listed pairs (m() > 0)
    int up(const char* me) {
        const int n = m();
        if (500 + slack > INT32_MAX) return po_fail(PO_E_ARG, std::string(me) + ": alignment band beyond 2^31 - 1");
        band = (int)(500 + slack);   // call_guides' rule: one band for the call's pairs
        // the aligner's workspace is per workgroup in flight: as many pairs a launch as ~4 GiB of it hold
        const size_t per_pair = po_align_workspace_bytes(1, m1, m2, band);
        step = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)4 << 30) / per_pair));
        wab = po_align_workspace_bytes(step, m1, m2, band);
        PO_HIPCHK(pair_read.up(reads.data(), sizeof(int32_t) * n));
        PO_HIPCHK(pair_off.up(so.data(), sizeof(int64_t) * so.size()));
        PO_HIPCHK(aln_off.up(ao.data(), sizeof(int64_t) * ao.size()));
        PO_HIPCHK(pair_seq.up(nullptr, (size_t)so.back()));
        PO_HIPCHK(aln1.up(nullptr, (size_t)ao.back()));
        PO_HIPCHK(aln2.up(nullptr, (size_t)ao.back()));
        PO_HIPCHK(ncol.up(nullptr, sizeof(int32_t) * n));
        PO_HIPCHK(ast.up(nullptr, sizeof(int32_t) * n));
        PO_HIPCHK(wsa.up(nullptr, wab));
        return PO_OK;
    }
    // po_align_batch over the gathered strings
    int run(hipStream_t stream) {
        const int n = m();
        for (int p0 = 0; p0 < n; p0 += step) {
            const int rc = po_align_batch(pair_seq, pair_off.as<int64_t>() + 2 * p0, std::min(step, n - p0), band, aln1, aln2,
                                          aln_off.as<int64_t>() + p0, ncol.as<int32_t>() + p0, ast.as<int32_t>() + p0, wsa, wab, stream);
            if (rc != PO_OK) return rc;
        }
        return PO_OK;
    }
};

#pragma GCC visibility pop
