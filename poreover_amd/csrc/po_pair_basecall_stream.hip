// po_pair_basecaller: `pair-basecall` over one or several devices of a node, on the engine layer (po_engine.h, DESIGN.md
// §17.6).  Its items are pairs; a group is a contiguous run of them (po_pair_basecall_group_plan).  A group's distinct reads
// are compacted and indexed locally; it runs po_pair_basecall_body — the body of po_pair_basecall_batch_h /
// po_pair_basecall_fastq_batch_h; a window's bits do not depend on its call, DESIGN.md §16.3, and a pair's chain reads its
// own two tables alone.  On the raw route a pair that names a read which kept nothing is not run (PO_E_ARG in its status).
// A read's logits and kept count are written by the first group that names it.  The body's slice-pool query (po_engine.h)
// is po_pair_decode_workspace_bytes.
#include <algorithm>
#include <cstring>

#include "po_engine.h"
#include "po_pair_basecall_group_rules.h"
#include "po_pair_basecall_pass.h"

struct PoPairBasecallWorker : PoEngineWorker {
    PoPairBasecallResident* st = nullptr;
};

struct po_pair_basecaller : PoEngine<PoPairBasecallWorker> {
    po_pair_basecaller_options opt;
    struct Stat { int64_t pairs = 0, reads = 0, samples = 0; int groups = 0; double busy_ms = 0; };
    std::vector<Stat> stats;        // per worker, of the last run
};

// The groups of a run (po_pair_basecall_group_rules.h has the rule): the byte sum is pair_basecall.pair_groups' — 24 per
// sample of the run's distinct reads, 40 per frame of every pair side, the pair chain's workspace and (fastq) the quality
// stages' bytes — and, with ndev > 1, a run holds at most ceil(total pair-side frames / (2 ndev)) pair-side frames.
// Writes first[g], count[g] for g < min(groups, cap) and returns the number of groups, or PO_E_ARG.
extern "C" int po_pair_basecall_group_plan(const int64_t* len, int n_reads, const int32_t* pair_idx, int n_pairs,
                                           const po_pair_options* opt, int fastq, int band_size, int64_t resident_bytes, int ndev,
                                           int32_t* first, int32_t* count, int cap) {
    const std::string me = "po_pair_basecall_group_plan: ";
    if (n_reads < 0 || n_pairs < 0 || (n_reads > 0 && !len) || (n_pairs > 0 && !pair_idx) || !opt || resident_bytes < 0 || ndev < 1 ||
        cap < 0 || (cap > 0 && (!first || !count)))
        return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads) + ", n_pairs " + std::to_string(n_pairs) + ", resident_bytes " +
                       std::to_string(resident_bytes) + ", ndev " + std::to_string(ndev) + ", cap " + std::to_string(cap));
    int64_t frames = 0;
    for (int i = 0; i < n_pairs; ++i)
        for (int s = 0; s < 2; ++s) {
            const int64_t r = pair_idx[2 * (size_t)i + s];
            if (r < 0 || r >= n_reads || len[r] < 0)
                return po_fail(PO_E_ARG, me + "pair " + std::to_string(i) + " names read " + std::to_string(r) + " (reads 0 to " +
                               std::to_string(n_reads - 1) + ")");
            frames += len[r];
        }
    // the pair chain's workspace and (fastq) pair_basecall.qual_bytes_query's bytes
    auto extra = [&](int n, const int64_t* t, const int64_t* m) {
        int64_t b = (int64_t)po_pair_decode_workspace_bytes(n, t[0], t[1], m[0], m[1], NOUT, opt);
        if (fastq) {
            size_t ws = 0;
            for (int side = 0; side < 2; ++side)
                for (const int64_t L : {t[side], t[0] + t[1]})
                    ws = std::max(ws, po_qual_workspace_bytes(n, t[side], m[side], L, band_size, opt->model));
            b += (t[0] + t[1]) * ((band_size > 0 ? 17 : 0) + 2 + 41 * 3) + (int64_t)ws;
        }
        return b;
    };
    return po_pair_group_plan(len, n_reads, pair_idx, n_pairs, resident_bytes ? resident_bytes : DEFAULT_RESIDENT,
                              po_pair_group_share(frames, ndev), extra, first, count, cap);
}

namespace {

struct Run {
    po_pair_basecaller* b;
    // f32 route: signal / off; raw route: raw / off with offset / alpha
    const float* signal = nullptr;
    const int16_t* raw = nullptr;
    const int64_t* off = nullptr;
    const double *offset = nullptr, *alpha = nullptr;
    int n_reads = 0, n_pairs = 0;
    const int32_t* pair_idx = nullptr;
    char* seq1d; const int64_t* seq1d_off; int32_t* len1; int32_t* len2; double* identity;
    char* seq; const int64_t* seq_off; int32_t* seq_len; int32_t* status; float* logits;
    const int32_t* unbanded; char* qual1d; char* qual; int32_t* qual_status; int64_t* kept;
    std::vector<int32_t> first, count, owner;   // owner[r]: the first group that names read r (-1: none does)
    const char* name = "";
};

// one group: pairs f .. f + c - 1.  Its distinct reads in ascending order are the call's reads; the pairs that run are
// indexed into them; outputs go through buffers of the call's own layout and from there to the pairs' places.
int run_group(Run& r, PoPairBasecallWorker& w, po_pair_basecaller::Stat& stat, int g) {
    const po_pair_basecaller* b = r.b;
    const po_pair_basecaller_options& o = b->opt;
    const int f = r.first[g], c = r.count[g];
    std::vector<int> reads;
    for (int i = f; i < f + c; ++i) { reads.push_back(r.pair_idx[2 * (size_t)i]); reads.push_back(r.pair_idx[2 * (size_t)i + 1]); }
    std::sort(reads.begin(), reads.end());
    reads.erase(std::unique(reads.begin(), reads.end()), reads.end());
    const int nr = (int)reads.size();
    std::vector<int64_t> ro((size_t)nr + 1, 0);
    for (int j = 0; j < nr; ++j) ro[j + 1] = ro[j] + (r.off[reads[j] + 1] - r.off[reads[j]]);
    stat.pairs += c;
    stat.reads += nr;
    stat.samples += ro[nr];

    // ---- the signal of the group's reads, and so[]: the offsets of the samples the network sees
    std::vector<float> sig;
    std::vector<int64_t> so;
    if (r.raw) {
        std::vector<int16_t> raw((size_t)ro[nr]);
        for (int j = 0; j < nr; ++j)
            if (ro[j + 1] > ro[j]) std::memcpy(raw.data() + ro[j], r.raw + r.off[reads[j]], sizeof(int16_t) * (size_t)(ro[j + 1] - ro[j]));
        std::vector<double> of, al;   // in the group's order
        if (r.offset)
            for (int j = 0; j < nr; ++j) { of.push_back(r.offset[reads[j]]); al.push_back(r.alpha[reads[j]]); }
        const int rc = w.prepare_raw(raw.data(), ro.data(), nr, r.offset ? of.data() : nullptr, r.offset ? al.data() : nullptr, o.scaling,
                                     o.lo, o.hi, r.name, po_pair_basecall_resident_net(w.st), so);
        if (rc != PO_OK) return rc;
        for (int j = 0; j < nr; ++j)
            if (r.owner[reads[j]] == g) r.kept[reads[j]] = so[j + 1] - so[j];
    } else {
        so = ro;
        sig.resize((size_t)ro[nr]);
        for (int j = 0; j < nr; ++j) std::memcpy(sig.data() + ro[j], r.signal + r.off[reads[j]], sizeof(float) * (size_t)(ro[j + 1] - ro[j]));
    }
    // the reads with a sample, back to back as they lie (a read that kept nothing has no samples), and their local indices
    std::vector<int> local((size_t)nr, -1), kept_reads;
    std::vector<int64_t> lo(1, 0);
    for (int j = 0; j < nr; ++j)
        if (so[j + 1] > so[j]) { local[j] = (int)kept_reads.size(); kept_reads.push_back(j); lo.push_back(so[j + 1]); }
    const int m_reads = (int)kept_reads.size();

    // ---- the pairs that run, their outputs' tables from 0 with the caller's room
    std::vector<int> run;
    std::vector<int32_t> idx;
    std::vector<int64_t> s1o(1, 0), co(1, 0);
    for (int i = f; i < f + c; ++i) {
        int l[2];
        for (int s = 0; s < 2; ++s)
            l[s] = local[std::lower_bound(reads.begin(), reads.end(), r.pair_idx[2 * (size_t)i + s]) - reads.begin()];
        if (l[0] < 0 || l[1] < 0) {   // names a read that kept nothing: not run
            r.status[i] = PO_E_ARG;
            r.len1[i] = r.len2[i] = r.seq_len[i] = 0;
            r.identity[i] = 0.0;
            if (r.qual_status) std::fill(r.qual_status + 4 * (size_t)i, r.qual_status + 4 * (size_t)i + 4, 0);
            continue;
        }
        run.push_back(i);
        for (int s = 0; s < 2; ++s) {
            idx.push_back(l[s]);
            s1o.push_back(s1o.back() + (r.seq1d_off[2 * (size_t)i + s + 1] - r.seq1d_off[2 * (size_t)i + s]));
        }
        co.push_back(co.back() + (r.seq_off[i + 1] - r.seq_off[i]));
    }
    const int m = (int)run.size();
    if (m == 0) return PO_OK;
    std::vector<char> seq1d((size_t)s1o.back()), seq((size_t)co.back()), qual1d(o.fastq ? (size_t)s1o.back() : 0), qual(o.fastq ? (size_t)co.back() : 0);
    std::vector<int32_t> l1((size_t)m), l2((size_t)m), ln((size_t)m), st((size_t)m), qst(o.fastq ? 4 * (size_t)m : 0), ub;
    std::vector<double> idn((size_t)m);
    std::vector<float> lg(r.logits ? (size_t)lo[m_reads] * NOUT : 0);
    if (o.fastq && r.unbanded)
        for (int k = 0; k < m; ++k) ub.insert(ub.end(), r.unbanded + 4 * (size_t)run[k], r.unbanded + 4 * (size_t)run[k] + 4);
    const PoPairBasecallFastq fq = {o.band_size, ub.empty() ? nullptr : ub.data(), qual1d.data(), qual.data(), qst.data(), nullptr, nullptr, nullptr};
    const int rc = po_pair_basecall_body(w.st, w.stream, r.raw != nullptr, r.name, r.raw ? nullptr : sig.data(), lo.data(), m_reads, o.window,
                                         o.overlap, b->layers.data(), (int)b->layers.size(), b->weights.data(), (int64_t)b->weights.size(),
                                         o.max_windows_per_pass, idx.data(), m, o.reverse_complement, &o.pair, seq1d.data(), s1o.data(),
                                         l1.data(), l2.data(), idn.data(), seq.data(), co.data(), ln.data(), st.data(),
                                         r.logits ? lg.data() : nullptr, nullptr, o.fastq ? &fq : nullptr, nullptr);
    if (rc != PO_OK) return rc;
    for (int k = 0; k < m; ++k) {
        const int i = run[k];
        r.len1[i] = l1[k]; r.len2[i] = l2[k]; r.seq_len[i] = ln[k]; r.status[i] = st[k]; r.identity[i] = idn[k];
        for (int s = 0; s < 2; ++s) {
            const size_t room = (size_t)(s1o[2 * k + s + 1] - s1o[2 * k + s]);
            std::memcpy(r.seq1d + r.seq1d_off[2 * (size_t)i + s], seq1d.data() + s1o[2 * k + s], room);
            if (o.fastq) std::memcpy(r.qual1d + r.seq1d_off[2 * (size_t)i + s], qual1d.data() + s1o[2 * k + s], room);
        }
        std::memcpy(r.seq + r.seq_off[i], seq.data() + co[k], (size_t)(co[k + 1] - co[k]));
        if (o.fastq) {
            std::memcpy(r.qual + r.seq_off[i], qual.data() + co[k], (size_t)(co[k + 1] - co[k]));
            std::memcpy(r.qual_status + 4 * (size_t)i, qst.data() + 4 * (size_t)k, sizeof(int32_t) * 4);
        }
    }
    if (r.logits)
        for (int q = 0; q < m_reads; ++q) {
            const int rd = reads[kept_reads[q]];
            if (r.owner[rd] == g) std::memcpy(r.logits + r.off[rd] * NOUT, lg.data() + lo[q] * NOUT, sizeof(float) * NOUT * (size_t)(lo[q + 1] - lo[q]));
        }
    return PO_OK;
}

int run(Run& r, const char* name) {
    po_pair_basecaller* b = r.b;
    r.name = name;
    for (auto& s : b->stats) s = po_pair_basecaller::Stat();
    if (r.kept) std::fill(r.kept, r.kept + r.n_reads, (int64_t)-1);
    if (r.n_pairs == 0) return PO_OK;
    std::vector<int64_t> len((size_t)r.n_reads);
    for (int i = 0; i < r.n_reads; ++i) len[i] = r.off[i + 1] - r.off[i];
    const int ndev = (int)b->workers.size();
    r.first.resize((size_t)r.n_pairs);
    r.count.resize((size_t)r.n_pairs);
    // (a run with "no band" flags scores those items on the lattice without a band: its groups are sized for that workspace)
    const int ng = po_pair_basecall_group_plan(len.data(), r.n_reads, r.pair_idx, r.n_pairs, &b->opt.pair, b->opt.fastq,
                                               b->opt.fastq && r.unbanded ? 0 : b->opt.band_size, b->opt.resident_bytes, ndev,
                                               r.first.data(), r.count.data(), r.n_pairs);
    if (ng < 0) return ng;
    r.first.resize((size_t)ng);
    r.count.resize((size_t)ng);
    r.owner.assign((size_t)r.n_reads, -1);
    for (int g = 0; g < ng; ++g)
        for (int i = 2 * r.first[g]; i < 2 * (r.first[g] + r.count[g]); ++i)
            if (r.owner[r.pair_idx[i]] < 0) r.owner[r.pair_idx[i]] = g;
    return po_engine_run(b, ng, [&r](PoPairBasecallWorker& w, po_pair_basecaller::Stat& s, int g) { return run_group(r, w, s, g); });
}

// the checks of a run, before any work: pointers, tables from 0 and non-decreasing, every pair's reads and its room
int check_run(const std::string& me, const po_pair_basecaller* b, const void* data, const char* data_name, const int64_t* off,
              const char* off_name, int n_reads, const int32_t* pair_idx, int n_pairs, const void* seq1d, const int64_t* seq1d_off,
              const void* len1, const void* len2, const void* identity, const void* seq, const int64_t* seq_off, const void* seq_len,
              const void* status, const void* qual1d, const void* qual, const void* qual_status, bool empty_ok) {
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if (n_pairs < 0) return po_fail(PO_E_ARG, me + "n_pairs " + std::to_string(n_pairs));
    const bool fq = b->opt.fastq != 0;
    const struct { const void* p; const char* name; } ptrs[] = {
        {data, data_name}, {off, off_name}, {pair_idx, "pair_idx_h"}, {seq1d, "seq1d_h"}, {seq1d_off, "seq1d_off_h"}, {len1, "len1_h"},
        {len2, "len2_h"}, {identity, "identity_h"}, {seq, "seq_h"}, {seq_off, "seq_off_h"}, {seq_len, "seq_len_h"}, {status, "status_h"},
        {fq ? qual1d : &fq, "qual1d_h"}, {fq ? qual : &fq, "qual_h"}, {fq ? qual_status : &fq, "qual_status_h"}};
    for (const auto& a : ptrs)
        if (!a.p) return po_fail(PO_E_ARG, me + "null argument " + a.name);
    int rc = po_engine_check_from_zero(me, off, off_name);
    if (rc == PO_OK) rc = po_engine_check_from_zero(me, seq1d_off, "seq1d_off");
    if (rc == PO_OK) rc = po_engine_check_from_zero(me, seq_off, "seq_off");
    if (rc != PO_OK) return rc;
    for (int i = 0; i < n_reads; ++i) {
        const int64_t L = off[i + 1] - off[i];
        if (L < 0 || L > INT32_MAX) return po_fail(PO_E_ARG, me + "read " + std::to_string(i) + " has " + std::to_string(L) + " samples");
    }
    for (int i = 0; i < n_pairs; ++i) {
        for (int s = 0; s < 2; ++s) {
            const int64_t rd = pair_idx[2 * (size_t)i + s];
            if (rd < 0 || rd >= n_reads)
                return po_fail(PO_E_ARG, me + "pair " + std::to_string(i) + " names read " + std::to_string(rd) + " (reads 0 to " +
                               std::to_string(n_reads - 1) + ")");
            const int64_t L = off[rd + 1] - off[rd], room = seq1d_off[2 * (size_t)i + s + 1] - seq1d_off[2 * (size_t)i + s];
            if (L < 1 && !empty_ok)
                return po_fail(PO_E_ARG, me + "pair " + std::to_string(i) + ": read " + std::to_string(rd) + " has " + std::to_string(L) +
                               " samples (at least 1)");
            if (room < L)
                return po_fail(PO_E_CAP, me + "pair " + std::to_string(i) + ": read " + std::to_string(rd) + " has " + std::to_string(L) +
                               " samples and room for " + std::to_string(room) + " characters");
        }
        if (seq_off[i + 1] < seq_off[i])
            return po_fail(PO_E_CAP, me + "pair " + std::to_string(i) + " has room for " + std::to_string(seq_off[i + 1] - seq_off[i]) + " characters");
    }
    return PO_OK;
}

}  // namespace

extern "C" po_pair_basecaller* po_pair_basecaller_create(const int* devices, int ndev, const po_call_layer* layers_h, int n_layers,
                                                         const float* weights_h, int64_t n_weights,
                                                         const po_pair_basecaller_options* opt) {
    const std::string me = "po_pair_basecaller_create: ";
    po_set_error("");
    if (po_engine_check_devices(me, devices, ndev, layers_h, weights_h, opt) != PO_OK) return nullptr;
    // every argument error of the single-device entry, by that entry (no reads, no pairs: it stops after its checks)
    {
        const int64_t zero[1] = {0};
        char c = 0;
        int32_t w = 0;
        double d = 0;
        const float f = 0.f;
        const int rc = opt->fastq ? po_pair_basecall_fastq_batch_h(&f, zero, 0, opt->window, opt->overlap, layers_h, n_layers, weights_h,
                                                                  n_weights, opt->max_windows_per_pass, &w, 0, opt->reverse_complement,
                                                                  &opt->pair, &c, zero, &w, &w, &d, &c, zero, &w, &w, nullptr,
                                                                  opt->band_size, nullptr, &c, &c, &w, nullptr, nullptr, nullptr, nullptr)
                                  : po_pair_basecall_batch_h(&f, zero, 0, opt->window, opt->overlap, layers_h, n_layers, weights_h, n_weights,
                                                             opt->max_windows_per_pass, &w, 0, opt->reverse_complement, &opt->pair, &c, zero,
                                                             &w, &w, &d, &c, zero, &w, &w, nullptr, nullptr);
        if (rc != PO_OK) return nullptr;
    }
    if (po_engine_check_options("po_pair_basecaller_create", opt->scaling, opt->lo, opt->hi, opt->resident_bytes) != PO_OK) return nullptr;
    po_pair_basecaller* b = new po_pair_basecaller;
    b->opt = *opt;
    b->stats.resize((size_t)ndev);
    const int rc = po_engine_init(b, me, devices, ndev, layers_h, n_layers, weights_h, n_weights, [](PoPairBasecallWorker& w) -> PoBasecallPasses& {
        w.st = po_pair_basecall_resident_new();
        return po_pair_basecall_resident_net(w.st);
    });
    if (rc != PO_OK) {
        const std::string msg = po_last_error();
        po_pair_basecaller_destroy(b);
        po_fail(rc, msg);
        return nullptr;
    }
    return b;
}

extern "C" void po_pair_basecaller_destroy(po_pair_basecaller* b) {
    if (!b) return;
    po_engine_free(b, po_pair_basecall_resident_free);
    delete b;
}

extern "C" int po_pair_basecaller_run_f32(po_pair_basecaller* b, const float* signal_h, const int64_t* sig_off_h, int n_reads,
                                          const int32_t* pair_idx_h, int n_pairs, char* seq1d_h, const int64_t* seq1d_off_h,
                                          int32_t* len1_h, int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                                          int32_t* seq_len_h, int32_t* status_h, float* logits_h, const int32_t* unbanded_h,
                                          char* qual1d_h, char* qual_h, int32_t* qual_status_h) {
    const std::string me = "po_pair_basecaller_run_f32: ";
    po_set_error("");
    if (!b) return po_fail(PO_E_ARG, me + "null argument basecaller");
    const int rc = check_run(me, b, signal_h, "signal_h", sig_off_h, "sig_off", n_reads, pair_idx_h, n_pairs, seq1d_h, seq1d_off_h, len1_h,
                             len2_h, identity_h, seq_h, seq_off_h, seq_len_h, status_h, qual1d_h, qual_h, qual_status_h, false);
    if (rc != PO_OK) return rc;
    const bool fq = b->opt.fastq != 0;
    Run r;
    r.b = b; r.signal = signal_h; r.off = sig_off_h; r.n_reads = n_reads; r.pair_idx = pair_idx_h; r.n_pairs = n_pairs;
    r.seq1d = seq1d_h; r.seq1d_off = seq1d_off_h; r.len1 = len1_h; r.len2 = len2_h; r.identity = identity_h;
    r.seq = seq_h; r.seq_off = seq_off_h; r.seq_len = seq_len_h; r.status = status_h; r.logits = logits_h;
    r.unbanded = fq ? unbanded_h : nullptr; r.qual1d = fq ? qual1d_h : nullptr; r.qual = fq ? qual_h : nullptr;
    r.qual_status = fq ? qual_status_h : nullptr; r.kept = nullptr;
    return run(r, "po_pair_basecaller_run_f32");
}

extern "C" int po_pair_basecaller_run_raw(po_pair_basecaller* b, const int16_t* raw_h, const int64_t* raw_off_h, int n_reads,
                                          const double* offset_h, const double* alpha_h, const int32_t* pair_idx_h, int n_pairs,
                                          char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h,
                                          double* identity_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h,
                                          int32_t* status_h, float* logits_h, const int32_t* unbanded_h, char* qual1d_h, char* qual_h,
                                          int32_t* qual_status_h, int64_t* kept_h) {
    const std::string me = "po_pair_basecaller_run_raw: ";
    po_set_error("");
    if (!b) return po_fail(PO_E_ARG, me + "null argument basecaller");
    int rc = po_engine_check_raw_args(me, kept_h, b->opt.scaling, offset_h, alpha_h);
    if (rc != PO_OK) return rc;
    rc = check_run(me, b, raw_h, "raw_h", raw_off_h, "raw_off", n_reads, pair_idx_h, n_pairs, seq1d_h, seq1d_off_h, len1_h, len2_h,
                             identity_h, seq_h, seq_off_h, seq_len_h, status_h, qual1d_h, qual_h, qual_status_h, true);
    if (rc != PO_OK) return rc;
    const bool fq = b->opt.fastq != 0, cur = b->opt.scaling == PO_SCALE_CURRENT;
    Run r;
    r.b = b; r.raw = raw_h; r.off = raw_off_h; r.n_reads = n_reads; r.pair_idx = pair_idx_h; r.n_pairs = n_pairs;
    r.offset = cur ? offset_h : nullptr; r.alpha = cur ? alpha_h : nullptr;
    r.seq1d = seq1d_h; r.seq1d_off = seq1d_off_h; r.len1 = len1_h; r.len2 = len2_h; r.identity = identity_h;
    r.seq = seq_h; r.seq_off = seq_off_h; r.seq_len = seq_len_h; r.status = status_h; r.logits = logits_h;
    r.unbanded = fq ? unbanded_h : nullptr; r.qual1d = fq ? qual1d_h : nullptr; r.qual = fq ? qual_h : nullptr;
    r.qual_status = fq ? qual_status_h : nullptr; r.kept = kept_h;
    return run(r, "po_pair_basecaller_run_raw");
}

extern "C" int po_pair_basecaller_stats(po_pair_basecaller* b, int i, int64_t* pairs, int64_t* reads, int64_t* samples, int* groups,
                                        double* busy_ms) {
    if (!b || i < 0 || i >= (int)b->stats.size()) return po_fail(PO_E_ARG, "po_pair_basecaller_stats: worker " + std::to_string(i));
    const po_pair_basecaller::Stat& s = b->stats[(size_t)i];
    if (pairs) *pairs = s.pairs;
    if (reads) *reads = s.reads;
    if (samples) *samples = s.samples;
    if (groups) *groups = s.groups;
    if (busy_ms) *busy_ms = s.busy_ms;
    return PO_OK;
}
