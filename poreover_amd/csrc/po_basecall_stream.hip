// po_basecaller: `basecall` over one or several devices of a node, on the engine layer (po_engine.h).  Its
// items are reads; a group is a contiguous run of them (po_basecall_group_plan) and runs po_basecall_body — the body of
// po_basecall_batch_h / po_basecall_fastq_batch_h; a read's bits do not depend on its batch, DESIGN.md §16.3.  On the raw
// route the kept counts are per-read words, and a read that kept nothing is left out of the body's call.
#include <algorithm>
#include <cstring>

#include "po_engine.h"

struct PoBasecallWorker : PoEngineWorker {
    PoBasecallResident* st = nullptr;
};

struct po_basecaller : PoEngine<PoBasecallWorker> {
    std::string alphabet;
    bool has_alphabet = false;
    po_basecaller_options opt;
    int64_t budget_samples = 1;     // resident bytes / resident bytes per sample
    struct Stat { int64_t reads = 0, samples = 0; int groups = 0; double busy_ms = 0; };
    std::vector<Stat> stats;        // per worker, of the last run
};

// Groups are contiguous runs of reads in input order, of at most `group_samples` samples (at least one read: a longer
// read goes alone).  Writes first[g], count[g] for g < min(groups, cap) and returns the number of groups, or PO_E_ARG.
extern "C" int po_basecall_group_plan(const int64_t* len, int n, int64_t group_samples, int ndev, int32_t* first, int32_t* count,
                                      int cap) {
    (void)ndev;
    if (n < 0 || (n > 0 && !len) || group_samples < 1 || cap < 0 || (cap > 0 && (!first || !count)))
        return po_fail(PO_E_ARG, "po_basecall_group_plan: n " + std::to_string(n) + ", group_samples " + std::to_string(group_samples) +
                       ", cap " + std::to_string(cap));
    int g = 0, i = 0;
    while (i < n) {
        int64_t total = 0;
        const int f = i;
        while (i < n && (i == f || total + len[i] <= group_samples)) total += len[i++];
        if (g < cap) { first[g] = f; count[g] = i - f; }
        ++g;
    }
    return g;
}

// the group size of a run: min(resident budget, ceil(total / (2 ndev))) samples, 1 at least
extern "C" int64_t po_basecall_group_samples(int64_t total, int64_t budget_samples, int ndev) {
    const int64_t share = (total + 2 * (int64_t)ndev - 1) / (2 * (int64_t)ndev);
    return std::max<int64_t>(1, std::min(budget_samples, share));
}

namespace {

// resident device bytes per sample of one single-device call (basecall.py's _bytes_per_sample)
int64_t bytes_per_sample(const po_basecaller_options& o) {
    const int64_t rows = 1 << 20;
    int64_t b = 4 + NOUT * 4 + NOUT * 8 + 1;
    if (o.beam_width > 0) b += (int64_t)((po_beam1d_workspace_bytes(1, rows, rows, NOUT, o.beam_width, o.model) + rows - 1) / rows);
    if (o.fastq) {
        b += 4 + 4 + 1 + 1 + NOUT * 8 + 1 + (o.beam_width > 0 ? 4 : 0);
        b += (int64_t)((po_qual_workspace_bytes(1, rows, rows, rows, std::max(o.band_size, 0), o.model) + rows - 1) / rows);
    }
    return b;
}

struct Run {
    po_basecaller* b;
    // f32 route: signal / off; raw route: raw / off with offset / alpha
    const float* signal = nullptr;
    const int16_t* raw = nullptr;
    const int64_t* off = nullptr;
    const double *offset = nullptr, *alpha = nullptr;
    int n = 0;
    char* seq; const int64_t* seq_off; int32_t* seq_len; int32_t* status; float* logits;
    char* qual; int32_t* qual_status; int64_t* kept;
    std::vector<int32_t> first, count;
    const char* name = "";
};

// one group through the body on the worker's state and stream: c reads, their offsets from 0 in so; sig == NULL: the signal
// is in the state's buffer
int call_body(const Run& r, PoBasecallWorker& w, const float* sig, const std::vector<int64_t>& so, int c, char* seq,
              const std::vector<int64_t>& qo, int32_t* len, int32_t* st, float* logits, char* qual, int32_t* qst) {
    const po_basecaller* b = r.b;
    const po_basecaller_options& o = b->opt;
    const PoBasecallFastq fq = {o.band_size, qual, qst, nullptr, nullptr};
    return po_basecall_body(w.st, w.stream, sig == nullptr, r.name, sig, so.data(), c, o.window, o.overlap, b->layers.data(),
                            (int)b->layers.size(), b->weights.data(), (int64_t)b->weights.size(),
                            b->has_alphabet ? b->alphabet.c_str() : nullptr, o.kind, o.beam_width, o.model, o.max_windows_per_pass, seq,
                            qo.data(), len, st, logits, nullptr, o.fastq ? &fq : nullptr);
}

int run_group_f32(Run& r, PoBasecallWorker& w, int f, int c) {
    std::vector<int64_t> so((size_t)c + 1), qo((size_t)c + 1);
    for (int i = 0; i <= c; ++i) { so[i] = r.off[f + i] - r.off[f]; qo[i] = r.seq_off[f + i] - r.seq_off[f]; }
    return call_body(r, w, r.signal + r.off[f], so, c, r.seq + r.seq_off[f], qo, r.seq_len + f, r.status + f,
                      r.logits ? r.logits + r.off[f] * NOUT : nullptr, r.qual ? r.qual + r.seq_off[f] : nullptr,
                      r.qual_status ? r.qual_status + f : nullptr);
}

// raw route: prepare, leave out the reads that kept nothing, call, and put every read's results at its own raw offsets
int run_group_raw(Run& r, PoBasecallWorker& w, int f, int c) {
    const po_basecaller_options& o = r.b->opt;
    std::vector<int64_t> ro((size_t)c + 1), ko;
    for (int i = 0; i <= c; ++i) ro[i] = r.off[f + i] - r.off[f];
    int rc = w.prepare_raw(r.raw + r.off[f], ro.data(), c, r.offset ? r.offset + f : nullptr, r.offset ? r.alpha + f : nullptr,
                           o.scaling, o.lo, o.hi, r.name, po_basecall_resident_net(w.st), ko);
    if (rc != PO_OK) return rc;
    std::vector<int> idx;                 // the group's reads that kept a sample
    std::vector<int64_t> so(1, 0);
    for (int i = 0; i < c; ++i) {
        const int64_t k = ko[i + 1] - ko[i];
        r.kept[f + i] = k;
        r.seq_len[f + i] = 0;
        r.status[f + i] = PO_OK;
        if (r.qual_status) r.qual_status[f + i] = PO_OK;
        if (k > 0) { idx.push_back(i); so.push_back(so.back() + k); }
    }
    const int m = (int)idx.size();
    if (m == 0) return PO_OK;
    // the kept samples are back to back already (a read that kept nothing has no samples): so indexes the signal as it lies
    std::vector<char> seq((size_t)so[m]), qual(o.fastq ? (size_t)so[m] : 0);
    std::vector<int32_t> len((size_t)m), st((size_t)m), qst(o.fastq ? (size_t)m : 0);
    std::vector<float> lg(r.logits ? (size_t)so[m] * NOUT : 0);
    rc = call_body(r, w, nullptr, so, m, seq.data(), so, len.data(), st.data(), r.logits ? lg.data() : nullptr,
                   o.fastq ? qual.data() : nullptr, o.fastq ? qst.data() : nullptr);
    if (rc != PO_OK) return rc;
    for (int j = 0; j < m; ++j) {
        const int i = f + idx[j];
        const int64_t k = so[j + 1] - so[j];
        r.seq_len[i] = len[j];
        r.status[i] = st[j];
        std::memcpy(r.seq + r.seq_off[i], seq.data() + so[j], (size_t)std::max(len[j], 0));
        if (o.fastq) {
            r.qual_status[i] = qst[j];
            std::memcpy(r.qual + r.seq_off[i], qual.data() + so[j], (size_t)std::max(len[j], 0));
        }
        if (r.logits) std::memcpy(r.logits + r.off[i] * NOUT, lg.data() + so[j] * NOUT, sizeof(float) * NOUT * (size_t)k);
    }
    return PO_OK;
}

int run(Run& r, const char* name) {
    po_basecaller* b = r.b;
    r.name = name;
    for (auto& s : b->stats) s = po_basecaller::Stat();
    if (r.n == 0) return PO_OK;
    std::vector<int64_t> len((size_t)r.n);
    for (int i = 0; i < r.n; ++i) len[i] = r.off[i + 1] - r.off[i];
    const int ndev = (int)b->workers.size();
    const int64_t gs = po_basecall_group_samples(r.off[r.n], b->budget_samples, ndev);
    r.first.resize((size_t)r.n);
    r.count.resize((size_t)r.n);
    const int ng = po_basecall_group_plan(len.data(), r.n, gs, ndev, r.first.data(), r.count.data(), r.n);
    if (ng < 0) return ng;
    r.first.resize((size_t)ng);
    r.count.resize((size_t)ng);
    return po_engine_run(b, ng, [&r](PoBasecallWorker& w, po_basecaller::Stat& s, int g) {
        const int f = r.first[g], c = r.count[g];
        s.reads += c;
        s.samples += r.off[f + c] - r.off[f];
        return r.raw ? run_group_raw(r, w, f, c) : run_group_f32(r, w, f, c);
    });
}

// the offsets' and pointers' checks of a run, before any work: tables from 0, non-decreasing, room for every read
int check_run(const std::string& me, const void* data, const char* data_name, const int64_t* off, const char* off_name, int n,
              const void* seq, const int64_t* seq_off, const void* seq_len, const void* status, bool fastq, const void* qual,
              const void* qual_status, bool empty_ok) {
    if (n < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n));
    const char* null = !data ? data_name : !off ? off_name : !seq ? "seq_h" : !seq_off ? "seq_off_h" : !seq_len ? "seq_len_h" :
                       !status ? "status_h" : fastq && !qual ? "qual_h" : fastq && !qual_status ? "qual_status_h" : nullptr;
    if (null) return po_fail(PO_E_ARG, me + "null argument " + null);
    int rc = po_engine_check_from_zero(me, off, off_name);
    if (rc == PO_OK) rc = po_engine_check_from_zero(me, seq_off, "seq_off");
    if (rc != PO_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const int64_t L = off[i + 1] - off[i];
        if (L < (empty_ok ? 0 : 1) || L > INT32_MAX)
            return po_fail(PO_E_ARG, me + "read " + std::to_string(i) + " has " + std::to_string(L) + " samples");
        if (seq_off[i + 1] - seq_off[i] < L)
            return po_fail(PO_E_CAP, me + "read " + std::to_string(i) + " has " + std::to_string(L) + " samples and room for " +
                           std::to_string(seq_off[i + 1] - seq_off[i]) + " characters");
    }
    return PO_OK;
}

}  // namespace

extern "C" po_basecaller* po_basecaller_create(const int* devices, int ndev, const po_call_layer* layers_h, int n_layers,
                                               const float* weights_h, int64_t n_weights, const char* alphabet,
                                               const po_basecaller_options* opt) {
    const std::string me = "po_basecaller_create: ";
    po_set_error("");
    if (po_engine_check_devices(me, devices, ndev, layers_h, weights_h, opt) != PO_OK) return nullptr;
    // every argument error of the single-device entry, by that entry (no reads: it stops after its checks)
    {
        const int64_t zero = 0;
        char c = 0;
        int32_t w = 0;
        const float f = 0.f;
        const int rc = opt->fastq ? po_basecall_fastq_batch_h(&f, &zero, 0, opt->window, opt->overlap, layers_h, n_layers, weights_h, n_weights,
                                                             alphabet, opt->kind, opt->beam_width, opt->model, opt->max_windows_per_pass, &c,
                                                             &zero, &w, &w, nullptr, opt->band_size, &c, &w, nullptr, nullptr, nullptr)
                                  : po_basecall_batch_h(&f, &zero, 0, opt->window, opt->overlap, layers_h, n_layers, weights_h, n_weights,
                                                        alphabet, opt->kind, opt->beam_width, opt->model, opt->max_windows_per_pass, &c, &zero,
                                                        &w, &w, nullptr, nullptr);
        if (rc != PO_OK) return nullptr;
    }
    if (po_engine_check_options("po_basecaller_create", opt->scaling, opt->lo, opt->hi, opt->resident_bytes) != PO_OK) return nullptr;
    po_basecaller* b = new po_basecaller;
    if (alphabet) { b->alphabet = alphabet; b->has_alphabet = true; }
    b->opt = *opt;
    b->budget_samples = std::max<int64_t>(1, (opt->resident_bytes ? opt->resident_bytes : DEFAULT_RESIDENT) / bytes_per_sample(*opt));
    b->stats.resize((size_t)ndev);
    const int rc = po_engine_init(b, me, devices, ndev, layers_h, n_layers, weights_h, n_weights, [](PoBasecallWorker& w) -> PoBasecallPasses& {
        w.st = po_basecall_resident_new();
        return po_basecall_resident_net(w.st);
    });
    if (rc != PO_OK) {
        const std::string msg = po_last_error();
        po_basecaller_destroy(b);
        po_fail(rc, msg);
        return nullptr;
    }
    return b;
}

extern "C" void po_basecaller_destroy(po_basecaller* b) {
    if (!b) return;
    po_engine_free(b, po_basecall_resident_free);
    delete b;
}

extern "C" int po_basecaller_run_f32(po_basecaller* b, const float* signal_h, const int64_t* sig_off_h, int n_reads, char* seq_h,
                                     const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h, float* logits_h, char* qual_h,
                                     int32_t* qual_status_h) {
    const std::string me = "po_basecaller_run_f32: ";
    po_set_error("");
    if (!b) return po_fail(PO_E_ARG, me + "null argument basecaller");
    const int rc = check_run(me, signal_h, "signal_h", sig_off_h, "sig_off", n_reads, seq_h, seq_off_h, seq_len_h, status_h, b->opt.fastq != 0,
                             qual_h, qual_status_h, false);
    if (rc != PO_OK) return rc;
    Run r;
    r.b = b; r.signal = signal_h; r.off = sig_off_h; r.n = n_reads;
    r.seq = seq_h; r.seq_off = seq_off_h; r.seq_len = seq_len_h; r.status = status_h; r.logits = logits_h;
    r.qual = b->opt.fastq ? qual_h : nullptr; r.qual_status = b->opt.fastq ? qual_status_h : nullptr; r.kept = nullptr;
    return run(r, "po_basecaller_run_f32");
}

extern "C" int po_basecaller_run_raw(po_basecaller* b, const int16_t* raw_h, const int64_t* raw_off_h, int n_reads, const double* offset_h,
                                     const double* alpha_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                                     float* logits_h, char* qual_h, int32_t* qual_status_h, int64_t* kept_h) {
    const std::string me = "po_basecaller_run_raw: ";
    po_set_error("");
    if (!b) return po_fail(PO_E_ARG, me + "null argument basecaller");
    int rc = po_engine_check_raw_args(me, kept_h, b->opt.scaling, offset_h, alpha_h);
    if (rc != PO_OK) return rc;
    rc = check_run(me, raw_h, "raw_h", raw_off_h, "raw_off", n_reads, seq_h, seq_off_h, seq_len_h, status_h, b->opt.fastq != 0,
                             qual_h, qual_status_h, true);
    if (rc != PO_OK) return rc;
    Run r;
    r.b = b; r.raw = raw_h; r.off = raw_off_h; r.n = n_reads;
    r.offset = b->opt.scaling == PO_SCALE_CURRENT ? offset_h : nullptr;
    r.alpha = b->opt.scaling == PO_SCALE_CURRENT ? alpha_h : nullptr;
    r.seq = seq_h; r.seq_off = seq_off_h; r.seq_len = seq_len_h; r.status = status_h; r.logits = logits_h;
    r.qual = b->opt.fastq ? qual_h : nullptr; r.qual_status = b->opt.fastq ? qual_status_h : nullptr; r.kept = kept_h;
    return run(r, "po_basecaller_run_raw");
}

extern "C" int po_basecaller_stats(po_basecaller* b, int i, int64_t* reads, int64_t* samples, int* groups, double* busy_ms) {
    if (!b || i < 0 || i >= (int)b->stats.size()) return po_fail(PO_E_ARG, "po_basecaller_stats: worker " + std::to_string(i));
    const po_basecaller::Stat& s = b->stats[(size_t)i];
    if (reads) *reads = s.reads;
    if (samples) *samples = s.samples;
    if (groups) *groups = s.groups;
    if (busy_ms) *busy_ms = s.busy_ms;
    return PO_OK;
}
