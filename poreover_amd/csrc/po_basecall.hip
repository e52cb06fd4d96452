// `basecall`: scaled signals in, decoded strings out, in one device-resident pass.
//
// What `call` followed by `decode` does in two commands — the network's forward pass (po_call.hip), the log-softmax of its
// logits (po_ingest.hip) and Viterbi or the 1-D beam search (po_viterbi.hip, po_beam1d.hip) — with the per-frame data staying
// on the device in between, and with windows that may overlap: a read of L samples is cut into windows of W samples every
// S = W - O samples, each window runs through the network from a zero state as in `call`, and every output frame is taken
// from the window whose middle it lies in (po_basecall_plan.h).  O = 0 is `call`'s windowing.
//
//   window_gather_kernel   the window-major [n_win][W] f32 input of a pass from the ragged signals, zeros past a read's end
//   window_stitch_kernel   the kept frames' logits of a pass to their read-major rows
//
// Both are streaming copies, one lane per f32 value of the pass, consecutive lanes on consecutive addresses on the pass's
// side and on runs of consecutive addresses on the reads' side; every output value has one writer.
//
// The buffers of the network part and its pass loop (gather -> po_call_batch -> stitch) are PoBasecallPasses
// (po_basecall_pass.h), defined here and run by po_pair_basecall.hip too: one loop, the same logits bits in both.
//
// po_basecall_fastq_batch_h (`basecall --fastq`) is the same body followed by the quality stages on the
// same stream: FastqStages below enqueues them (kernels: po_fastq.hip, the lattice: po_qual.hip) on the table and the
// strings the decoder left on the device.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "po_basecall_pass.h"
#include "po_fastq_rules.h"
#include "po_fastq_stages.h"

namespace {

constexpr int NOUT = 5;     // Dense outputs (A, C, G, T, blank)
constexpr int TILE = 16;    // windows per recurrence workgroup of po_call_batch: a pass holds whole tiles

struct WinArgs {
    const int64_t* sig_off;    // [n_reads + 1] sample (= row) offsets
    const int64_t* win_off;    // [n_reads + 1] first global window of each read
    const int32_t* win_read;   // [windows] read of each global window
    int64_t w0;                // first global window of the pass
    int64_t count;             // values of the pass: windows * W (gather), windows * W * NOUT (stitch)
    int W, S, O;
};

// out[(g - w0) * W + k] = sample j * S + k of the read of global window g (its j-th), or 0 past the read's end
__global__ __launch_bounds__(256) void window_gather_kernel(WinArgs a, const float* __restrict__ signal, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = a.w0 + i / a.W;
        const int k = (int)(i % a.W);
        const int r = a.win_read[g];
        const int64_t s0 = a.sig_off[r], L = a.sig_off[r + 1] - s0;
        const int64_t t = (g - a.win_off[r]) * a.S + k;
        out[i] = t < L ? signal[s0 + t] : 0.f;
    }
}

// logits[(sig_off[r] + t) * NOUT + c] = pass[((g - w0) * W + k) * NOUT + c] for the frames t = j * S + k that window g keeps
__global__ __launch_bounds__(256) void window_stitch_kernel(WinArgs a, const float* __restrict__ pass, float* __restrict__ logits) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / NOUT;
        const int c = (int)(i - f * NOUT);
        const int64_t g = a.w0 + f / a.W;
        const int k = (int)(f % a.W);
        const int r = a.win_read[g];
        const int64_t s0 = a.sig_off[r], L = a.sig_off[r + 1] - s0;
        const int64_t j = g - a.win_off[r];
        const int64_t t = j * a.S + k;
        int64_t lo, hi;
        po_basecall_keep(j, a.win_off[r + 1] - a.win_off[r], L, a.S, a.O, &lo, &hi);
        if (t >= lo && t < hi && t < L) logits[(s0 + t) * NOUT + c] = pass[i];
    }
}

unsigned grid_for(int64_t count) { return (unsigned)std::min<int64_t>((count + 255) / 256, 256 * 64); }

}  // namespace

int PoBasecallPasses::up(const PoBasecallPlan& plan, const float* signal_h, const int64_t* sig_off_h, int n_reads, int window,
                         const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                         int max_windows_per_pass) {
    // ---- windows per pass: as many as ~4 GiB of pass buffers hold (po_call_batch_h's rule), whole recurrence tiles
    // (the part of the workspace that grows with the windows: under PO_CALL_BF16 the size of no windows is the bf16 copy of W,
    // which a pass holds once; 0 under PO_CALL_F32)
    const size_t ws_const = po_call_workspace_bytes(0, window, layers_h, n_layers);
    const size_t per_window = po_call_workspace_bytes(1, window, layers_h, n_layers) - ws_const + (size_t)window * NOUT * 4 * 2 +
                              (size_t)window * 4;
    chunk = (int64_t)std::max<size_t>(1, ((size_t)4 << 30) / per_window);
    if (chunk >= TILE) chunk = chunk / TILE * TILE;
    if (max_windows_per_pass > 0) chunk = std::min<int64_t>(chunk, max_windows_per_pass);   // (a smaller bound: the tests')
    chunk = std::min<int64_t>(chunk, plan.windows);
    const int64_t Mc = chunk * window;
    ws_bytes = po_call_workspace_bytes((int)chunk, window, layers_h, n_layers);
    if (!w_up) PO_HIPCHK(w.up(weights_h, (size_t)n_weights * 4));
    PO_HIPCHK(sig.up(signal_h, (size_t)plan.rows * 4));             // each read's signal once, whatever the overlap (NULL: it is there)
    PO_HIPCHK(sig_off.up(sig_off_h, sizeof(int64_t) * ((size_t)n_reads + 1)));
    PO_HIPCHK(win_off.up(plan.win_off.data(), sizeof(int64_t) * plan.win_off.size()));
    PO_HIPCHK(win_read.up(plan.win_read.data(), sizeof(int32_t) * plan.win_read.size()));
    PO_HIPCHK(win.up(nullptr, (size_t)Mc * 4));
    PO_HIPCHK(prob.up(nullptr, (size_t)Mc * NOUT * 4));
    PO_HIPCHK(plog.up(nullptr, (size_t)Mc * NOUT * 4));
    PO_HIPCHK(ws.up(nullptr, ws_bytes));
    PO_HIPCHK(logits.up(nullptr, (size_t)plan.rows * NOUT * 4));
    return PO_OK;
}

int PoBasecallPasses::run(const PoBasecallPlan& plan, int window, int overlap, const po_call_layer* layers_h, int n_layers,
                          int64_t n_weights, hipStream_t stream, float* stage_ms_h, PoSpans& stitch) {
    WinArgs a;
    a.sig_off = sig_off; a.win_off = win_off; a.win_read = win_read;
    a.W = window; a.S = plan.stride; a.O = overlap;
    for (int64_t w0 = 0; w0 < plan.windows; w0 += chunk) {
        const int nc = (int)std::min<int64_t>(chunk, plan.windows - w0);
        a.w0 = w0;
        a.count = (int64_t)nc * window;
        PO_HIPCHK(stitch.mark(stream));
        hipLaunchKernelGGL(window_gather_kernel, dim3(grid_for(a.count)), dim3(256), 0, stream, a, sig.as<float>(), win.as<float>());
        PO_HIPCHK(stitch.mark(stream));
        PO_HIPCHK(hipGetLastError());
        const int rc = po_call_batch(win, nc, window, layers_h, n_layers, w, n_weights, prob, plog, ws, ws_bytes, stream, stage_ms_h);
        if (rc != PO_OK) return rc;
        a.count = (int64_t)nc * window * NOUT;
        PO_HIPCHK(stitch.mark(stream));
        hipLaunchKernelGGL(window_stitch_kernel, dim3(grid_for(a.count)), dim3(256), 0, stream, a, plog.as<float>(), logits.as<float>());
        PO_HIPCHK(stitch.mark(stream));
        PO_HIPCHK(hipGetLastError());
    }
    return PO_OK;
}

namespace {

typedef PoBasecallFastq FastqOut;

// the decode's strings as the quality stages read them: a PoSeqOut of this call, or buffers the caller holds (po_fastq_tables)
struct FqStrings {
    const char* seq; const int64_t* off; const int32_t* len; const int32_t* status;   // device
    size_t cap;                                                                       // bytes of seq: off[n]
};
FqStrings fq_strings(const PoSeqOut& out) { return {out.seq.as<char>(), out.off.as<int64_t>(), out.len.as<int32_t>(), out.status.as<int32_t>(), out.cap}; }

// The quality stages, enqueued behind the decoder on its stream: the table dy, the strings of `out` and
// (Viterbi) the frame map stay where they are; lengths, statuses, modes and offsets are the only words that cross.
// po_basecall_body runs them behind its decoder, po_fastq_tables on tables and strings of the caller's.
struct FastqStages {
    PoDev map, vseq, vlen, vst, mode, consumed, guide, labels, label_off, label_off_u, odds, logp, qst, qual, wsv, wsq;
    PoFqAligner al;   // the pairs that need an alignment (po_fastq_stages.h)
    std::vector<int64_t> label_off_h, label_off_u_h;   // the dense label layout of the banded call, of the one without a band
    int64_t total_b = 0, total_u = 0;                  // labels of the first call (all of them without flags), of the second
    int32_t* called_len = nullptr;   // device: the Viterbi call's lengths
    const int32_t* mapp = nullptr;   // device: the frame map of the Viterbi call: `map`, or the caller's
    // The Viterbi call with its frame map is the decode itself only for Viterbi of PO_KIND_POREOVER.  For PO_KIND_BONITO the
    // map follows the reference's get_sequence_mapping, whose count can differ from the string's; po_viterbi_batch reports
    // that as PO_E_ARG in the read's status (such a read gets the diagonal, as in quality.call_guides), and the decode's
    // own status has to stay what po_basecall_batch_h gives: the map then comes from a second Viterbi call, as for the beam.
    // (po_fastq_tables' caller may pass the map-making call's strings, status and map: no second call for either kind.)
    bool second = false;
    bool align = false;   // the scored strings are not the Viterbi call's: the pairs that differ go to the aligner
    int qual_route = PO_QUAL_ROUTE_GENERAL;   // the lattice's kernels: po_qual_batch's (po_fastq_tables: po_qual_entry_route())

    // before the decoder: the buffers whose size is known from the signals.  caller_map: the frame map, where the caller has it
    int prepare(int n, int64_t rows, int kind, bool second_, bool align_, size_t cap, const int32_t* caller_map = nullptr) {
        al.reset();
        second = second_;
        align = align_;
        if (!caller_map) PO_HIPCHK(map.up(nullptr, sizeof(int32_t) * (size_t)rows));
        mapp = caller_map ? caller_map : map.as<int32_t>();
        PO_HIPCHK(mode.up(nullptr, sizeof(int32_t) * n));
        PO_HIPCHK(guide.up(nullptr, sizeof(int32_t) * (size_t)rows));
        PO_HIPCHK(qst.up(nullptr, sizeof(int32_t) * n));
        PO_HIPCHK(logp.up(nullptr, sizeof(double) * n));
        PO_HIPCHK(qual.up(nullptr, cap));
        if (second) {
            PO_HIPCHK(vseq.up(nullptr, cap));
            PO_HIPCHK(vlen.up(nullptr, sizeof(int32_t) * n));
            PO_HIPCHK(vst.up(nullptr, sizeof(int32_t) * n));
            PO_HIPCHK(wsv.up(nullptr, po_viterbi_workspace_bytes(n, rows, NOUT, kind)));
        }
        if (align) PO_HIPCHK(consumed.up(nullptr, sizeof(int32_t) * (size_t)rows));
        return PO_OK;
    }

    // steps 1 to 3: the Viterbi call with its map, the pairs that need an alignment, the guide
    int guides(const char* me, int band_size, const double* dy, const int64_t* dsoff, int n, int64_t rows, const char* alphabet,
               int kind, const FqStrings& out, hipStream_t stream) {
        int rc;
        const char* called = out.seq;
        const int32_t* called_st = out.status;
        called_len = const_cast<int32_t*>(out.len);
        if (second) {
            rc = po_viterbi_batch(dy, dsoff, n, NOUT, alphabet, kind, nullptr, vseq, out.off, vlen, map, vst, wsv,
                                  po_viterbi_workspace_bytes(n, rows, NOUT, kind), stream);
            if (rc != PO_OK) return rc;
            called = vseq.as<char>();
            called_st = vst.as<int32_t>();
            called_len = vlen.as<int32_t>();
        }
        po_launch_fastq_mode(out.seq, out.len, called, called_len, called_st, out.off, n, mode, stream);
        PO_HIPCHK(hipGetLastError());
        if (align) {
            std::vector<int32_t> h(3 * (size_t)n);   // mode | scored lengths | called lengths
            PO_HIPCHK(hipMemcpyAsync(h.data(), mode.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
            PO_HIPCHK(hipMemcpyAsync(h.data() + n, out.len, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
            PO_HIPCHK(hipMemcpyAsync(h.data() + 2 * n, vlen.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
            PO_HIPCHK(hipStreamSynchronize(stream));
            for (int i = 0; i < n; ++i)
                if (h[i] == PO_FQ_ALIGN) al.add(i, h[2 * (size_t)n + i], h[(size_t)n + i]);
            const int m = al.m();
            if (m > 0) {
                rc = al.up(me);
                if (rc != PO_OK) return rc;
                po_launch_fastq_gather(called, out.seq, out.off, al.pair_read, 2, al.pair_off, 2 * m, al.so.back(), al.pair_seq, stream);
                PO_HIPCHK(hipGetLastError());
                rc = al.run(stream);
                if (rc != PO_OK) return rc;
                po_launch_fastq_consumed(al.aln1, al.aln2, al.aln_off, al.ncol, al.ast, m, al.pair_read, dsoff, called_len, out.len, consumed, mode, stream);
                PO_HIPCHK(hipGetLastError());
            }
        }
        if (band_size > 0) {
            po_launch_fastq_guide(mapp, align ? consumed.as<int32_t>() : nullptr, dsoff, n, rows, called_len, out.len, mode,
                                  guide, stream);
            PO_HIPCHK(hipGetLastError());
        }
        return PO_OK;
    }

    // steps 4 to 6: dense labels, the lattice on the resident table, Phred characters at the strings' offsets in `qual_out`.
    // unbanded_h (or NULL): with a band, a flagged read is scored in a second po_qual_batch call without one and has L = 0
    // in the first, as the pair stages do it (po_pair_fastq_plan.h): the second call's labels and odds lie behind the
    // first's, and the read's status is the second call's.  Without flags this is one call, as it always was.
    int lattice(int band_size, const int32_t* unbanded_h, const double* dy, const int64_t* dsoff, int n, int64_t rows, int64_t max_rows,
                const char* alphabet, int kind, const FqStrings& out, char* qual_out, hipStream_t stream) {
        std::vector<int32_t> len((size_t)n);
        PO_HIPCHK(hipMemcpyAsync(len.data(), out.len, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipStreamSynchronize(stream));
        bool split = false;
        for (int i = 0; unbanded_h && band_size > 0 && i < n; ++i) split = split || unbanded_h[i] != 0;
        label_off_h.assign((size_t)n + 1, 0);
        label_off_u_h.assign((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) {
            const bool u = split && unbanded_h[i] != 0;
            label_off_h[(size_t)i + 1] = label_off_h[i] + (u ? 0 : std::max(len[i], 0));
            label_off_u_h[(size_t)i + 1] = label_off_u_h[i] + (u ? std::max(len[i], 0) : 0);
        }
        total_b = label_off_h[n];
        total_u = label_off_u_h[n];
        const int64_t total = total_b + total_u;
        const int model = kind == PO_KIND_BONITO ? PO_MODEL_MERGE : PO_MODEL_CTC;   // the tree model of the decoder's kind
        size_t wqb = po_qual_workspace_bytes(n, rows, max_rows, total_b, band_size, model);
        if (split) wqb = std::max(wqb, po_qual_workspace_bytes(n, rows, max_rows, total_u, 0, model));
        PO_HIPCHK(label_off.up(label_off_h.data(), sizeof(int64_t) * label_off_h.size()));
        if (split) {   // (the statuses of the call without a band: a second half, before anything is written to the first)
            PO_HIPCHK(label_off_u.up(label_off_u_h.data(), sizeof(int64_t) * label_off_u_h.size()));
            PO_HIPCHK(qst.up(nullptr, sizeof(int32_t) * 2 * (size_t)n));
        }
        PO_HIPCHK(labels.up(nullptr, (size_t)total));
        PO_HIPCHK(odds.up(nullptr, sizeof(double) * 5 * (size_t)total));
        PO_HIPCHK(wsq.up(nullptr, wqb));
        for (int u = 0; u < (split ? 2 : 1); ++u) {
            const int64_t tot = u ? total_u : total_b, at = u ? total_b : 0;
            const int64_t* lo = u ? label_off_u.as<int64_t>() : label_off.as<int64_t>();
            const int band = u ? 0 : band_size;
            char* lab = labels.as<char>() + at;
            double* od = odds.as<double>() + at * 5;
            int32_t* q = qst.as<int32_t>() + (u ? n : 0);
            po_launch_fastq_gather(out.seq, out.seq, out.off, nullptr, 1, lo, n, tot, lab, stream);
            PO_HIPCHK(hipGetLastError());
            const int rc = po_qual_batch_route(dy, dsoff, n, NOUT, alphabet, model, lab, lo, band > 0 ? guide.as<int32_t>() : nullptr, band,
                                               od, logp, q, wsq, wqb, stream, qual_route);
            if (rc != PO_OK) return rc;
            po_launch_fastq_phred(od, lab, lo, q, out.off, n, tot, alphabet, qual_out, stream);
            PO_HIPCHK(hipGetLastError());
        }
        for (int i = 0; split && i < n; ++i)   // (the retry's few reads: a word each)
            if (unbanded_h[i] != 0)
                PO_HIPCHK(hipMemcpyAsync(qst.as<int32_t>() + i, qst.as<int32_t>() + n + i, sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
        return PO_OK;
    }

    // after the synchronise: the characters, the statuses and (where asked for) the odds and the guide
    int down(const FastqOut& fq, const int64_t* seq_off_h, int n, int64_t rows, size_t cap) {
        PO_HIPCHK(qual.down(fq.qual_h, cap));
        PO_HIPCHK(qst.down(fq.qual_status_h, sizeof(int32_t) * n));
        if (fq.guide_h && fq.band_size > 0) PO_HIPCHK(guide.down(fq.guide_h, sizeof(int32_t) * (size_t)rows));
        if (fq.odds_h) {   // dense on the device, at the strings' offsets in the caller's table
            const int64_t total = label_off_h[n];
            std::vector<double> dense((size_t)total * 5);
            PO_HIPCHK(odds.down(dense.data(), sizeof(double) * dense.size()));
            for (int i = 0; i < n; ++i) {
                const int64_t L = label_off_h[(size_t)i + 1] - label_off_h[i];
                if (L > 0) std::memcpy(fq.odds_h + seq_off_h[i] * 5, dense.data() + label_off_h[i] * 5, sizeof(double) * 5 * (size_t)L);
            }
        }
        return PO_OK;
    }
};

}  // namespace

// everything a call keeps on the device: one call's, or a po_basecaller worker's between groups and runs
struct PoBasecallResident {
    PoBasecallPasses net;
    PoDev dy, dws2;
    PoSeqOut out;
    FastqStages fs;
};

PoBasecallResident* po_basecall_resident_new() { return new PoBasecallResident; }
void po_basecall_resident_free(PoBasecallResident* st) { delete st; }
PoBasecallPasses& po_basecall_resident_net(PoBasecallResident* st) { return st->net; }

// po_basecall_batch_h (fq == NULL) and po_basecall_fastq_batch_h under their own names, and a po_basecaller's groups
int po_basecall_body(PoBasecallResident* st, hipStream_t stream, bool signal_resident, const char* name, const float* signal_h,
                     const int64_t* sig_off_h, int n_reads, int window, int overlap, const po_call_layer* layers_h, int n_layers,
                     const float* weights_h, int64_t n_weights, const char* alphabet, int kind, int beam_width, int model,
                     int max_windows_per_pass, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                     float* logits_h, float* stage_ms_h, const PoBasecallFastq* fq) {
    const std::string me = std::string(name) + ": ";
    const int n_stages = fq ? 8 : 6;
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if ((!signal_h && !signal_resident) || !sig_off_h || !layers_h || !weights_h || !seq_h || !seq_off_h || !seq_len_h || !status_h)
        return po_fail(PO_E_ARG, me + "null argument " +
                       (!signal_h && !signal_resident ? "signal_h" : !sig_off_h ? "sig_off_h" : !layers_h ? "layers_h" : !weights_h ? "weights_h" :
                        !seq_h ? "seq_h" : !seq_off_h ? "seq_off_h" : !seq_len_h ? "seq_len_h" : "status_h"));
    if (fq && (!fq->qual_h || !fq->qual_status_h))
        return po_fail(PO_E_ARG, me + "null argument " + (!fq->qual_h ? "qual_h" : "qual_status_h"));
    PoBasecallPlan plan;
    std::string err;
    int rc = po_basecall_make_plan(sig_off_h, n_reads, window, overlap, seq_off_h, &plan, &err, name);
    if (rc != PO_OK) return po_fail(rc, err);
    if (kind == PO_KIND_FLIPFLOP || model == PO_MODEL_FLIPFLOP)
        return po_fail(PO_E_UNSUPPORTED, me + "flip-flop decoding (kind " + std::to_string(kind) + ", model " +
                       std::to_string(model) + "): the network's output is a CTC table");
    if (kind != PO_KIND_POREOVER && kind != PO_KIND_BONITO) return po_fail(PO_E_ARG, me + "kind " + std::to_string(kind));
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, me + "model " + std::to_string(model));
    if (beam_width > 64) return po_fail(PO_E_ARG, me + "beam_width " + std::to_string(beam_width) + " (at most 64)");
    if (alphabet && std::strlen(alphabet) != NOUT - 1)
        return po_fail(PO_E_ARG, me + "alphabet \"" + alphabet + "\" (4 symbols: the network has 5 outputs)");
    // the model and the weights' length: po_call_batch's own checks, which come before it looks at a buffer (no windows:
    // the pointers are not followed)
    rc = po_call_batch(weights_h, 0, window, layers_h, n_layers, weights_h, n_weights, (float*)weights_h, nullptr, nullptr, 0,
                       nullptr, nullptr);
    if (rc != PO_OK) return rc;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + n_stages, 0.f);
    if (n_reads == 0) return PO_OK;

    const int64_t rows = plan.rows;
    PoBasecallPasses& net = st->net;
    PoDev &dy = st->dy, &dws2 = st->dws2;
    PoSeqOut& out = st->out;
    rc = net.up(plan, signal_resident ? nullptr : signal_h, sig_off_h, n_reads, window, layers_h, n_layers, weights_h, n_weights, max_windows_per_pass);
    if (rc != PO_OK) return rc;
    const PoDev &dsoff = net.sig_off, &dlog = net.logits;   // resident: the stitched logits ...
    PO_HIPCHK(dy.up(nullptr, (size_t)rows * NOUT * 8));     // ... and the f64 log-probability table
    PO_HIPCHK(out.up(seq_off_h, n_reads));
    const size_t wsb2 = beam_width <= 0 ? po_viterbi_workspace_bytes(n_reads, rows, NOUT, kind)
                                        : po_beam1d_workspace_bytes(n_reads, rows, plan.max_rows, NOUT, beam_width, model);
    PO_HIPCHK(dws2.up(nullptr, wsb2));
    FastqStages& fs = st->fs;
    if (fq) {
        rc = fs.prepare(n_reads, rows, kind, beam_width > 0 || kind != PO_KIND_POREOVER, beam_width > 0, out.cap);
        if (rc != PO_OK) return rc;
    }

    PoSpans stitch(stage_ms_h != nullptr), decode(stage_ms_h != nullptr), guides(stage_ms_h != nullptr), lattice(stage_ms_h != nullptr);
    rc = net.run(plan, window, overlap, layers_h, n_layers, n_weights, stream, stage_ms_h, stitch);
    if (rc != PO_OK) return rc;
    // the reference's f32 log-softmax of the logits, widened (decode.py:34-39), then the decoder over all reads at once
    PO_HIPCHK(stitch.mark(stream));
    rc = po_launch_ingest(dlog, dsoff, n_reads, NOUT, PO_INGEST_LOGITS_F32, nullptr, 0, rows, dy, stream);
    if (rc != PO_OK) return po_fail(rc, me + "ingest");
    PO_HIPCHK(stitch.mark(stream));
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(decode.mark(stream));
    rc = beam_width <= 0 ? po_viterbi_batch(dy, dsoff, n_reads, NOUT, alphabet, kind, nullptr, out.seq, out.off, out.len,
                                            fq && !fs.second ? fs.map.as<int32_t>() : nullptr, out.status, dws2, wsb2, stream)
                         : po_beam1d_batch(dy, dsoff, n_reads, NOUT, alphabet, beam_width, model, out.seq, out.off, out.len,
                                           out.status, dws2, wsb2, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(decode.mark(stream));
    if (fq) {   // the quality stages, on the table, the strings and (Viterbi) the frame map the decoder left on the device
        PO_HIPCHK(guides.mark(stream));
        rc = fs.guides(name, fq->band_size, dy, dsoff, n_reads, rows, alphabet, kind, fq_strings(out), stream);
        if (rc != PO_OK) return rc;
        PO_HIPCHK(guides.mark(stream));
        PO_HIPCHK(lattice.mark(stream));
        rc = fs.lattice(fq->band_size, nullptr, dy, dsoff, n_reads, rows, plan.max_rows, alphabet, kind, fq_strings(out), fs.qual, stream);
        if (rc != PO_OK) return rc;
        PO_HIPCHK(lattice.mark(stream));
    }
    PO_HIPCHK(hipStreamSynchronize(stream));
    if (stage_ms_h) {
        stage_ms_h[4] = stitch.total();
        stage_ms_h[5] = decode.total();
        if (fq) {
            stage_ms_h[6] = guides.total();
            stage_ms_h[7] = lattice.total();
        }
    }
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    PO_HIPCHK(dlog.down(logits_h, (size_t)rows * NOUT * 4));
    if (fq) {
        rc = fs.down(*fq, seq_off_h, n_reads, rows, out.cap);
        if (rc != PO_OK) return rc;
    }
    return PO_OK;
}

namespace {
// a call of its own: a fresh state, freed when the call returns, on the null stream
int basecall_impl(const char* name, const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                  const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights, const char* alphabet,
                  int kind, int beam_width, int model, int max_windows_per_pass, char* seq_h, const int64_t* seq_off_h,
                  int32_t* seq_len_h, int32_t* status_h, float* logits_h, float* stage_ms_h, const FastqOut* fq) {
    PoBasecallResident st;
    return po_basecall_body(&st, nullptr, false, name, signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers, weights_h,
                            n_weights, alphabet, kind, beam_width, model, max_windows_per_pass, seq_h, seq_off_h, seq_len_h, status_h,
                            logits_h, stage_ms_h, fq);
}
}  // namespace

extern "C" int po_basecall_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                   const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                   const char* alphabet, int kind, int beam_width, int model, int max_windows_per_pass,
                                   char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                                   float* logits_h, float* stage_ms_h) {
    return basecall_impl("po_basecall_batch_h", signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers, weights_h,
                         n_weights, alphabet, kind, beam_width, model, max_windows_per_pass, seq_h, seq_off_h, seq_len_h, status_h,
                         logits_h, stage_ms_h, nullptr);
}

extern "C" int po_basecall_fastq_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                         const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                         const char* alphabet, int kind, int beam_width, int model, int max_windows_per_pass,
                                         char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                                         float* logits_h, int band_size, char* qual_h, int32_t* qual_status_h, double* odds_h,
                                         int32_t* guide_h, float* stage_ms_h) {
    const FastqOut fq = {band_size, qual_h, qual_status_h, odds_h, guide_h};
    return basecall_impl("po_basecall_fastq_batch_h", signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers, weights_h,
                         n_weights, alphabet, kind, beam_width, model, max_windows_per_pass, seq_h, seq_off_h, seq_len_h, status_h,
                         logits_h, stage_ms_h, &fq);
}

// The quality stages alone, on tables and strings that somebody else left on the device: what
// po_basecall_fastq_batch_h runs behind its decoder, through the same FastqStages.
extern "C" int po_fastq_tables(const double* y, const int64_t* y_off, int n, int C, int model, int kind, const char* seq,
                               const int64_t* seq_off, const int32_t* seq_len, const int32_t* status, const int32_t* map,
                               int scored_is_viterbi, int band_size, const int32_t* unbanded_h, char* qual, int32_t* qual_status,
                               double* odds, int32_t* guide, void* stream_) {
    const char* name = "po_fastq_tables";
    const std::string me = std::string(name) + ": ";
    hipStream_t stream = (hipStream_t)stream_;
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n < 0) return po_fail(PO_E_ARG, me + "n " + std::to_string(n));
    if (scored_is_viterbi != 0 && scored_is_viterbi != 1)
        return po_fail(PO_E_ARG, me + "scored_is_viterbi " + std::to_string(scored_is_viterbi) + " (0 or 1)");
    const struct { const void* p; const char* name; } ptrs[] = {
        {y, "y"}, {y_off, "y_off"}, {seq, "seq"}, {seq_off, "seq_off"}, {seq_len, "seq_len"}, {status, "status"},
        {scored_is_viterbi ? (const void*)map : (const void*)name, "map"}, {qual, "qual"}, {qual_status, "qual_status"}};
    for (const auto& a : ptrs)
        if (!a.p) return po_fail(PO_E_ARG, me + "null argument " + a.name);
    if (model == PO_MODEL_FLIPFLOP || kind == PO_KIND_FLIPFLOP)
        return po_fail(PO_E_UNSUPPORTED, me + "the flip-flop model has no quality lattice");
    if (C != NOUT) return po_fail(PO_E_ARG, me + "C " + std::to_string(C) + " (5: A, C, G, T and the blank)");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, me + "model " + std::to_string(model));
    if (kind != PO_KIND_POREOVER && kind != PO_KIND_BONITO) return po_fail(PO_E_ARG, me + "kind " + std::to_string(kind));
    if ((kind == PO_KIND_BONITO) != (model == PO_MODEL_MERGE))
        return po_fail(PO_E_ARG, me + "model " + std::to_string(model) + " is not the tree model of kind " + std::to_string(kind));
    if (n == 0) return PO_OK;
    std::vector<int64_t> h(2 * ((size_t)n + 1));   // the tables' row offsets | the strings'
    PO_HIPCHK(po_read_tables(y_off, seq_off, n, stream, h.data()));
    const int64_t *yo = h.data(), *so = h.data() + n + 1;
    if (yo[0] != 0 || so[0] != 0) return po_fail(PO_E_ARG, me + (yo[0] != 0 ? "y_off" : "seq_off") + "[0] must be 0");
    int64_t max_rows = 0;
    for (int i = 0; i < n; ++i) {
        if (yo[i + 1] < yo[i] || so[i + 1] < so[i])
            return po_fail(PO_E_ARG, me + (yo[i + 1] < yo[i] ? "y_off" : "seq_off") + " decreases at read " + std::to_string(i));
        if (so[i + 1] - so[i] < yo[i + 1] - yo[i])   // (the Viterbi call of the guides is written at the strings' offsets)
            return po_fail(PO_E_CAP, me + "read " + std::to_string(i) + " has room for " + std::to_string(so[i + 1] - so[i]) +
                           " characters and " + std::to_string(yo[i + 1] - yo[i]) + " frames");
        max_rows = std::max(max_rows, yo[i + 1] - yo[i]);
    }
    const int64_t rows = yo[n];
    std::vector<int32_t> len_h((size_t)n);
    PO_HIPCHK(hipMemcpyAsync(len_h.data(), seq_len, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
    PO_HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i)
        if (len_h[i] > so[i + 1] - so[i])
            return po_fail(PO_E_CAP, me + "read " + std::to_string(i) + " has " + std::to_string(len_h[i]) + " characters in room for " +
                           std::to_string(so[i + 1] - so[i]));
    const FqStrings out = {seq, seq_off, seq_len, status, (size_t)so[n]};

    FastqStages fs;
    fs.qual_route = po_qual_entry_route();
    int rc = fs.prepare(n, rows, kind, !scored_is_viterbi, !scored_is_viterbi, out.cap, scored_is_viterbi ? map : nullptr);
    if (rc == PO_OK) rc = fs.guides(name, band_size, y, y_off, n, rows, "ACGT", kind, out, stream);
    if (rc == PO_OK) rc = fs.lattice(band_size, unbanded_h, y, y_off, n, rows, max_rows, "ACGT", kind, out, qual, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(po_out(qual_status, fs.qst.p, sizeof(int32_t) * n, true, stream));
    PO_HIPCHK(po_out(odds, fs.odds.p, sizeof(double) * 5 * (size_t)(fs.total_b + fs.total_u), true, stream));
    if (band_size > 0) PO_HIPCHK(po_out(guide, fs.guide.p, sizeof(int32_t) * (size_t)rows, true, stream));
    PO_HIPCHK(hipStreamSynchronize(stream));   // (the stages' buffers are this call's: they go when it returns)
    return PO_OK;
}
