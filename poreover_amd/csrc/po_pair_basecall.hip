// `pair-basecall`: scaled signals and a list of read pairs in, 1D² consensus strings out, in one device-resident pass
// (DESIGN.md §17).
//
// What `call` followed by `pair-decode` does in two commands and a file per read — the network's forward pass (po_call.hip),
// the log-softmax of its logits with read 2's time reversal and column permutation (po_ingest.hip) and the pair chain
// (po_pair.hip: Viterbi of both reads, length skip, alignment, identity skip, envelope, pair beam search) — with the
// per-frame data staying on the device in between and with `basecall`'s overlapping windows (po_basecall_pass.h: the same
// pass loop, so a window's logits are the same bits).
//
//   pair_table_kernel   the stitched logits (read-major f32) to the two pair-major f64 log-probability tables that
//                       po_pair_decode_batch reads; a read may stand in several pairs and on either side
//
// A streaming copy like ingest_kernel: one lane per output frame, 20 bytes in, 40 bytes out, a frame's five values
// contiguous on both sides; every output value has one writer, so two runs give the same bits.
#include <algorithm>
#include <string>

#include "po_basecall_pass.h"
#include "po_ingest_rules.h"
#include "po_pair_basecall_plan.h"

namespace {

constexpr int NOUT = 5;   // Dense outputs (A, C, G, T, blank)

struct PTArgs {
    const float* logits;        // [rows of all reads][NOUT], read-major
    const int64_t* sig_off;     // [n_reads + 1] row offsets of the reads
    const int32_t* pair_idx;    // [2 * n_pairs]
    const int64_t* y_off[2];    // [n_pairs + 1] each
    double* y[2];
    int64_t rows0, total;       // rows of table 0, rows of both
    int n_pairs, reverse2;
    int perm2[NOUT];
};

// y[side][row][c] = log-softmax(logits[source row])[c'] with c' = c (side 0) or perm2[c] (side 1); lanes [0, rows0) make
// table 0, lanes [rows0, total) table 1 (po_pair_basecall_plan.h: the source row)
__global__ __launch_bounds__(64) void pair_table_kernel(PTArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * blockDim.x) {
        const int side = i >= a.rows0 ? 1 : 0;
        const int64_t row = side ? i - a.rows0 : i;
        const int64_t src = po_pair_table_source(a.sig_off, a.pair_idx, a.y_off[side], a.n_pairs, side, a.reverse2, row, nullptr);
        double v[NOUT];
        po_ingest_log_softmax_f32(a.logits + src * NOUT, NOUT, v);
        double* o = a.y[side] + row * NOUT;
#pragma unroll
        for (int c = 0; c < NOUT; ++c) {   // (selects, not an indexed read of v: the five values stay in registers)
            const int p = side ? a.perm2[c] : c;
            o[c] = p == 0 ? v[0] : p == 1 ? v[1] : p == 2 ? v[2] : p == 3 ? v[3] : v[4];
        }
    }
}

// the plan's two tables on the device, and the launch
struct PairTables {
    PoDev idx, off[2], y[2];
    int up(const PoPairBasecallPlan& pp, const int32_t* pair_idx_h, int n_pairs) {
        PO_HIPCHK(idx.up(pair_idx_h, sizeof(int32_t) * 2 * (size_t)n_pairs));
        for (int s = 0; s < 2; ++s) {
            PO_HIPCHK(off[s].up(pp.y_off[s].data(), sizeof(int64_t) * pp.y_off[s].size()));
            PO_HIPCHK(y[s].up(nullptr, sizeof(double) * NOUT * (size_t)pp.rows[s]));
        }
        return PO_OK;
    }
    int launch(const PoPairBasecallPlan& pp, const float* logits, const int64_t* sig_off, int n_pairs, int reverse2, const int* perm2,
               hipStream_t stream) {
        PTArgs a;
        a.logits = logits; a.sig_off = sig_off; a.pair_idx = idx;
        for (int s = 0; s < 2; ++s) { a.y_off[s] = off[s]; a.y[s] = y[s]; }
        a.rows0 = pp.rows[0]; a.total = pp.rows[0] + pp.rows[1];
        a.n_pairs = n_pairs; a.reverse2 = reverse2 ? 1 : 0;
        for (int c = 0; c < NOUT; ++c) a.perm2[c] = perm2 ? perm2[c] : c;
        if (a.total <= 0) return PO_OK;
        const int64_t blocks = std::min<int64_t>((a.total + 63) / 64, 256 * 32);
        hipLaunchKernelGGL(pair_table_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, a);
        PO_HIPCHK(hipGetLastError());
        return PO_OK;
    }
};

int check_perm(const std::string& me, const int* perm2_h) {
    for (int c = 0; perm2_h && c < NOUT; ++c)
        if (perm2_h[c] < 0 || perm2_h[c] >= NOUT)
            return po_fail(PO_E_ARG, me + "perm2[" + std::to_string(c) + "] is " + std::to_string(perm2_h[c]) + " (0 to 4)");
    return PO_OK;
}

}  // namespace

extern "C" int po_pair_tables_h(const float* logits_h, const int64_t* row_off_h, int n_reads, const int32_t* pair_idx_h, int n_pairs,
                                int reverse2, const int* perm2_h, double* y1_h, double* y2_h) {
    const std::string me = "po_pair_tables_h: ";
    po_set_error("");
    if (!logits_h || !row_off_h || !pair_idx_h || !y1_h || !y2_h)
        return po_fail(PO_E_ARG, me + "null argument " +
                       (!logits_h ? "logits_h" : !row_off_h ? "row_off_h" : !pair_idx_h ? "pair_idx_h" : !y1_h ? "y1_h" : "y2_h"));
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if (row_off_h[0] != 0) return po_fail(PO_E_ARG, me + "row_off[0] is " + std::to_string(row_off_h[0]) + " (must be 0)");
    for (int r = 0; r < n_reads; ++r)
        if (row_off_h[r + 1] < row_off_h[r]) return po_fail(PO_E_ARG, me + "row_off decreases at read " + std::to_string(r));
    PoPairBasecallPlan pp;
    std::string err;
    int rc = po_pair_basecall_make_plan(row_off_h, n_reads, pair_idx_h, n_pairs, nullptr, nullptr, &pp, &err, "po_pair_tables_h");
    if (rc != PO_OK) return po_fail(rc, err);
    rc = check_perm(me, perm2_h);
    if (rc != PO_OK) return rc;
    if (n_pairs == 0) return PO_OK;
    PoDev lg, so;
    PairTables t;
    PO_HIPCHK(lg.up(logits_h, sizeof(float) * NOUT * (size_t)row_off_h[n_reads]));
    PO_HIPCHK(so.up(row_off_h, sizeof(int64_t) * ((size_t)n_reads + 1)));
    rc = t.up(pp, pair_idx_h, n_pairs);
    if (rc != PO_OK) return rc;
    rc = t.launch(pp, lg, so, n_pairs, reverse2, perm2_h, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(t.y[0].down(y1_h, sizeof(double) * NOUT * (size_t)pp.rows[0]));
    PO_HIPCHK(t.y[1].down(y2_h, sizeof(double) * NOUT * (size_t)pp.rows[1]));
    return PO_OK;
}

extern "C" int po_pair_basecall_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                        const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                        int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                                        const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                                        int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                                        int32_t* seq_len_h, int32_t* status_h, float* logits_h, float* stage_ms_h) {
    const char* name = "po_pair_basecall_batch_h";
    const std::string me = std::string(name) + ": ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if (n_pairs < 0) return po_fail(PO_E_ARG, me + "n_pairs " + std::to_string(n_pairs));
    const struct { const void* p; const char* name; } ptrs[] = {
        {signal_h, "signal_h"}, {sig_off_h, "sig_off_h"}, {layers_h, "layers_h"}, {weights_h, "weights_h"}, {pair_idx_h, "pair_idx_h"},
        {opt, "opt"}, {seq1d_h, "seq1d_h"}, {seq1d_off_h, "seq1d_off_h"}, {len1_h, "len1_h"}, {len2_h, "len2_h"},
        {identity_h, "identity_h"}, {seq_h, "seq_h"}, {seq_off_h, "seq_off_h"}, {seq_len_h, "seq_len_h"}, {status_h, "status_h"}};
    for (const auto& a : ptrs)
        if (!a.p) return po_fail(PO_E_ARG, me + "null argument " + a.name);
    PoBasecallPlan plan;
    PoPairBasecallPlan pp;
    std::string err;
    int rc = po_basecall_make_plan(sig_off_h, n_reads, window, overlap, nullptr, &plan, &err, name);
    if (rc != PO_OK) return po_fail(rc, err);
    rc = po_pair_basecall_make_plan(sig_off_h, n_reads, pair_idx_h, n_pairs, seq1d_off_h, seq_off_h, &pp, &err, name);
    if (rc != PO_OK) return po_fail(rc, err);
    if (reverse_complement != 0 && reverse_complement != 1)
        return po_fail(PO_E_ARG, me + "reverse_complement " + std::to_string(reverse_complement) + " (0 or 1)");
    if (opt->model == PO_MODEL_FLIPFLOP)
        return po_fail(PO_E_UNSUPPORTED, me + "flip-flop decoding (model " + std::to_string(opt->model) +
                       "): the network's output is a CTC table");
    if (opt->model != PO_MODEL_CTC && opt->model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, me + "model " + std::to_string(opt->model));
    if (opt->beam_width < 1 || opt->beam_width > 25)
        return po_fail(PO_E_ARG, me + "beam_width " + std::to_string(opt->beam_width) + " (1 to 25)");
    if (opt->method != PO_METHOD_ROW && opt->method != PO_METHOD_ROW_COL && opt->method != PO_METHOD_GRID)
        return po_fail(PO_E_ARG, me + "method " + std::to_string(opt->method));
    // the model and the weights' length: po_call_batch's own checks, which come before it looks at a buffer (no windows:
    // the pointers are not followed)
    rc = po_call_batch(weights_h, 0, window, layers_h, n_layers, weights_h, n_weights, (float*)weights_h, nullptr, nullptr, 0,
                       nullptr, nullptr);
    if (rc != PO_OK) return rc;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + 6, 0.f);
    if (n_pairs == 0 || n_reads == 0) return PO_OK;

    hipStream_t stream = nullptr;
    static const int RC_PERM[NOUT] = {3, 2, 1, 0, 4};   // the complement: A <-> T, C <-> G, blank stays
    PoBasecallPasses net;
    PairTables t;
    PoSeqOut out;
    PoDev s1o, s1, l1, l2, idn, ws;
    const size_t s1b = (size_t)seq1d_off_h[2 * (size_t)n_pairs], per = sizeof(int32_t) * (size_t)n_pairs;
    rc = net.up(plan, signal_h, sig_off_h, n_reads, window, layers_h, n_layers, weights_h, n_weights, max_windows_per_pass);
    if (rc != PO_OK) return rc;
    rc = t.up(pp, pair_idx_h, n_pairs);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(out.up(seq_off_h, n_pairs));
    PO_HIPCHK(s1o.up(seq1d_off_h, sizeof(int64_t) * (2 * (size_t)n_pairs + 1)));
    PO_HIPCHK(s1.up(nullptr, s1b));
    PO_HIPCHK(l1.up(nullptr, per));
    PO_HIPCHK(l2.up(nullptr, per));
    PO_HIPCHK(idn.up(nullptr, sizeof(double) * (size_t)n_pairs));
    const size_t wsb = po_pair_decode_workspace_bytes(n_pairs, pp.rows[0], pp.rows[1], pp.max_rows[0], pp.max_rows[1], NOUT, opt);
    PO_HIPCHK(ws.up(nullptr, wsb));

    PoSpans stitch(stage_ms_h != nullptr), decode(stage_ms_h != nullptr);
    rc = net.run(plan, window, overlap, layers_h, n_layers, n_weights, stream, stage_ms_h, stitch);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(stitch.mark(stream));
    rc = t.launch(pp, net.logits, net.sig_off, n_pairs, reverse_complement, reverse_complement ? RC_PERM : nullptr, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(stitch.mark(stream));
    PO_HIPCHK(decode.mark(stream));
    rc = po_pair_decode_batch(t.y[0], t.off[0], t.y[1], t.off[1], n_pairs, NOUT, opt, s1, s1o, l1, l2, idn, nullptr, out.seq, out.off,
                              out.len, out.status, ws, wsb, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(decode.mark(stream));
    PO_HIPCHK(hipStreamSynchronize(stream));
    if (stage_ms_h) {
        stage_ms_h[4] = stitch.total();
        stage_ms_h[5] = decode.total();
    }
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    PO_HIPCHK(s1.down(seq1d_h, s1b));
    PO_HIPCHK(l1.down(len1_h, per));
    PO_HIPCHK(l2.down(len2_h, per));
    PO_HIPCHK(idn.down(identity_h, sizeof(double) * (size_t)n_pairs));
    PO_HIPCHK(net.logits.down(logits_h, (size_t)plan.rows * NOUT * 4));
    return PO_OK;
}
