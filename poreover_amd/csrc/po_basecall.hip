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
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "po_basecall_plan.h"
#include "po_hostbuf.h"

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

// event pairs on the call's stream, summed into one figure at the end (only where stage times are asked for)
struct Spans {
    std::vector<hipEvent_t> ev;
    bool on;
    explicit Spans(bool on_) : on(on_) {}
    ~Spans() { for (auto e : ev) (void)hipEventDestroy(e); }
    hipError_t mark(hipStream_t s) {
        if (!on) return hipSuccess;
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
    float total() const {   // after a synchronise
        float sum = 0.f, ms = 0.f;
        for (size_t i = 0; i + 1 < ev.size(); i += 2)
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) sum += ms;
        return sum;
    }
};

}  // namespace

extern "C" int po_basecall_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                   const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                   const char* alphabet, int kind, int beam_width, int model, int max_windows_per_pass,
                                   char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                                   float* logits_h, float* stage_ms_h) {
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n_reads < 0) return po_fail(PO_E_ARG, "po_basecall_batch_h: n_reads " + std::to_string(n_reads));
    if (!signal_h || !sig_off_h || !layers_h || !weights_h || !seq_h || !seq_off_h || !seq_len_h || !status_h)
        return po_fail(PO_E_ARG, std::string("po_basecall_batch_h: null argument ") +
                       (!signal_h ? "signal_h" : !sig_off_h ? "sig_off_h" : !layers_h ? "layers_h" : !weights_h ? "weights_h" :
                        !seq_h ? "seq_h" : !seq_off_h ? "seq_off_h" : !seq_len_h ? "seq_len_h" : "status_h"));
    PoBasecallPlan plan;
    std::string err;
    int rc = po_basecall_make_plan(sig_off_h, n_reads, window, overlap, seq_off_h, &plan, &err);
    if (rc != PO_OK) return po_fail(rc, err);
    if (kind == PO_KIND_FLIPFLOP || model == PO_MODEL_FLIPFLOP)
        return po_fail(PO_E_UNSUPPORTED, "po_basecall_batch_h: flip-flop decoding (kind " + std::to_string(kind) + ", model " +
                       std::to_string(model) + "): the network's output is a CTC table");
    if (kind != PO_KIND_POREOVER && kind != PO_KIND_BONITO) return po_fail(PO_E_ARG, "po_basecall_batch_h: kind " + std::to_string(kind));
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, "po_basecall_batch_h: model " + std::to_string(model));
    if (beam_width > 64) return po_fail(PO_E_ARG, "po_basecall_batch_h: beam_width " + std::to_string(beam_width) + " (at most 64)");
    if (alphabet && std::strlen(alphabet) != NOUT - 1)
        return po_fail(PO_E_ARG, std::string("po_basecall_batch_h: alphabet \"") + alphabet + "\" (4 symbols: the network has 5 outputs)");
    // the model and the weights' length: po_call_batch's own checks, which come before it looks at a buffer (no windows:
    // the pointers are not followed)
    rc = po_call_batch(weights_h, 0, window, layers_h, n_layers, weights_h, n_weights, (float*)weights_h, nullptr, nullptr, 0,
                       nullptr, nullptr);
    if (rc != PO_OK) return rc;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + 6, 0.f);
    if (n_reads == 0) return PO_OK;

    // ---- windows per pass: as many as ~4 GiB of pass buffers hold (po_call_batch_h's rule), whole recurrence tiles
    const size_t per_window = po_call_workspace_bytes(1, window, layers_h, n_layers) + (size_t)window * NOUT * 4 * 2 + (size_t)window * 4;
    int64_t chunk = (int64_t)std::max<size_t>(1, ((size_t)4 << 30) / per_window);
    if (chunk >= TILE) chunk = chunk / TILE * TILE;
    if (max_windows_per_pass > 0) chunk = std::min<int64_t>(chunk, max_windows_per_pass);   // (a smaller bound: the tests')
    chunk = std::min<int64_t>(chunk, plan.windows);
    const int64_t Mc = chunk * window;
    const size_t wsb = po_call_workspace_bytes((int)chunk, window, layers_h, n_layers);

    hipStream_t stream = nullptr;
    const int64_t rows = plan.rows;
    PoDev dw, dsig, dsoff, dwoff, dwread, dwin, dprob, dplog, dws, dlog, dy, dws2;
    PoSeqOut out;
    PO_HIPCHK(dw.up(weights_h, (size_t)n_weights * 4));
    PO_HIPCHK(dsig.up(signal_h, (size_t)rows * 4));             // each read's signal once, whatever the overlap
    PO_HIPCHK(dsoff.up(sig_off_h, sizeof(int64_t) * ((size_t)n_reads + 1)));
    PO_HIPCHK(dwoff.up(plan.win_off.data(), sizeof(int64_t) * plan.win_off.size()));
    PO_HIPCHK(dwread.up(plan.win_read.data(), sizeof(int32_t) * plan.win_read.size()));
    PO_HIPCHK(dwin.up(nullptr, (size_t)Mc * 4));
    PO_HIPCHK(dprob.up(nullptr, (size_t)Mc * NOUT * 4));
    PO_HIPCHK(dplog.up(nullptr, (size_t)Mc * NOUT * 4));
    PO_HIPCHK(dws.up(nullptr, wsb));
    PO_HIPCHK(dlog.up(nullptr, (size_t)rows * NOUT * 4));       // resident: the stitched logits ...
    PO_HIPCHK(dy.up(nullptr, (size_t)rows * NOUT * 8));         // ... and the f64 log-probability table
    PO_HIPCHK(out.up(seq_off_h, n_reads));
    const size_t wsb2 = beam_width <= 0 ? po_viterbi_workspace_bytes(n_reads, rows, NOUT, kind)
                                        : po_beam1d_workspace_bytes(n_reads, rows, plan.max_rows, NOUT, beam_width, model);
    PO_HIPCHK(dws2.up(nullptr, wsb2));

    Spans stitch(stage_ms_h != nullptr), decode(stage_ms_h != nullptr);
    WinArgs a;
    a.sig_off = dsoff; a.win_off = dwoff; a.win_read = dwread;
    a.W = window; a.S = plan.stride; a.O = overlap;
    for (int64_t w0 = 0; w0 < plan.windows; w0 += chunk) {
        const int nc = (int)std::min<int64_t>(chunk, plan.windows - w0);
        a.w0 = w0;
        a.count = (int64_t)nc * window;
        PO_HIPCHK(stitch.mark(stream));
        hipLaunchKernelGGL(window_gather_kernel, dim3(grid_for(a.count)), dim3(256), 0, stream, a, dsig.as<float>(), dwin.as<float>());
        PO_HIPCHK(stitch.mark(stream));
        PO_HIPCHK(hipGetLastError());
        rc = po_call_batch(dwin, nc, window, layers_h, n_layers, dw, n_weights, dprob, dplog, dws, wsb, stream, stage_ms_h);
        if (rc != PO_OK) return rc;
        a.count = (int64_t)nc * window * NOUT;
        PO_HIPCHK(stitch.mark(stream));
        hipLaunchKernelGGL(window_stitch_kernel, dim3(grid_for(a.count)), dim3(256), 0, stream, a, dplog.as<float>(), dlog.as<float>());
        PO_HIPCHK(stitch.mark(stream));
        PO_HIPCHK(hipGetLastError());
    }
    // the reference's f32 log-softmax of the logits, widened (decode.py:34-39), then the decoder over all reads at once
    PO_HIPCHK(stitch.mark(stream));
    rc = po_launch_ingest(dlog, dsoff, n_reads, NOUT, PO_INGEST_LOGITS_F32, nullptr, 0, rows, dy, stream);
    if (rc != PO_OK) return po_fail(rc, "po_basecall_batch_h: ingest");
    PO_HIPCHK(stitch.mark(stream));
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(decode.mark(stream));
    rc = beam_width <= 0 ? po_viterbi_batch(dy, dsoff, n_reads, NOUT, alphabet, kind, nullptr, out.seq, out.off, out.len, nullptr,
                                            out.status, dws2, wsb2, stream)
                         : po_beam1d_batch(dy, dsoff, n_reads, NOUT, alphabet, beam_width, model, out.seq, out.off, out.len,
                                           out.status, dws2, wsb2, stream);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(decode.mark(stream));
    PO_HIPCHK(hipStreamSynchronize(stream));
    if (stage_ms_h) {
        stage_ms_h[4] = stitch.total();
        stage_ms_h[5] = decode.total();
    }
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    PO_HIPCHK(dlog.down(logits_h, (size_t)rows * NOUT * 4));
    return PO_OK;
}
