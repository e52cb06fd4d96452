// The network part of `basecall`, once: the buffers and the pass loop window_gather_kernel -> po_call_batch ->
// window_stitch_kernel that leave the stitched logits of every read on the device (po_basecall.hip defines it).
// po_basecall_batch_h, po_basecall_fastq_batch_h and po_pair_basecall_batch_h (po_pair_basecall.hip) all run this loop, so
// a window's logits are the same bits in each.  Host only, hidden: nothing here is part of the library's symbol table.
#pragma once
#include <vector>

#include "po_basecall_plan.h"
#include "po_hostbuf.h"

#pragma GCC visibility push(hidden)

// event pairs on the call's stream, summed into one figure at the end (only where stage times are asked for)
struct PoSpans {
    std::vector<hipEvent_t> ev;
    bool on;
    explicit PoSpans(bool on_) : on(on_) {}
    PoSpans(const PoSpans&) = delete;
    PoSpans& operator=(const PoSpans&) = delete;
    ~PoSpans() { for (auto e : ev) (void)hipEventDestroy(e); }
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

struct PoBasecallPasses {
    PoDev w, sig, sig_off, win_off, win_read, win, prob, plog, ws, logits;   // logits: [rows][5] f32, read-major, resident
    bool w_up = false;      // the weights are on the device already (an engine's resident state): up() leaves them
    int64_t chunk = 0;      // windows per pass
    size_t ws_bytes = 0;    // po_call_batch's workspace for a pass
    // the weights, each read's signal (once, whatever the overlap), the plan's tables; the pass buffers and the logits.
    // Windows per pass: as many as ~4 GiB of pass buffers hold (po_call_batch_h's rule), whole recurrence tiles;
    // max_windows_per_pass > 0: at most that many.  plan.windows >= 1.
    int up(const PoBasecallPlan& plan, const float* signal_h, const int64_t* sig_off_h, int n_reads, int window,
           const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights, int max_windows_per_pass);
    // signal_h == NULL: the signal is in `sig` already (po_launch_signal_prep wrote it there), plan.rows values from 0
    // enqueues every pass on `stream`; stage_ms_h (or NULL): po_call_batch's four stages, added; the gather and stitch
    // kernels are bracketed in `stitch`
    int run(const PoBasecallPlan& plan, int window, int overlap, const po_call_layer* layers_h, int n_layers, int64_t n_weights,
            hipStream_t stream, float* stage_ms_h, PoSpans& stitch);
    // an engine's resident state.  The weights, once: up() then leaves them where they are
    int weights_resident(const float* weights_h, int64_t n_weights) {
        PO_HIPCHK(w.up(weights_h, (size_t)n_weights * 4));
        w_up = true;
        return PO_OK;
    }
    // `sig` with room for `samples` f32 values: where po_launch_signal_prep writes for a body call with signal_resident
    int signal_room(int64_t samples, float** signal) {
        PO_HIPCHK(sig.up(nullptr, (size_t)samples * 4));
        *signal = sig.as<float>();
        return PO_OK;
    }
};

// ---- the body of po_basecall_batch_h / po_basecall_fastq_batch_h (po_basecall.hip) on a state that may outlive the call.
// The entries run it on a fresh state and the null stream; a po_basecaller worker (po_basecall_stream.hip) keeps one state
// per worker - weights uploaded once, every buffer grow-only - and gives its own stream.
struct PoBasecallFastq {   // what po_basecall_fastq_batch_h adds to po_basecall_batch_h's arguments
    int band_size;
    char* qual_h; int32_t* qual_status_h; double* odds_h; int32_t* guide_h;
};
struct PoBasecallResident;
PoBasecallResident* po_basecall_resident_new();
void po_basecall_resident_free(PoBasecallResident* st);
PoBasecallPasses& po_basecall_resident_net(PoBasecallResident* st);
int po_basecall_body(PoBasecallResident* st, hipStream_t stream, bool signal_resident, const char* name, const float* signal_h,
                     const int64_t* sig_off_h, int n_reads, int window, int overlap, const po_call_layer* layers_h, int n_layers,
                     const float* weights_h, int64_t n_weights, const char* alphabet, int kind, int beam_width, int model,
                     int max_windows_per_pass, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                     float* logits_h, float* stage_ms_h, const PoBasecallFastq* fq);

#pragma GCC visibility pop
