// What po_basecaller (po_basecall_stream.hip) and po_pair_basecaller (po_pair_basecall_stream.hip) share on the device
// side.  An engine holds the model, its options and one worker per listed device: the worker's resident
// state (the weights, uploaded once at create, and every buffer of the body, grow-only between groups and runs), its stream
// and the raw route's buffers.  A run cuts its items, in input order, into groups and deals them (po_engine_deal.h) to one
// host thread per worker; a group runs the single-device entry's body on the worker's state and stream, and its results
// land in the caller's arrays at the items' own indices.  On the raw route prepare_raw sends the int16 samples up,
// po_launch_signal_prep writes the f32 signal into the state's signal buffer, the kept counts come back for the window
// plan, and the body runs on the signal where it lies.
//
// Streams: a worker's stream is a blocking one (hipStreamCreate), so the body's blocking copies, which are null-stream
// work, are ordered against it in both directions; the body synchronises the stream before its downloads.
// Errors: the message is thread-local (po_capi.hip) and carried from the worker's thread to the caller.
// The slice pool of beam2d_reg_kernel (po_beam2d_route.hip) is one per device and is made by the workspace-size query on
// the thread whose current device it is: a body makes that query on the worker's own thread, after po_set_device, before
// the group's first launch, so the launch path never allocates.
// Host only, hidden: nothing here is part of the library's symbol table.
#pragma once
#include <string>
#include <vector>

#include "po_basecall_pass.h"
#include "po_engine_deal.h"
#include "po_hostbuf.h"
#include "po_prep_rules.h"

#pragma GCC visibility push(hidden)

namespace {
constexpr int NOUT = 5;
constexpr int MAX_WORKERS = 16;
constexpr int64_t DEFAULT_RESIDENT = (int64_t)16 << 30;
}  // namespace

struct PoEngineWorker {
    int dev = 0;
    hipStream_t stream = nullptr;
    PoDev raw, raw_off, slab_off, slab_read, offset, alpha, sig_off, stats, ws;   // the raw route's, grow-only

    // The raw route's preparation of a group's c reads: their int16 samples back to back in `raw`, offsets ro from 0,
    // offset / alpha in the group's order (or NULL).  The f32 signal is left in net's signal buffer, ko gets the kept
    // samples' offsets.
    int prepare_raw(const int16_t* raw_h, const int64_t* ro, int c, const double* offset_h, const double* alpha_h, int scaling,
                    int lo, int hi, const char* name, PoBasecallPasses& net, std::vector<int64_t>& ko) {
        PoPrepPlan plan;
        std::string err;
        int rc = po_prep_make_plan(ro, c, scaling, lo, hi, &plan, &err, name);
        if (rc != PO_OK) return po_fail(rc, err);
        ko.assign((size_t)c + 1, 0);
        if (plan.total == 0) return PO_OK;
        const int64_t slabs = (int64_t)plan.slab_read.size();
        const size_t wsb = po_prep_workspace_bytes(c, slabs, plan.bins);
        float* sig = nullptr;
        PO_HIPCHK(raw.up(raw_h, (size_t)plan.total * 2));
        PO_HIPCHK(raw_off.up(ro, sizeof(int64_t) * ((size_t)c + 1)));
        PO_HIPCHK(slab_off.up(plan.slab_off.data(), sizeof(int64_t) * plan.slab_off.size()));
        PO_HIPCHK(slab_read.up(plan.slab_read.data(), sizeof(int32_t) * plan.slab_read.size()));
        if (offset_h) {
            PO_HIPCHK(offset.up(offset_h, sizeof(double) * c));
            PO_HIPCHK(alpha.up(alpha_h, sizeof(double) * c));
        }
        PO_HIPCHK(sig_off.up(nullptr, sizeof(int64_t) * ((size_t)c + 1)));
        PO_HIPCHK(stats.up(nullptr, sizeof(po_prep_stats) * (size_t)c));
        PO_HIPCHK(ws.up(nullptr, wsb));
        rc = net.signal_room(plan.total, &sig);
        if (rc != PO_OK) return rc;
        rc = po_launch_signal_prep(raw, raw_off, c, plan.total, slab_off, slab_read, slabs, scaling, lo, hi,
                                   offset_h ? offset.as<double>() : nullptr, offset_h ? alpha.as<double>() : nullptr, sig, sig_off,
                                   stats, ws, wsb, stream);
        if (rc != PO_OK) return rc;
        PO_HIPCHK(hipMemcpyAsync(ko.data(), sig_off.p, sizeof(int64_t) * ((size_t)c + 1), hipMemcpyDeviceToHost, stream));
        PO_HIPCHK(hipStreamSynchronize(stream));
        return PO_OK;
    }
};

// What an engine holds whatever it calls: W derives from PoEngineWorker and adds its state `st`.  The engine (E below)
// derives from this and adds its options and `stats`, a vector of its Stat (with groups and busy_ms) per worker.
template <class W>
struct PoEngine {
    std::vector<W*> workers;
    std::vector<int> devices;
    std::vector<po_call_layer> layers;
    std::vector<float> weights;
};

// ---- create.  `me` is "<entry>: ": every message is the calling entry's.
// the arguments' checks that come before the single-device entry's own
inline int po_engine_check_devices(const std::string& me, const int* devices, int ndev, const void* layers_h, const void* weights_h,
                                   const void* opt) {
    if (!devices || !layers_h || !weights_h || !opt)
        return po_fail(PO_E_ARG, me + "null argument " + (!devices ? "devices" : !layers_h ? "layers_h" : !weights_h ? "weights_h" : "options"));
    if (ndev < 1 || ndev > MAX_WORKERS)
        return po_fail(PO_E_ARG, me + "ndev " + std::to_string(ndev) + " (1 to " + std::to_string(MAX_WORKERS) + ")");
    const int nd = po_device_count();
    for (int i = 0; i < ndev; ++i)
        if (devices[i] < 0 || devices[i] >= nd)
            return po_fail(PO_E_ARG, me + "device " + std::to_string(devices[i]) + " (0 to " + std::to_string(nd - 1) + ")");
    return PO_OK;
}

// and those after it: the raw route's scaling and range (po_signal_prep_h's messages), the budget
inline int po_engine_check_options(const char* name, int scaling, int lo, int hi, int64_t resident_bytes) {
    const int64_t zero = 0;
    PoPrepPlan plan;
    std::string err;
    const int rc = po_prep_make_plan(&zero, 0, scaling, lo, hi, &plan, &err, name);
    if (rc != PO_OK) return po_fail(rc, err);
    if (resident_bytes < 0) return po_fail(PO_E_ARG, std::string(name) + ": resident_bytes " + std::to_string(resident_bytes));
    return PO_OK;
}

// the model, and a worker per listed device: its state (new_state(worker) makes it and returns its passes), its stream,
// and the weights, uploaded here and never again.  On failure the engine holds what was made: po_engine_free takes it.
template <class W, class NewState>
int po_engine_init(PoEngine<W>* b, const std::string& me, const int* devices, int ndev, const po_call_layer* layers_h, int n_layers,
                   const float* weights_h, int64_t n_weights, NewState new_state) {
    b->devices.assign(devices, devices + ndev);
    b->layers.assign(layers_h, layers_h + n_layers);
    b->weights.assign(weights_h, weights_h + n_weights);
    int before = 0;
    (void)hipGetDevice(&before);
    int rc = PO_OK;
    for (int i = 0; i < ndev && rc == PO_OK; ++i) {
        W* w = new W;
        w->dev = devices[i];
        b->workers.push_back(w);
        rc = po_set_device(w->dev);
        if (rc != PO_OK) break;
        PoBasecallPasses& net = new_state(*w);
        if (hipStreamCreate(&w->stream) != hipSuccess) { w->stream = nullptr; rc = po_fail(PO_E_HIP, me + "hipStreamCreate"); break; }
        rc = net.weights_resident(weights_h, n_weights);
    }
    (void)hipSetDevice(before);
    return rc;
}

template <class W, class FreeState>
void po_engine_free(PoEngine<W>* b, FreeState free_state) {
    int before = 0;
    (void)hipGetDevice(&before);
    for (W* w : b->workers) {
        (void)hipSetDevice(w->dev);
        if (w->stream) { (void)hipStreamSynchronize(w->stream); (void)hipStreamDestroy(w->stream); }
        if (w->st) free_state(w->st);
        delete w;      // (its buffers free themselves)
    }
    (void)hipSetDevice(before);
}

// ---- run.  The checks that both engines' entries make under their own names
inline int po_engine_check_raw_args(const std::string& me, const void* kept_h, int scaling, const void* offset_h, const void* alpha_h) {
    if (!kept_h) return po_fail(PO_E_ARG, me + "null argument kept_h");
    if (scaling == PO_SCALE_CURRENT && (!offset_h || !alpha_h))
        return po_fail(PO_E_ARG, me + "null argument " + (!offset_h ? "offset_h" : "alpha_h") + " (PO_SCALE_CURRENT)");
    return PO_OK;
}

inline int po_engine_check_from_zero(const std::string& me, const int64_t* off, const char* off_name) {
    if (off[0] != 0) return po_fail(PO_E_ARG, me + off_name + "[0] is " + std::to_string(off[0]) + " (must be 0)");
    return PO_OK;
}

// deals n_groups groups to the engine's workers, run(worker, its stat, g) on the worker's thread and device
template <class E, class RunGroup>
int po_engine_run(E* b, int n_groups, RunGroup run) {
    const PoDealResult r = po_engine_deal(
        (int)b->workers.size(), n_groups, b->stats.data(), [&](int w) { return po_set_device(b->workers[w]->dev); },
        [&](int w, int g) { return run(*b->workers[w], b->stats[w], g); }, [] { return std::string(po_last_error()); });
    if (r.rc != PO_OK) return po_fail(r.rc, "device " + std::to_string(b->devices[r.worker]) + ": " + r.message);
    return PO_OK;
}

#pragma GCC visibility pop
