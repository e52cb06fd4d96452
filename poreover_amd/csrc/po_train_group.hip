// Data-parallel training over several devices (`poreover train --gpus N`): a group of R replicas, each a
// po_trainer on a device of a list (a device may appear more than once), driven by one host thread per replica as po_multi
// drives its pipelines.  The rules are po_train_dp_rules.h's.
//
//   accumulate   micro-batch j of a call goes to replica j: po_train_accumulate itself, on the replica's thread and stream,
//                all replicas at once; every replica's checks run before any replica launches
//   all-reduce   a reduce-scatter and an all-gather, two launches per replica with a hand-off between them:
//     dp_reduce_slice_kernel  on replica r's device: slice r of every contributing accumulator, its own and its peers', read
//                             with 16-byte loads and summed in replica order (plain f32 additions) into slice r of a staging
//                             vector on its own device
//     dp_gather_kernel        on every replica: each slice, from its owner's staging vector, into the replica's accumulator
//                each kernel: one lane per 16 bytes (the n % 4 tail by one lane of the last slice), grid-stride, no LDS, one
//                writer per output value, and no flag of another device or kernel is waited for in device code: the
//                hand-offs are host barriers between the replicas' threads, each after a hipStreamSynchronize
//   apply        po_train_apply on every replica's copy of the sum: the same bits in, the same bits out, no broadcast
//
// Two routes for the slices (po_set_dp_route).  PEER: the kernels read the peers' memory directly (peer access is enabled once,
// at create; replicas on one device need none).  HOST: every contributing accumulator goes to a pinned host buffer, replica r
// uploads slice r of each peer's, the same kernel sums them in the same order; the staging slices come back the same way.
// AUTO is PEER where every pair of the group's devices can do it, else HOST.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "po_train_dp_rules.h"

#include "po_hostbuf.h"

namespace {

// element e of source k is p[k][e - base[k]] (base 0: a whole vector; a slice uploaded from the host starts at its first element)
struct DpSrc {
    const float* p[PO_DP_MAX_REPLICAS];
    int64_t base[PO_DP_MAX_REPLICAS];
    int n;
};

// stage[e] = ((src_0[e] + src_1[e]) + ...) for the groups [g0, g1) and the elements [t0, t1) (the tail: the last slice's)
__global__ __launch_bounds__(256) void dp_reduce_slice_kernel(DpSrc s, float* __restrict__ stage, int64_t g0, int64_t g1,
                                                              int64_t t0, int64_t t1) {
    const int64_t nv = g1 - g0, total = nv + (t1 > t0 ? 1 : 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < nv) {
            const int64_t e = 4 * (g0 + i);
            float4 a = *reinterpret_cast<const float4*>(s.p[0] + (e - s.base[0]));
            for (int k = 1; k < s.n; ++k) {
                const float4 x = *reinterpret_cast<const float4*>(s.p[k] + (e - s.base[k]));
                a.x = po_dp_add(a.x, x.x); a.y = po_dp_add(a.y, x.y); a.z = po_dp_add(a.z, x.z); a.w = po_dp_add(a.w, x.w);
            }
            *reinterpret_cast<float4*>(stage + e) = a;
        } else {
            for (int64_t e = t0; e < t1; ++e) {
                float a = s.p[0][e - s.base[0]];
                for (int k = 1; k < s.n; ++k) a = po_dp_add(a, s.p[k][e - s.base[k]]);
                stage[e] = a;
            }
        }
    }
}

// ga[e] = the staging vector of e's owner at e (s.p[o]: owner o's, s.n = R)
__global__ __launch_bounds__(256) void dp_gather_kernel(DpSrc s, float* __restrict__ ga, int64_t n) {
    const int64_t nvec = n / 4, total = nvec + (n % 4 ? 1 : 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < nvec) {
            const int o = po_dp_slice_of(nvec, s.n, i);
            reinterpret_cast<float4*>(ga)[i] = *reinterpret_cast<const float4*>(s.p[o] + (4 * i - s.base[o]));
        } else {
            const int o = s.n - 1;
            for (int64_t e = 4 * nvec; e < n; ++e) ga[e] = s.p[o][e - s.base[o]];
        }
    }
}

inline unsigned dp_blocks(int64_t lanes) { return (unsigned)std::min<int64_t>((lanes + 255) / 256, 2048); }

std::atomic<int> g_route{PO_DP_ROUTE_AUTO};

// all R threads meet; reusable
struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int n = 0, waiting = 0;
    uint64_t gen = 0;
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t g = gen;
        if (++waiting == n) {
            waiting = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
};

// a replica's host thread: bound to its device once, runs one job at a time
struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    bool has = false, done = false, quit = false;
    int rc = PO_OK;
    std::string err;
};

struct Member {
    int device = 0;
    po_trainer* tr = nullptr;        // NULL: po_dp_allreduce_h's buffers alone
    float* ga = nullptr;             // the accumulator (the trainer's, or this member's own)
    int64_t own_count = 0;
    int64_t* count = nullptr;        // contributions since it was emptied
    hipStream_t stream = nullptr;
    float *stage = nullptr, *inbuf = nullptr, *hsend = nullptr;   // staging vector [n]; HOST route: the peers' slices [R][slot], pinned copy [n]
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

struct Core {
    int R = 0;
    int64_t n = 0, slot = 0;         // elements; the longest slice, rounded up to whole 16-byte groups
    std::vector<Member> mem;
    std::vector<std::unique_ptr<Worker>> wk;
    float* hres = nullptr;           // HOST route: the reduced vector, pinned, every owner writes its slice
    Barrier bar;
    std::atomic<bool> failed{false};
    int nopeer_a = -1, nopeer_b = -1;   // a pair of the group's devices without peer access (first found), or -1
    std::mutex peer_mu;
};

void worker_main(Core* c, int r) {
    Worker& w = *c->wk[(size_t)r];
    const bool bound = hipSetDevice(c->mem[(size_t)r].device) == hipSuccess;
    for (;;) {
        std::function<int()> job;
        {
            std::unique_lock<std::mutex> lk(w.mu);
            w.cv.wait(lk, [&] { return w.has || w.quit; });
            if (!w.has) return;
            job = std::move(w.job);
            w.has = false;
        }
        po_set_error("");
        int rc = bound ? job() : po_fail(PO_E_HIP, "hipSetDevice failed");
        {
            std::lock_guard<std::mutex> lk(w.mu);
            w.rc = rc;
            w.err = rc == PO_OK ? "" : po_last_error();
            w.done = true;
        }
        w.cv.notify_all();
    }
}

// fn(r) on the threads of the replicas in `who` (all at once), the first failure in replica order reported to the caller
int run_on(Core* c, const std::vector<int>& who, const std::function<int(int)>& fn) {
    for (int r : who) {
        Worker& w = *c->wk[(size_t)r];
        {
            std::lock_guard<std::mutex> lk(w.mu);
            w.job = [fn, r] { return fn(r); };
            w.has = true;
            w.done = false;
        }
        w.cv.notify_all();
    }
    int rc = PO_OK;
    std::string err;
    for (int r : who) {
        Worker& w = *c->wk[(size_t)r];
        std::unique_lock<std::mutex> lk(w.mu);
        w.cv.wait(lk, [&] { return w.done; });
        if (w.rc != PO_OK && rc == PO_OK) {
            rc = w.rc;
            err = "replica " + std::to_string(r) + " (device " + std::to_string(c->mem[(size_t)r].device) + "): " + w.err;
        }
    }
    if (rc != PO_OK) return po_fail(rc, err);
    return PO_OK;
}

std::vector<int> everyone(const Core* c) {
    std::vector<int> v((size_t)c->R);
    for (int r = 0; r < c->R; ++r) v[(size_t)r] = r;
    return v;
}

void start_workers(Core* c) {
    c->bar.n = c->R;
    for (int r = 0; r < c->R; ++r) c->wk.emplace_back(new Worker);
    for (int r = 0; r < c->R; ++r) c->wk[(size_t)r]->th = std::thread(worker_main, c, r);
}

void stop_workers(Core* c) {
    for (auto& w : c->wk) {
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->quit = true;
        }
        w->cv.notify_all();
        if (w->th.joinable()) w->th.join();
    }
    c->wk.clear();
}

// on replica r's thread: peer access from its device to every other device of the group, once
int enable_peers(Core* c, int r) {
    const int me = c->mem[(size_t)r].device;
    std::vector<int> seen;
    for (const Member& m : c->mem) {
        const int d = m.device;
        if (d == me || std::find(seen.begin(), seen.end(), d) != seen.end()) continue;
        seen.push_back(d);
        int can = 0;
        PO_HIPCHK(hipDeviceCanAccessPeer(&can, me, d));
        if (can) {
            const hipError_t e = hipDeviceEnablePeerAccess(d, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else if (e != hipSuccess) can = 0, (void)hipGetLastError();
        }
        if (!can) {
            std::lock_guard<std::mutex> lk(c->peer_mu);
            if (c->nopeer_a < 0) { c->nopeer_a = me; c->nopeer_b = d; }
        }
    }
    return PO_OK;
}

// on replica r's thread: the reduce's own buffers (the accumulator and its stream are the member's already)
int alloc_reduce_buffers(Core* c, int r) {
    Member& m = c->mem[(size_t)r];
    const size_t bytes = std::max<size_t>((size_t)c->n * 4, 16);
    PO_HIPCHK(hipMalloc(&m.stage, bytes));
    PO_HIPCHK(hipMalloc(&m.inbuf, std::max<size_t>((size_t)c->R * c->slot * 4, 16)));
    PO_HIPCHK(hipHostMalloc(&m.hsend, bytes, hipHostMallocPortable));
    PO_HIPCHK(hipEventCreate(&m.ev0));
    PO_HIPCHK(hipEventCreate(&m.ev1));
    if (r == 0) PO_HIPCHK(hipHostMalloc(&c->hres, bytes, hipHostMallocPortable));
    return PO_OK;
}

void free_reduce_buffers(Core* c, int r) {
    Member& m = c->mem[(size_t)r];
    if (m.stage) (void)hipFree(m.stage);
    if (m.inbuf) (void)hipFree(m.inbuf);
    if (m.hsend) (void)hipHostFree(m.hsend);
    if (m.ev0) (void)hipEventDestroy(m.ev0);
    if (m.ev1) (void)hipEventDestroy(m.ev1);
    if (r == 0 && c->hres) (void)hipHostFree(c->hres);
    m.stage = m.inbuf = m.hsend = nullptr;
    m.ev0 = m.ev1 = nullptr;
    if (r == 0) c->hres = nullptr;
}

void set_slot(Core* c) {
    int64_t longest = 0;
    for (int r = 0; r < c->R; ++r) {
        int64_t e0, e1;
        po_dp_slice_elems(c->n, c->R, r, &e0, &e1);
        longest = std::max(longest, e1 - e0);
    }
    c->slot = (longest + 3) / 4 * 4;
}

// a phase of the reduce on replica r's thread: what fails marks the group, everyone still meets at the barriers
#define DP_STEP(x)                                                      \
    do {                                                                \
        if (rc == PO_OK && !c->failed.load()) {                         \
            const hipError_t e_ = (x);                                  \
            if (e_ != hipSuccess) { rc = po_fail_hip(e_, #x); c->failed.store(true); } \
        }                                                               \
    } while (0)

// the all-reduce on replica r's thread.  contrib: the contributing replicas, ascending.  Every accumulator is at rest when this
// starts (po_train_accumulate and the loads return after a stream synchronise, and run_on is a host barrier)
int reduce_on(Core* c, int r, bool host, const std::vector<int>& contrib, float* ms_h) {
    Member& m = c->mem[(size_t)r];
    const bool mine = std::find(contrib.begin(), contrib.end(), r) != contrib.end();
    int64_t e0, e1;
    po_dp_slice_elems(c->n, c->R, r, &e0, &e1);
    const int64_t nvec = c->n / 4;
    const int64_t g0 = po_dp_slice_begin(nvec, c->R, r), g1 = po_dp_slice_begin(nvec, c->R, r + 1);
    const int64_t t0 = r == c->R - 1 ? 4 * nvec : c->n, t1 = c->n;
    const int64_t lanes = (g1 - g0) + (t1 > t0 ? 1 : 0);
    int rc = PO_OK;
    if (ms_h && r == 0) DP_STEP(hipEventRecord(m.ev0, m.stream));
    DpSrc src;
    std::memset(&src, 0, sizeof(src));
    src.n = (int)contrib.size();
    if (host) {
        // every contributing accumulator to its pinned copy; then slice r of each peer's copy up to this device
        if (mine) DP_STEP(hipMemcpyAsync(m.hsend, m.ga, (size_t)c->n * 4, hipMemcpyDeviceToHost, m.stream));
        DP_STEP(hipStreamSynchronize(m.stream));
        c->bar.wait();
        for (size_t k = 0; k < contrib.size(); ++k) {
            const int s = contrib[k];
            if (s == r) {
                src.p[k] = m.ga;
                src.base[k] = 0;
            } else {
                float* in = m.inbuf + (int64_t)k * c->slot;
                if (e1 > e0)
                    DP_STEP(hipMemcpyAsync(in, c->mem[(size_t)s].hsend + e0, (size_t)(e1 - e0) * 4, hipMemcpyHostToDevice, m.stream));
                src.p[k] = in;
                src.base[k] = e0;
            }
        }
    } else {
        for (size_t k = 0; k < contrib.size(); ++k) {
            src.p[k] = c->mem[(size_t)contrib[k]].ga;
            src.base[k] = 0;
        }
    }
    if (lanes > 0 && rc == PO_OK && !c->failed.load()) {
        hipLaunchKernelGGL(dp_reduce_slice_kernel, dim3(dp_blocks(lanes)), dim3(256), 0, m.stream, src, m.stage, g0, g1, t0, t1);
        DP_STEP(hipGetLastError());
    }
    if (host && e1 > e0) DP_STEP(hipMemcpyAsync(c->hres + e0, m.stage + e0, (size_t)(e1 - e0) * 4, hipMemcpyDeviceToHost, m.stream));
    DP_STEP(hipStreamSynchronize(m.stream));
    c->bar.wait();     // every slice is summed (and no accumulator is read any more) before any accumulator is written
    DpSrc own;
    std::memset(&own, 0, sizeof(own));
    own.n = c->R;
    if (host) DP_STEP(hipMemcpyAsync(m.stage, c->hres, (size_t)c->n * 4, hipMemcpyHostToDevice, m.stream));
    for (int o = 0; o < c->R; ++o) own.p[o] = host ? m.stage : c->mem[(size_t)o].stage;
    if (rc == PO_OK && !c->failed.load()) {
        const int64_t total = nvec + (c->n % 4 ? 1 : 0);
        hipLaunchKernelGGL(dp_gather_kernel, dim3(dp_blocks(total)), dim3(256), 0, m.stream, own, m.ga, c->n);
        DP_STEP(hipGetLastError());
    }
    if (ms_h && r == 0) DP_STEP(hipEventRecord(m.ev1, m.stream));
    DP_STEP(hipStreamSynchronize(m.stream));
    if (ms_h && r == 0) DP_STEP(hipEventElapsedTime(ms_h, m.ev0, m.ev1));
    c->bar.wait();     // no staging vector is rewritten by a next reduce while a peer still reads it
    return rc;
}

// the all-reduce of the group's accumulators under the current route; afterwards each holds the sum and counts one contribution
int reduce(Core* c, const char* me, float* ms_h) {
    std::vector<int> contrib;
    for (int r = 0; r < c->R; ++r)
        if (*c->mem[(size_t)r].count > 0) contrib.push_back(r);
    if (contrib.empty()) return po_fail(PO_E_ARG, std::string(me) + ": nothing is accumulated on any replica");
    const int route = g_route.load();
    if (route == PO_DP_ROUTE_PEER && c->nopeer_a >= 0)
        return po_fail(PO_E_UNSUPPORTED, std::string(me) + ": PO_DP_ROUTE_PEER, but device " + std::to_string(c->nopeer_a) +
                       " has no peer access to device " + std::to_string(c->nopeer_b));
    if (ms_h) *ms_h = 0.f;
    if (c->R > 1) {
        const bool host = route == PO_DP_ROUTE_HOST || (route == PO_DP_ROUTE_AUTO && c->nopeer_a >= 0);
        c->failed.store(false);
        const int rc = run_on(c, everyone(c), [&](int r) { return reduce_on(c, r, host, contrib, ms_h); });
        if (rc != PO_OK) return rc;
    }
    for (Member& m : c->mem) *m.count = 1;
    return PO_OK;
}

int check_devices(const std::string& me, const int* devices_h, int R) {
    if (!devices_h) return po_fail(PO_E_ARG, me + ": null argument devices_h");
    if (R < 1 || R > PO_DP_MAX_REPLICAS)
        return po_fail(PO_E_ARG, me + ": " + std::to_string(R) + " replicas (1 to " + std::to_string(PO_DP_MAX_REPLICAS) + ")");
    const int nd = po_device_count();
    for (int r = 0; r < R; ++r)
        if (devices_h[r] < 0 || devices_h[r] >= nd)
            return po_fail(PO_E_ARG, me + ": replica " + std::to_string(r) + " names device " + std::to_string(devices_h[r]) +
                           ", " + std::to_string(nd) + " visible");
    return PO_OK;
}

}  // namespace

struct po_train_group {
    Core core;
    int max_batch = 0, T = 0;
    int64_t nw = 0;
};

namespace {

void group_free(po_train_group* g) {
    Core* c = &g->core;
    if (!c->wk.empty())
        (void)run_on(c, everyone(c), [&](int r) {
            Member& m = c->mem[(size_t)r];
            if (m.stream) (void)hipStreamSynchronize(m.stream);
            free_reduce_buffers(c, r);
            if (m.tr) po_train_destroy(m.tr);
            m.tr = nullptr;
            return PO_OK;
        });
    stop_workers(c);
    delete g;
}

// the micro-batches of a group call: replica r's n_h[r] windows follow replica r - 1's in every array
struct Shares {
    std::vector<int> who;            // the replicas with windows
    std::vector<int64_t> win, lab;   // [R + 1] the first window and the first label of each replica's share
};

int plan_shares(const po_train_group* g, const std::string& me, const int* n_h, const int32_t* label_len_h, Shares* s) {
    const int R = g->core.R;
    s->win.assign((size_t)R + 1, 0);
    s->lab.assign((size_t)R + 1, 0);
    for (int r = 0; r < R; ++r) {
        if (n_h[r] < 0 || n_h[r] > g->max_batch)
            return po_fail(PO_E_ARG, me + ": replica " + std::to_string(r) + " is given " + std::to_string(n_h[r]) +
                           " windows, a replica holds 0 to " + std::to_string(g->max_batch));
        s->win[(size_t)r + 1] = s->win[(size_t)r] + n_h[r];
        if (n_h[r] > 0) s->who.push_back(r);
    }
    if (s->who.empty()) return po_fail(PO_E_ARG, me + ": no replica is given a window");
    for (int r = 0; r < R; ++r) {
        int64_t l = 0;
        for (int64_t w = s->win[(size_t)r]; w < s->win[(size_t)r + 1]; ++w) l += std::max<int32_t>(label_len_h[w], 0);
        s->lab[(size_t)r + 1] = s->lab[(size_t)r] + l;
    }
    return PO_OK;
}

// every replica's checks of its share, under the single-trainer entry's name, before any replica launches
int check_shares(const po_train_group* g, const char* entry, const int* n_h, const int32_t* labels_h, const int32_t* label_len_h,
                 int merge_repeated, const Shares& s) {
    for (int r : s.who) {
        const int rc = po_trainer_check_batch(g->core.mem[(size_t)r].tr, entry, n_h[r], labels_h ? labels_h + s.lab[(size_t)r] : nullptr,
                                              label_len_h + s.win[(size_t)r], merge_repeated);
        if (rc != PO_OK)
            return po_fail(rc, "replica " + std::to_string(r) + " (device " + std::to_string(g->core.mem[(size_t)r].device) +
                           "): " + po_last_error());
    }
    return PO_OK;
}

int bad_replica(const po_train_group* g, const std::string& me, int replica) {
    return po_fail(PO_E_ARG, me + ": replica " + std::to_string(replica) + " (the group has " + std::to_string(g->core.R) + ")");
}

}  // namespace

extern "C" {

int po_set_dp_route(int route) {
    po_set_error("");
    if (route != PO_DP_ROUTE_AUTO && route != PO_DP_ROUTE_PEER && route != PO_DP_ROUTE_HOST)
        return po_fail(PO_E_ARG, "po_set_dp_route: route " + std::to_string(route) +
                       " (PO_DP_ROUTE_AUTO, PO_DP_ROUTE_PEER or PO_DP_ROUTE_HOST)");
    g_route.store(route);
    return PO_OK;
}

int po_get_dp_route(void) { return g_route.load(); }

po_train_group* po_train_group_create(const po_call_layer* layers_h, int n_layers, int max_batch, int T, const int* devices_h,
                                      int n_replicas) {
    po_set_error("");
    // ---- every argument error, before the first allocation (the model's own: po_train_create's, on replica 0, before its first)
    if (!layers_h) { po_fail(PO_E_ARG, "po_train_group_create: null argument layers_h"); return nullptr; }
    if (check_devices("po_train_group_create", devices_h, n_replicas) != PO_OK) return nullptr;
    if (max_batch < 1 || T < 1) { po_fail(PO_E_ARG, "po_train_group_create: max_batch and T must be positive"); return nullptr; }
    po_train_group* g = new po_train_group;
    Core* c = &g->core;
    c->R = n_replicas;
    c->mem.resize((size_t)n_replicas);
    for (int r = 0; r < n_replicas; ++r) c->mem[(size_t)r].device = devices_h[r];
    g->max_batch = max_batch;
    g->T = T;
    start_workers(c);
    auto make = [&](int r) {
        Member& m = c->mem[(size_t)r];
        m.tr = po_train_create(layers_h, n_layers, max_batch, T);
        if (!m.tr) return PO_E_ARG;     // (po_train_create's message stands)
        po_trainer_accum v;
        int rc = po_trainer_accum_view(m.tr, &v);
        if (rc != PO_OK) return rc;
        m.ga = v.ga;
        m.count = v.count;
        m.stream = v.stream;
        if (r == 0) {
            c->n = g->nw = v.n;
            set_slot(c);
        }
        return PO_OK;
    };
    // replica 0 first: a model that is refused is refused once, with nothing else made; peer access before the peers' memory
    int rc = run_on(c, {0}, make);
    if (rc == PO_OK) rc = run_on(c, everyone(c), [&](int r) { return enable_peers(c, r); });
    if (rc == PO_OK && n_replicas > 1) {
        std::vector<int> rest;
        for (int r = 1; r < n_replicas; ++r) rest.push_back(r);
        rc = run_on(c, rest, make);
    }
    if (rc == PO_OK) rc = run_on(c, everyone(c), [&](int r) { return alloc_reduce_buffers(c, r); });
    if (rc != PO_OK) {
        const std::string keep = po_last_error();
        group_free(g);
        po_set_error(keep.c_str());
        return nullptr;
    }
    return g;
}

void po_train_group_destroy(po_train_group* g) {
    if (g) group_free(g);
}

int po_train_group_size(po_train_group* g) {
    po_set_error("");
    if (!g) return po_fail(PO_E_ARG, "po_train_group_size: null group");
    return g->core.R;
}

int po_train_group_set_params(po_train_group* g, const float* w_h, int64_t n) {
    po_set_error("");
    if (!g || !w_h) return po_fail(PO_E_ARG, std::string("po_train_group_set_params: null argument ") + (!g ? "g" : "w_h"));
    if (n != g->nw) return po_fail(PO_E_ARG, "po_train_group_set_params: the model has " + std::to_string(g->nw) + " weights, " +
                                   std::to_string(n) + " given");
    Core* c = &g->core;
    return run_on(c, everyone(c), [&](int r) { return po_train_set_params(c->mem[(size_t)r].tr, w_h, n); });
}

int po_train_group_get_replica_params(po_train_group* g, int replica, float* w_h, int64_t n) {
    po_set_error("");
    if (!g || !w_h) return po_fail(PO_E_ARG, std::string("po_train_group_get_replica_params: null argument ") + (!g ? "g" : "w_h"));
    if (replica < 0 || replica >= g->core.R) return bad_replica(g, "po_train_group_get_replica_params", replica);
    Core* c = &g->core;
    return run_on(c, {replica}, [&](int r) { return po_train_get_params(c->mem[(size_t)r].tr, w_h, n); });
}

int po_train_group_get_params(po_train_group* g, float* w_h, int64_t n) {
    po_set_error("");
    if (!g || !w_h) return po_fail(PO_E_ARG, std::string("po_train_group_get_params: null argument ") + (!g ? "g" : "w_h"));
    return po_train_group_get_replica_params(g, 0, w_h, n);
}

int po_train_group_set_state(po_train_group* g, const float* m_h, const float* v_h, int64_t n, int64_t step) {
    po_set_error("");
    if (!g || !m_h || !v_h)
        return po_fail(PO_E_ARG, std::string("po_train_group_set_state: null argument ") + (!g ? "g" : !m_h ? "m_h" : "v_h"));
    if (n != g->nw) return po_fail(PO_E_ARG, "po_train_group_set_state: n " + std::to_string(n) + " (the model has " +
                                   std::to_string(g->nw) + " weights)");
    if (step < 0) return po_fail(PO_E_ARG, "po_train_group_set_state: step " + std::to_string(step) + " (0 or more)");
    Core* c = &g->core;
    return run_on(c, everyone(c), [&](int r) { return po_train_set_state(c->mem[(size_t)r].tr, m_h, v_h, n, step); });
}

int po_train_group_get_replica_state(po_train_group* g, int replica, float* m_h, float* v_h, int64_t n, int64_t* step_h) {
    po_set_error("");
    if (!g || !m_h || !v_h || !step_h)
        return po_fail(PO_E_ARG, std::string("po_train_group_get_replica_state: null argument ") +
                       (!g ? "g" : !m_h ? "m_h" : !v_h ? "v_h" : "step_h"));
    if (replica < 0 || replica >= g->core.R) return bad_replica(g, "po_train_group_get_replica_state", replica);
    Core* c = &g->core;
    return run_on(c, {replica}, [&](int r) { return po_train_get_state(c->mem[(size_t)r].tr, m_h, v_h, n, step_h); });
}

int po_train_group_get_state(po_train_group* g, float* m_h, float* v_h, int64_t n, int64_t* step_h) {
    po_set_error("");
    if (!g || !m_h || !v_h || !step_h)
        return po_fail(PO_E_ARG, std::string("po_train_group_get_state: null argument ") +
                       (!g ? "g" : !m_h ? "m_h" : !v_h ? "v_h" : "step_h"));
    return po_train_group_get_replica_state(g, 0, m_h, v_h, n, step_h);
}

int po_train_group_set_precision(po_train_group* g, int precision) {
    po_set_error("");
    if (!g) return po_fail(PO_E_ARG, "po_train_group_set_precision: null group");
    Core* c = &g->core;
    const int before = po_train_get_precision(c->mem[0].tr);
    // replica 0 first: a refusal (the value, the model's width) is every replica's, and then no replica has changed
    int rc = PO_OK, r = 0;
    for (; r < c->R && rc == PO_OK; ++r)
        rc = run_on(c, {r}, [&](int k) { return po_train_set_precision(c->mem[(size_t)k].tr, precision); });
    if (rc != PO_OK) {
        const std::string keep = po_last_error();
        for (int k = 0; k < r - 1; ++k)
            (void)run_on(c, {k}, [&](int q) { return po_train_set_precision(c->mem[(size_t)q].tr, before); });
        po_set_error(keep.c_str());
    }
    return rc;
}

int po_train_group_accumulate(po_train_group* g, const float* signal_h, const int* n_h, const int32_t* labels_h,
                              const int32_t* label_len_h, int merge_repeated, const float* weight_h, float* loss_h,
                              float* stage_ms_h) {
    const std::string me = "po_train_group_accumulate";
    po_set_error("");
    // ---- every refusal, every replica's, before any replica launches
    if (!g || !signal_h || !n_h || !label_len_h || !weight_h || !loss_h)
        return po_fail(PO_E_ARG, me + ": null argument " + (!g ? "g" : !signal_h ? "signal_h" : !n_h ? "n_h" : !label_len_h ? "label_len_h" :
                                                            !weight_h ? "weight_h" : "loss_h"));
    Shares s;
    int rc = plan_shares(g, me, n_h, label_len_h, &s);
    if (rc != PO_OK) return rc;
    for (int r : s.who)
        if (!std::isfinite(weight_h[r]))
            return po_fail(PO_E_ARG, me + ": replica " + std::to_string(r) + "'s weight " + std::to_string(weight_h[r]) + " (finite)");
    if ((rc = check_shares(g, "po_train_accumulate", n_h, labels_h, label_len_h, merge_repeated, s)) != PO_OK) return rc;
    Core* c = &g->core;
    const int T = g->T;
    return run_on(c, s.who, [&](int r) {
        const int64_t w0 = s.win[(size_t)r];
        return po_train_accumulate(c->mem[(size_t)r].tr, signal_h + w0 * T, n_h[r], labels_h ? labels_h + s.lab[(size_t)r] : nullptr,
                                   label_len_h + w0, merge_repeated, weight_h[r], loss_h + w0,
                                   stage_ms_h ? stage_ms_h + 5 * r : nullptr);
    });
}

int po_train_group_eval(po_train_group* g, const float* signal_h, const int* n_h, const int32_t* labels_h,
                        const int32_t* label_len_h, int merge_repeated, float* loss_h, int32_t* edit_h, int32_t* pred_len_h,
                        int32_t* status_h, uint8_t* pred_h, float* stage_ms_h) {
    const std::string me = "po_train_group_eval";
    po_set_error("");
    if (!g || !signal_h || !n_h || !label_len_h || !edit_h || !pred_len_h || !status_h) return po_fail(PO_E_ARG, me + ": null argument");
    Shares s;
    int rc = plan_shares(g, me, n_h, label_len_h, &s);
    if (rc != PO_OK) return rc;
    if ((rc = check_shares(g, "po_train_eval", n_h, labels_h, label_len_h, merge_repeated, s)) != PO_OK) return rc;
    Core* c = &g->core;
    const int T = g->T;
    return run_on(c, s.who, [&](int r) {
        const int64_t w0 = s.win[(size_t)r];
        return po_train_eval(c->mem[(size_t)r].tr, signal_h + w0 * T, n_h[r], labels_h ? labels_h + s.lab[(size_t)r] : nullptr,
                             label_len_h + w0, merge_repeated, loss_h ? loss_h + w0 : nullptr, edit_h + w0, pred_len_h + w0,
                             status_h + w0, pred_h ? pred_h + w0 * T : nullptr, stage_ms_h ? stage_ms_h + 3 * r : nullptr);
    });
}

int po_train_group_get_accum(po_train_group* g, int replica, float* g_h, int64_t n) {
    po_set_error("");
    if (!g || !g_h) return po_fail(PO_E_ARG, std::string("po_train_group_get_accum: null argument ") + (!g ? "g" : "g_h"));
    if (replica < 0 || replica >= g->core.R) return bad_replica(g, "po_train_group_get_accum", replica);
    Core* c = &g->core;
    return run_on(c, {replica}, [&](int r) { return po_train_get_accum(c->mem[(size_t)r].tr, g_h, n); });
}

int po_train_group_set_accum(po_train_group* g, int replica, const float* g_h, int64_t n) {
    po_set_error("");
    if (!g || !g_h) return po_fail(PO_E_ARG, std::string("po_train_group_set_accum: null argument ") + (!g ? "g" : "g_h"));
    if (replica < 0 || replica >= g->core.R) return bad_replica(g, "po_train_group_set_accum", replica);
    Core* c = &g->core;
    return run_on(c, {replica}, [&](int r) { return po_train_set_accum(c->mem[(size_t)r].tr, g_h, n); });
}

int po_train_group_reduce(po_train_group* g, float* ms_h) {
    po_set_error("");
    if (!g) return po_fail(PO_E_ARG, "po_train_group_reduce: null group");
    return reduce(&g->core, "po_train_group_reduce", ms_h);
}

int po_train_group_apply(po_train_group* g, float lr, float beta1, float beta2, float eps, float weight_decay, float clip_norm,
                         double* grad_norm_h, int* applied_h) {
    po_set_error("");
    // ---- every refusal, before any launch (po_train_apply's own, once for all)
    if (!g) return po_fail(PO_E_ARG, "po_train_group_apply: null group");
    if (!(clip_norm >= 0.f) || !std::isfinite(clip_norm))
        return po_fail(PO_E_ARG, "po_train_group_apply: clip_norm " + std::to_string(clip_norm) + " (0: no clipping, or positive and finite)");
    if (!(weight_decay >= 0.f) || !std::isfinite(weight_decay))
        return po_fail(PO_E_ARG, "po_train_group_apply: weight_decay " + std::to_string(weight_decay) + " (0 or positive and finite)");
    Core* c = &g->core;
    int rc = reduce(c, "po_train_group_apply", nullptr);
    if (rc != PO_OK) return rc;
    std::vector<double> norm((size_t)c->R, 0.0);
    std::vector<int> applied((size_t)c->R, 0);
    rc = run_on(c, everyone(c), [&](int r) {
        return po_train_apply(c->mem[(size_t)r].tr, lr, beta1, beta2, eps, weight_decay, clip_norm, &norm[(size_t)r], &applied[(size_t)r]);
    });
    if (rc != PO_OK) return rc;
    if (grad_norm_h) *grad_norm_h = norm[0];
    if (applied_h) *applied_h = applied[0];
    return PO_OK;
}

int po_dp_allreduce_h(const int* devices_h, int R, const float* const* bufs_h, const int* present_h, int64_t n,
                      float* const* out_h) {
    const std::string me = "po_dp_allreduce_h";
    po_set_error("");
    // ---- every argument error, before the first allocation
    int rc = check_devices(me, devices_h, R);
    if (rc != PO_OK) return rc;
    if (!bufs_h || !present_h || !out_h)
        return po_fail(PO_E_ARG, me + ": null argument " + (!bufs_h ? "bufs_h" : !present_h ? "present_h" : "out_h"));
    if (n < 0) return po_fail(PO_E_ARG, me + ": n " + std::to_string(n));
    if (n == 0) return PO_OK;
    bool any = false;
    for (int r = 0; r < R; ++r) {
        if (present_h[r] && !bufs_h[r]) return po_fail(PO_E_ARG, me + ": replica " + std::to_string(r) + " is present and has a null buffer");
        if (!out_h[r]) return po_fail(PO_E_ARG, me + ": null out_h[" + std::to_string(r) + "]");
        any = any || present_h[r];
    }
    if (!any) return po_fail(PO_E_ARG, me + ": no replica is present");
    std::unique_ptr<Core> core(new Core);
    Core* c = core.get();
    c->R = R;
    c->n = n;
    c->mem.resize((size_t)R);
    for (int r = 0; r < R; ++r) c->mem[(size_t)r].device = devices_h[r];
    set_slot(c);
    start_workers(c);
    rc = run_on(c, everyone(c), [&](int r) { return enable_peers(c, r); });
    if (rc == PO_OK)
        rc = run_on(c, everyone(c), [&](int r) {
            Member& m = c->mem[(size_t)r];
            m.count = &m.own_count;
            PO_HIPCHK(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
            PO_HIPCHK(hipMalloc(&m.ga, (size_t)n * 4));
            if (present_h[r]) {
                PO_HIPCHK(hipMemcpy(m.ga, bufs_h[r], (size_t)n * 4, hipMemcpyHostToDevice));
                m.own_count = 1;
            }
            return alloc_reduce_buffers(c, r);
        });
    if (rc == PO_OK) rc = reduce(c, "po_dp_allreduce_h", nullptr);
    if (rc == PO_OK)
        rc = run_on(c, everyone(c), [&](int r) {
            PO_HIPCHK(hipMemcpy(out_h[r], c->mem[(size_t)r].ga, (size_t)n * 4, hipMemcpyDeviceToHost));
            return PO_OK;
        });
    const std::string keep = po_last_error();
    (void)run_on(c, everyone(c), [&](int r) {
        Member& m = c->mem[(size_t)r];
        if (m.stream) (void)hipStreamSynchronize(m.stream);
        free_reduce_buffers(c, r);
        if (m.ga) (void)hipFree(m.ga);
        if (m.stream) (void)hipStreamDestroy(m.stream);
        return PO_OK;
    });
    stop_workers(c);
    po_set_error(keep.c_str());
    return rc;
}

}  // extern "C"
