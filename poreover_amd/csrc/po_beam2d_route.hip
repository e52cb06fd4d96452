// The host layer of the batched pair (2-D) CTC beam search: which kernel family takes a launch, with which process-wide
// settings, and on what memory — beam2d_reg_kernel (po_beam2d_reg.hip; its pre-pass and walk kernels, po_beam2d_pre.h, are compiled
// here), beam2d_kernel (po_beam2d.hip) or beam2d_grid_kernel (po_beam2d_grid.hip).  The kernel files keep no process-wide state:
// the settings below reach their launch functions in a PoB2Call (po_internal.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#define PO_WANT_ZERO_KERNEL 1
#include "po_device.h"
#include "po_host.h"
#include "po_beam2d_common.h"
#include "po_beam2d_pre.h"

namespace {
// The order in which a launch's persistent workgroups take their pairs: longest first (frames of both reads, 2048
// classes, descending; within a class as the atomics fall).  The tail of a launch — the last pair of every workgroup,
// running on a half-empty device — is then made of the SHORTEST pairs instead of whatever came last in the input:
// worth a few percent on the bench's pairs (lengths within 10 %), most of the tail on real reads, whose lengths differ
// tenfold.  Results do not depend on it (every pair is decoded by one workgroup, alone).  One workgroup: a histogram,
// its prefix sums and a scatter, all in LDS.
constexpr int ORD_BINS = 2048;
__global__ __launch_bounds__(1024) void pair_order_kernel(const int64_t* y1_off, const int64_t* y2_off, int n, int* order) {
    __shared__ int hist[ORD_BINS];
    __shared__ int part[1024 / 64];
    __shared__ long long cmax_s;
    const int tid = threadIdx.x;
    for (int b = tid; b < ORD_BINS; b += 1024) hist[b] = 0;
    if (tid == 0) cmax_s = 1;
    __syncthreads();
    long long cm = 1;
    for (int i = tid; i < n; i += 1024) cm = max(cm, (long long)((y1_off[i + 1] - y1_off[i]) + (y2_off[i + 1] - y2_off[i])));
    atomicMax((unsigned long long*)&cmax_s, (unsigned long long)cm);
    __syncthreads();
    const long long cmax = cmax_s;
    auto bin_of = [&](int i) -> int {
        const long long c = (y1_off[i + 1] - y1_off[i]) + (y2_off[i + 1] - y2_off[i]);
        const long long b = (max(c, 0ll) * (ORD_BINS - 1)) / cmax;
        return ORD_BINS - 1 - (int)min(b, (long long)(ORD_BINS - 1));   // longest -> bin 0
    };
    for (int i = tid; i < n; i += 1024) atomicAdd(&hist[bin_of(i)], 1);
    __syncthreads();
    // exclusive prefix sums of the 2048 counts: two per thread, wave scan, wave totals through LDS
    const int c0 = hist[2 * tid], c1 = hist[2 * tid + 1];
    int v = c0 + c1;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o); if (lane >= o) v += t; }
    if (lane == 63) part[wave] = v;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += part[w];
    __syncthreads();
    const int ex = base + v - (c0 + c1);
    hist[2 * tid] = ex; hist[2 * tid + 1] = ex + c0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) order[atomicAdd(&hist[bin_of(i)], 1)] = i;
}

// Kernel routing is a process-wide setting of the library (po_set_pair_route), not something a launch looks up in the
// environment: PO_ROUTE_AUTO (the engine's choice: beam2d_reg_kernel wherever it applies — row_col with an envelope, W <= 12,
// every tree model — and beam2d_kernel elsewhere), PO_ROUTE_REG (the same, named), PO_ROUTE_LEGACY (always beam2d_kernel) —
// for the tests, which run the pair path on both kernels, and for A/B timing.  The route's eleven environment variables only give
// INITIAL values and are all read HERE, once, when the library is first used, so that a workspace size and the launch that
// follows always agree.  (All but PO_REG_FIXED_SHAPE, PO_REG_POOL_SLICES and PO_REG_PERSIST are tested for PRESENCE: any value,
// "0" included, switches them on — ADVICE.md.)
struct B2Route { int route, defer_odd, debug_occ, no_order, reg_auto, chain_scan, reg_fixed, force_wide, pool_slices, persist; };
B2Route& b2_route() {
    static B2Route r = [] {
        B2Route x;
        // PO_B2_LEGACY: beam2d_kernel for every launch; PO_REG_FORCE: PO_ROUTE_REG (po_set_pair_route)
        x.route = getenv("PO_B2_LEGACY") ? PO_ROUTE_LEGACY : (getenv("PO_REG_FORCE") ? PO_ROUTE_REG : PO_ROUTE_AUTO);
        x.reg_auto = getenv("PO_REG_NEVER") ? 0 : 1;      // A/B: PO_ROUTE_AUTO chooses beam2d_kernel for everything
        x.defer_odd = getenv("PO_X2_DEFER_ODD") ? 1 : 0;  // test hook: every odd pair is handed to beam2d_kernel (po_set_pair_route)
        x.no_order = getenv("PO_B2_NO_ORDER") ? 1 : 0;    // A/B: pairs taken in input order
        x.debug_occ = getenv("PO_DEBUG_OCC") ? 1 : 0;     // the slice pool reports on stderr what it allocates
        x.chain_scan = getenv("PO_CHAIN_CLOSED") ? PO_CHAIN_CLOSED_FORM : PO_CHAIN_SERIAL;   // (po_set_chain_mode)
        {   // (po_set_reg_fixed_shape; PO_REG_FIXED_SHAPE=0: the run-time kernel for the default shape as well)
            const char* e = getenv("PO_REG_FIXED_SHAPE");
            x.reg_fixed = (e && atoi(e) == 0) ? 0 : 1;
        }
        x.force_wide = getenv("PO_REG_FORCE_WIDE") ? 1 : 0;   // experiments: the 64-slot layout for every width
        {   // PO_REG_POOL_SLICES: a smaller pool — several processes sharing one board, each with its own 9 GB otherwise; launches
            // are cut to that many waves (0: the device's own number; reg_pool takes values from 64 up to that number)
            const char* e = getenv("PO_REG_POOL_SLICES");
            x.pool_slices = e ? atoi(e) : 0;
        }
        {   // PO_REG_PERSIST=0 / 1 pins the launch form (A/B; -1: the engine's, persistent waves)
            const char* e = getenv("PO_REG_PERSIST");
            x.persist = e ? atoi(e) : -1;
        }
        return x;
    }();
    return r;
}
// profiling hooks (po_profile_*, po_capi.hip): handed to every launch
unsigned long long* g_b2_upd_counter = nullptr;                // po_b2_set_update_counter
void (*g_b2_mark)(int begin, hipStream_t stream) = nullptr;   // po_b2_set_mark: brackets the main pair beam kernel
// the queue's order for a launch (PoB2Call::order)
void pair_order(const int64_t* y1_off, const int64_t* y2_off, int n, int* order, hipStream_t stream) {
    hipLaunchKernelGGL(pair_order_kernel, dim3(1), dim3(1024), 0, stream, y1_off, y2_off, n, order);
}
// The register-state kernel (beam2d_reg_kernel, po_beam2d_reg.hip) with its batch-parallel pre-pass and walk kernels
// (po_beam2d_pre.h): the engine's choice (PO_ROUTE_AUTO) for row_col with an envelope at every batch size, every tree
// model, W <= 12.  PO_REG_NEVER / PO_ROUTE_LEGACY send everything to beam2d_kernel.
struct RegGeom {
    int blocks;        // pair waves (one-wave workgroups) of this launch
    size_t off_queue, off_meta, off_nmain, off_sched, off_envt, off_order, off_fb, fb_bytes, total;
};
// the 64-slot layout of the kernel (lane = element slot, the two reads one after the other): 7 <= W <= 12
inline int reg_wide(int W) { return (W > 6 || b2_route().force_wide) ? 1 : 0; }
struct RegPool;
RegPool* reg_pool(int model, int wide);
bool reg_eligible(int n, int W, int A, int model, int method) {
    const int rt = b2_route().route;
    // (every tree model since round 5: the kernel is templated on the model's values per entry)
    if (!(method == PO_METHOD_ROW_COL && W <= 12 && A >= 1 && W * (A + 1) <= po_reg_max_elements(reg_wide(W)))) return false;
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE && model != PO_MODEL_FLIPFLOP) return false;
    if (!(rt == PO_ROUTE_REG || (rt == PO_ROUTE_AUTO && b2_route().reg_auto != 0))) return false;
    // The route needs the library's slice pool (below).  It is made HERE — by the workspace-size query that precedes every
    // launch, a host-side call — and not inside the enqueue-only launch (multi-GB hipMalloc calls, a memset and a
    // copy on the null stream do not belong in a stream capture).  A pool that cannot be allocated is remembered as such: the size
    // query then answers for beam2d_kernel and the launch takes that kernel — the two always agree.
    {   // (a host without a device can only PLAN — the CPU tests' size queries: answer for the engine's route)
        static const bool no_device = [] { int nd = 0; const bool none = hipGetDeviceCount(&nd) != hipSuccess || nd <= 0; (void)hipGetLastError(); return none; }();
        if (no_device) return true;
    }
    return reg_pool(model, reg_wide(W)) != nullptr;
}

// ---- The library's SLICE POOL of the register-state kernel (one per device, tree model and lane layout; made at the first
// launch that needs it, kept for the life of the process).  A slice = the value store of one pair wave (2 - 8 MB: 128 row
// groups at R = 128) + its tree arena.  Rounds 1 - 4 carved these out of every call's workspace: 12 GB for a 10 000-pair call,
// 28 GB per slot of a pipeline — and a hipMalloc of that size stalls for 0.5 - 2.5 s on this driver every now and then
// (scripts/micro/malloc_cost.hip: never below 4 GB, one in three at 16 GB), which is what a process's FIRST call paid.
// There are never more pair waves on the device than its register file and LDS admit, whatever the number of launches in
// flight: ONE pool of that many slices serves them all, in chunks of at most 3.5 GB; a wave claims a slice when it starts
// (po_beam2d_reg.hip).  The slices hold VALUES only (no tags, no epochs: presence is bookkeeping in the kernel), so nothing is ever
// memset or cleared.  po_reg_pool_prewarm makes a pool ahead of the first launch, po_reg_pool_release frees the current device's.
struct RegPool {
    int nslices = 0, spc_log2 = 0;
    size_t pool_bytes = 0, slice_bytes = 0;
    long long arena_cap = 0;
    char* chunk[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int* claim = nullptr;
    char* words = nullptr;                       // the allocation claim / defer_count / tickets live in
    unsigned long long* defer_count = nullptr;   // pairs handed to beam2d_kernel since the last reset (tests)
    unsigned* tickets = nullptr;                 // {take, give} tickets of the ring of free slices (claim)
};
std::mutex g_reg_pool_mu;
RegPool* g_reg_pools[PO_MAX_DEVICES][6] = {};
bool g_reg_pool_failed[PO_MAX_DEVICES][6] = {};   // (sticky until po_reg_pool_release: the size query and the launch must agree)
inline int reg_pool_key(int model, int wide) { return (model == PO_MODEL_CTC ? 0 : (model == PO_MODEL_MERGE ? 1 : 2)) * 2 + (wide ? 1 : 0); }
RegPool* reg_pool(int model, int wide) {
    const int dev = po_cur_device();
    const int key = reg_pool_key(model, wide);
    std::lock_guard<std::mutex> lk(g_reg_pool_mu);
    if (g_reg_pools[dev][key]) return g_reg_pools[dev][key];
    if (g_reg_pool_failed[dev][key]) return nullptr;
    RegPool* p = new RegPool();
    p->nslices = po_dev_info().cus * po_reg_slots_per_cu(model, wide);
    if (const int v = b2_route().pool_slices; v >= 64 && v < p->nslices) p->nslices = v & ~1;   // (PO_REG_POOL_SLICES)
    p->pool_bytes = po_reg_pool_bytes(model, wide);
    // tree nodes a slice's arena holds: four per node that ever enters the beam.  1 024 beam entries per beam slot is ~ 4 x what
    // a T = 4000 pair makes; a pair that needs more is handed to beam2d_kernel (whose arenas are worst-case sized)
    const long long WM = wide ? 12 : 6;
    p->arena_cap = 1 + PO_A + (long long)PO_A * WM * 1024;
    // (+ the row headers: one int per store row and read)
    p->slice_bytes = al256(p->pool_bytes + sizeof(int) * 3 * (size_t)p->arena_cap + sizeof(int) * 2 * PO_A * (size_t)po_reg_ngl(wide));
    int spc = 1;
    while ((size_t)(2 * spc) * p->slice_bytes <= ((size_t)7 << 29) && 2 * spc <= p->nslices) spc *= 2;   // chunks of <= 3.5 GB
    while ((p->nslices + spc - 1) / spc > 8) spc *= 2;
    p->spc_log2 = 0;
    while ((1 << p->spc_log2) < spc) ++p->spc_log2;
    const int nchunks = (p->nslices + spc - 1) / spc;
    bool ok = true;
    for (int c = 0; c < nchunks && ok; ++c) {
        const int here = std::min(spc, p->nslices - c * spc);
        ok = hipMalloc((void**)&p->chunk[c], (size_t)here * p->slice_bytes) == hipSuccess;
    }
    // the ring of free slices (one int per slice), then — 256-byte aligned — the deferral counter and the two tickets
    const size_t ring = al256(sizeof(int) * (size_t)p->nslices), words = ring + 256;
    char* w = nullptr;
    ok = ok && hipMalloc((void**)&w, words) == hipSuccess && hipMemset(w, 0, words) == hipSuccess;
    if (ok) {   // every slice is free: ring word i holds slice i
        std::vector<int> ids((size_t)p->nslices);
        for (int i = 0; i < p->nslices; ++i) ids[(size_t)i] = i;
        ok = hipMemcpy(w, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        for (auto c : p->chunk) if (c) (void)hipFree(c);
        if (w) (void)hipFree(w);
        delete p;
        g_reg_pool_failed[dev][key] = true;
        if (b2_route().debug_occ) fprintf(stderr, "[po] register-state kernel pool (model %d, %s layout) could not be allocated: beam2d_kernel serves the route\n", model, wide ? "64-slot" : "32-slot");
        return nullptr;
    }
    p->words = w;
    p->claim = (int*)w;
    p->defer_count = (unsigned long long*)(w + ring);
    p->tickets = (unsigned*)(w + ring + 128);
    if (b2_route().debug_occ)
        fprintf(stderr, "[po] register-state kernel pool (model %d, %s layout): %d slices of %.2f MB in %d chunk(s)\n", model, wide ? "64-slot" : "32-slot",
                p->nslices, p->slice_bytes / 1048576.0, nchunks);
    g_reg_pools[dev][key] = p;
    return p;
}
// Per-call workspace of the route: the batch-sized arrays of the pre-pass and the walk, and the deferred-pairs pass.
RegGeom reg_geometry(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int W, int model) {
    (void)tr1;
    RegGeom g;
    g.blocks = po_dev_info().cus * po_reg_slots_per_cu(model, reg_wide(W));
    if (g.blocks > n) g.blocks = n > 0 ? n : 1;
    const size_t np = (size_t)(n > 0 ? n : 1);
    size_t o = 0;
    g.off_queue = o; o += 256;
    g.off_meta = o; o += al256(sizeof(int2) * np);
    g.off_nmain = o; o += al256(sizeof(int) * np);
    g.off_sched = o; o += al256(sizeof(int4) * (size_t)(tr2 > 0 ? tr2 : 1));
    g.off_envt = o; o += al256(sizeof(int) * 2 * (size_t)tr2);
    g.off_order = o; o += al256(sizeof(int) * np);   // the queue's order (pair_order_kernel)
    g.off_fb = o;
    g.fb_bytes = po_b2_legacy_ws_bytes(n, mr1, mr2, W, model, PO_METHOD_ROW_COL, REG_FB_BLOCKS);
    o += al256(g.fb_bytes);
    g.total = o + 256;
    return g;
}

}  // namespace

extern "C" size_t po_beam2d_ws_bytes_impl(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, int W,
                                          int model, int method) {
    (void)C;
    if (method == PO_METHOD_GRID) return po_b2_grid_ws_bytes(n, mr1, mr2, W, model, true);
    if (method == PO_METHOD_GRID_NOENV) return po_b2_grid_ws_bytes(n, mr1, mr2, W, model, false);
    if (reg_eligible(n, W, (model == PO_MODEL_FLIPFLOP) ? C / 2 : C - 1, model, method)) return reg_geometry(n, tr1, tr2, mr1, mr2, W, model).total;
    return po_b2_legacy_ws_bytes(n, mr1, mr2, W, model, method, 0) + po_b2_legacy_ws_bytes(n, mr1, mr2, W, model, method, REG_FB_BLOCKS);
}

extern "C" void po_b2_set_mark(void (*f)(int, hipStream_t)) { g_b2_mark = f; }
extern "C" int po_set_pair_route(int route, int defer_odd) {
    if (route != PO_ROUTE_AUTO && route != PO_ROUTE_LEGACY && route != PO_ROUTE_REG) return PO_E_ARG;   // (PO_ROUTE_X2 / PO_ROUTE_RING: kernels retired in round 5)
    b2_route().route = route;
    b2_route().defer_odd = defer_odd & 7;   // bit 0: odd pairs are handed on; bits 1, 2: starve the row groups / the arena
    return PO_OK;
}
// The slice pool ahead of time / given back (include/poreover_hip.h).
extern "C" int po_reg_pool_prewarm(int model, int beam_width) {
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE && model != PO_MODEL_FLIPFLOP) return PO_E_ARG;
    if (beam_width < 1 || beam_width > 12) return PO_E_ARG;
    return reg_pool(model, reg_wide(beam_width)) ? PO_OK : PO_E_NOMEM;
}
extern "C" int po_reg_pool_release(void) {
    if (hipDeviceSynchronize() != hipSuccess) return PO_E_HIP;   // (no pair wave may still hold a slice)
    const int dev = po_cur_device();
    std::lock_guard<std::mutex> lk(g_reg_pool_mu);
    for (int k = 0; k < 6; ++k) {
        g_reg_pool_failed[dev][k] = false;
        RegPool* p = g_reg_pools[dev][k];
        if (!p) continue;
        for (auto c : p->chunk) if (c) (void)hipFree(c);
        if (p->words) (void)hipFree(p->words);
        delete p;
        g_reg_pools[dev][k] = nullptr;
    }
    return PO_OK;
}
// How beam2d_reg_kernel computes a NEW element's window (po_beam2d_reg.hip, "closed form"): see include/poreover_hip.h.
extern "C" int po_set_chain_mode(int mode) {
    if (mode != PO_CHAIN_SERIAL && mode != PO_CHAIN_CLOSED_FORM && mode != PO_CHAIN_CLOSED_GUARD3) return PO_E_ARG;
    b2_route().chain_scan = mode;
    return PO_OK;
}
extern "C" int po_get_chain_mode(void) { return b2_route().chain_scan; }
// Whether a launch of the default shape takes beam2d_reg_kernel's fixed-shape instantiation: see include/poreover_hip.h.
extern "C" int po_set_reg_fixed_shape(int on) {
    b2_route().reg_fixed = on ? 1 : 0;
    return PO_OK;
}
extern "C" int po_get_reg_fixed_shape(void) { return b2_route().reg_fixed; }
// profiling: a device counter that the pair beam kernels add their number of update_prob evaluations to
extern "C" void po_b2_set_update_counter(unsigned long long* dev_counter) { g_b2_upd_counter = dev_counter; }
// tests: pairs the register-state kernel (or its pre-pass) handed to beam2d_kernel on this device since the last reset, summed
// over the pools in use (synchronises the device)
extern "C" long long po_debug_deferred_pairs(int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    const int dev = po_cur_device();
    long long tot = 0;
    std::lock_guard<std::mutex> lk(g_reg_pool_mu);
    for (RegPool* p : g_reg_pools[dev]) {
        if (!p) continue;
        unsigned long long v = 0;
        if (hipMemcpy(&v, p->defer_count, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        tot += (long long)v;
        if (reset && hipMemset(p->defer_count, 0, sizeof(v)) != hipSuccess) return -1;
    }
    return tot;
}

extern "C" int po_launch_beam2d_geom(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                                     const int32_t* env, int n, int C, int A, uint32_t alphabet, int W, int model,
                                     int method, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, char* seq,
                                     const int64_t* seq_off, int32_t* seq_len, int32_t* status, int use_pre_status,
                                     void* ws, size_t ws_bytes, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    if (A < 1 || A > PO_A || W < 1 || W > 25) return PO_E_ARG;
    if (method != PO_METHOD_ROW_COL && method != PO_METHOD_ROW && method != PO_METHOD_GRID) return PO_E_ARG;
    if ((model == PO_MODEL_FLIPFLOP) ? (C != 2 * A) : (C != A + 1)) return PO_E_ARG;
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE && model != PO_MODEL_FLIPFLOP) return PO_E_ARG;
    PoB2Call c;
    c.y1 = y1; c.y1_off = y1_off; c.y2 = y2; c.y2_off = y2_off; c.env = env;
    c.n = n; c.C = C; c.A = A; c.alphabet = alphabet; c.W = W; c.model = model; c.method = method;
    c.mr1 = mr1; c.mr2 = mr2;
    c.seq = seq; c.seq_off = seq_off; c.seq_len = seq_len; c.status = status; c.use_pre_status = use_pre_status;
    c.stream = stream;
    c.order = b2_route().no_order ? nullptr : pair_order;
    c.upd_count = g_b2_upd_counter;
    c.mark = g_b2_mark;
    // without an envelope the reference's dispatcher knows "row" and sends everything else to grid (BeamSearch.h:441-458)
    if (method == PO_METHOD_GRID || (!env && method != PO_METHOD_ROW)) return po_b2_launch_grid(c, ws, ws_bytes);
    if (reg_eligible(n, W, A, model, method)) {
        const RegGeom g = reg_geometry(n, tr1, tr2, mr1, mr2, W, model);
        if (ws_bytes < g.total) return PO_E_CAP;
        RegPool* const rp = reg_pool(model, reg_wide(W));   // (made by the size query before this launch: reg_eligible)
        if (!rp) return PO_E_NOMEM;                          // (cannot happen: eligibility said it exists)
        char* w = (char*)ws;
        RegArgs a = {};
        b2_caller_args(a, c);
        a.queue = (int*)(w + g.off_queue);
        a.meta = (int2*)(w + g.off_meta);
        a.nmain = (int*)(w + g.off_nmain);
        a.sched = (int4*)(w + g.off_sched);
        a.envt = (int*)(w + g.off_envt);
        a.pool_bytes = rp->pool_bytes; a.arena_cap = rp->arena_cap;
        for (int k = 0; k < 8; ++k) a.slice_chunk[k] = rp->chunk[k];
        a.slice_spc_log2 = rp->spc_log2; a.nslices = rp->nslices; a.slice_bytes = rp->slice_bytes; a.slice_claim = rp->claim;
        a.slice_tickets = rp->tickets;
        a.defer_count = rp->defer_count;
        a.persist = b2_route().persist >= 0 ? (b2_route().persist != 0) : 1;   // (PO_REG_PERSIST)
        a.starve = (b2_route().defer_odd >> 1) & 3;
        a.defer_odd = b2_route().defer_odd & 1;
        a.chain_scan = b2_route().chain_scan;
        a.fixed_shape = b2_route().reg_fixed;
        if (n > g.blocks && !b2_route().no_order) {   // more pairs than resident workgroups: longest first
            a.order = (int*)(w + g.off_order);
            pair_order(y1_off, y2_off, n, (int*)(w + g.off_order), stream);
        }
        const int grid = a.persist ? std::min(g.blocks, rp->nslices) : n;
        a.ngl = po_reg_ngl(reg_wide(W));
        if (po_zero_async(w + g.off_queue, 256, stream) != hipSuccess) return PO_E_HIP;
        if (model == PO_MODEL_CTC) hipLaunchKernelGGL(beam2d_prepass_kernel<PO_MODEL_CTC>, dim3(n), dim3(64), 0, stream, a);
        else if (model == PO_MODEL_MERGE) hipLaunchKernelGGL(beam2d_prepass_kernel<PO_MODEL_MERGE>, dim3(n), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL(beam2d_prepass_kernel<PO_MODEL_FLIPFLOP>, dim3(n), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(beam2d_walk_kernel, dim3(n), dim3(64), 0, stream, a);
        if (g_b2_mark) g_b2_mark(1, stream);
        po_reg_launch(&a, grid, model, reg_wide(W), stream);
        if (g_b2_mark) g_b2_mark(0, stream);
        // pairs the pre-pass or the kernel deferred (tier-2 row groups exhausted, windows beyond the store's ring):
        // one small pass of beam2d_kernel, a no-op when there are none
        return po_b2_launch_legacy(c, w + g.off_fb, g.fb_bytes, REG_FB_BLOCKS, a.meta, 0, a.queue + 16);
    }
    return po_b2_launch_legacy(c, ws, ws_bytes, 0, nullptr);
}

// max rows are not part of the device-pointer ABI: read them back from the offset arrays
extern "C" int po_launch_beam2d(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                                const int32_t* env, int n, int C, int A, uint32_t alphabet, int W, int model,
                                int method, char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status,
                                void* ws, size_t ws_bytes, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    int64_t* h = (int64_t*)malloc(sizeof(int64_t) * 2 * (size_t)(n + 1));
    if (!h) return PO_E_NOMEM;
    int rc = PO_OK;
    if (hipMemcpyAsync(h, y1_off, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(h + n + 1, y2_off, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        rc = PO_E_HIP;
    int64_t m1 = 0, m2 = 0, tr1 = 0, tr2 = 0;
    if (rc == PO_OK) {
        for (int i = 0; i < n; ++i) {
            m1 = std::max<int64_t>(m1, h[i + 1] - h[i]);
            m2 = std::max<int64_t>(m2, h[n + 1 + i + 1] - h[n + 1 + i]);
        }
        tr1 = h[n] - h[0];
        tr2 = h[n + 1 + n] - h[n + 1];
    }
    free(h);
    if (rc != PO_OK) return rc;
    return po_launch_beam2d_geom(y1, y1_off, y2, y2_off, env, n, C, A, alphabet, W, model, method, tr1, tr2, m1, m2, seq,
                                 seq_off, seq_len, status, 0, ws, ws_bytes, stream);
}

