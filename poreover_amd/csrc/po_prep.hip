// Signal preparation on the device: raw int16 reads in, the filtered and scaled f32 signals out, by the
// rule of po_prep_rules.h.  A read is cut into slabs of PO_PREP_SLAB samples from its own first sample on, one workgroup
// per slab, so a long read is many workgroups' work; a read's statistics come from its histogram, which is integers only.
//
//   prep_count_kernel    per slab: the kept samples' histogram in LDS (integer atomics), added to the read's histogram in
//                        global memory (integer atomics: the sums do not depend on their order), and the slab's kept count
//   prep_stats_kernel    per read: n, S, Q, min, max and the middle order statistics from the histogram, the scaling's a
//                        and b (po_prep_finish), and the exclusive scan of the read's slab counts
//   prep_offsets_kernel  one workgroup: the exclusive scan of the reads' kept counts, sig_off
//   prep_write_kernel    per slab: f32((f64(x) - a) / b) of every kept sample at sig_off[read] + the slab's base + the
//                        sample's rank among the slab's kept ones (a workgroup scan): one writer per value, no appending
//
// The int16 input is read in aligned pieces of 16 bytes (PO_PREP_VEC samples), consecutive lanes on consecutive pieces: a
// slab that starts anywhere (a read at an odd element offset) covers the pieces [s0 / 8, ceil(s1 / 8)), 513 at most, and
// masks what lies outside [s0, s1).  The last piece of the buffer is read sample by sample where it is not whole.
#include <algorithm>
#include <string>

#include "po_hostbuf.h"
#include "po_prep_rules.h"

namespace {

constexpr int TPB = PO_PREP_TPB;
constexpr int PASSES = (PO_PREP_SLAB / PO_PREP_VEC + 1 + TPB - 1) / TPB;   // pieces of a slab per lane: 3
constexpr int BINS_PER_LANE = PO_PREP_MAX_BINS / TPB;                      // prep_stats_kernel: 16 consecutive bins
static_assert(PO_PREP_MAX_BINS % TPB == 0, "the histogram is whole lanes' shares");

struct PrepArgs {
    const int16_t* raw;          // 16-byte aligned
    const int64_t* raw_off;      // [n_reads + 1] from 0
    const int64_t* slab_off;     // [n_reads + 1] first slab of each read
    const int32_t* slab_read;    // [slabs]
    int64_t total;               // raw samples in all
    int lo, hi, bins;
};

// workgroup-wide exclusive scan of one value per thread; returns the exclusive prefix, *total the sum
template <class T>
__device__ T block_excl_scan(T v, T* sh, T* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < TPB; o <<= 1) {
        const T u = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
    }
    const T incl = sh[t];
    *total = sh[TPB - 1];
    __syncthreads();
    return incl - v;
}

// the slab's read and its samples [s0, s1) as elements of raw
__device__ __forceinline__ int slab_range(const PrepArgs& a, int64_t slab, int64_t* s0, int64_t* s1) {
    const int r = a.slab_read[slab];
    *s0 = a.raw_off[r] + (slab - a.slab_off[r]) * PO_PREP_SLAB;
    *s1 = min(*s0 + (int64_t)PO_PREP_SLAB, a.raw_off[r + 1]);
    return r;
}

// piece c of raw (elements [8c, 8c + 8)): its samples, and the mask of those that lie in [s0, s1) and are kept
__device__ __forceinline__ unsigned load_piece(const PrepArgs& a, int64_t c, int64_t c1, int64_t s0, int64_t s1, int x[PO_PREP_VEC]) {
#pragma unroll
    for (int j = 0; j < PO_PREP_VEC; ++j) x[j] = 0;
    if (c >= c1) return 0u;
    const int64_t e0 = c * PO_PREP_VEC;
    if (e0 + PO_PREP_VEC <= a.total) {
        const int4 v = *reinterpret_cast<const int4*>(a.raw + e0);
        x[0] = (int16_t)(v.x & 0xffff); x[1] = v.x >> 16;
        x[2] = (int16_t)(v.y & 0xffff); x[3] = v.y >> 16;
        x[4] = (int16_t)(v.z & 0xffff); x[5] = v.z >> 16;
        x[6] = (int16_t)(v.w & 0xffff); x[7] = v.w >> 16;
    } else {
#pragma unroll
        for (int j = 0; j < PO_PREP_VEC; ++j)
            if (e0 + j < a.total) x[j] = a.raw[e0 + j];
    }
    unsigned mask = 0u;
#pragma unroll
    for (int j = 0; j < PO_PREP_VEC; ++j)
        if (e0 + j >= s0 && e0 + j < s1 && po_prep_keep(x[j], a.lo, a.hi)) mask |= 1u << j;
    return mask;
}

__global__ __launch_bounds__(TPB) void prep_count_kernel(PrepArgs a, uint32_t* __restrict__ hist, int32_t* __restrict__ slab_kept) {
    __shared__ uint32_t h[PO_PREP_MAX_BINS];
    __shared__ uint32_t kept;
    const int t = threadIdx.x;
    int64_t s0, s1;
    const int r = slab_range(a, blockIdx.x, &s0, &s1);
    for (int b = t; b < a.bins; b += TPB) h[b] = 0u;
    if (t == 0) kept = 0u;
    __syncthreads();
    const int64_t c0 = s0 / PO_PREP_VEC, c1 = (s1 + PO_PREP_VEC - 1) / PO_PREP_VEC;
    unsigned cnt = 0u;
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        int x[PO_PREP_VEC];
        const unsigned mask = load_piece(a, c0 + k * TPB + t, c1, s0, s1, x);
#pragma unroll
        for (int j = 0; j < PO_PREP_VEC; ++j)
            if (mask >> j & 1u) atomicAdd(&h[x[j] - a.lo - 1], 1u);
        cnt += __popc(mask);
    }
    if (cnt) atomicAdd(&kept, cnt);
    __syncthreads();
    uint32_t* g = hist + (size_t)r * a.bins;
    for (int b = t; b < a.bins; b += TPB)
        if (h[b]) atomicAdd(&g[b], h[b]);
    if (t == 0) slab_kept[blockIdx.x] = (int32_t)kept;
}

__global__ __launch_bounds__(TPB) void prep_stats_kernel(PrepArgs a, int scaling, const double* __restrict__ offset,
                                                         const double* __restrict__ alpha, const uint32_t* __restrict__ hist,
                                                         const int32_t* __restrict__ slab_kept, int32_t* __restrict__ slab_base,
                                                         po_prep_stats* __restrict__ stats) {
    __shared__ uint32_t h[PO_PREP_MAX_BINS];
    __shared__ uint64_t sh[TPB];
    __shared__ int ymin, ymax, ylo, yhi;
    const int t = threadIdx.x;
    const int r = blockIdx.x;
    const uint32_t* g = hist + (size_t)r * a.bins;
    for (int b = t; b < PO_PREP_MAX_BINS; b += TPB) h[b] = b < a.bins ? g[b] : 0u;
    if (t == 0) { ymin = PO_PREP_MAX_BINS; ymax = -1; ylo = 0; yhi = 0; }
    __syncthreads();
    uint64_t cnt = 0, sy = 0, qy = 0;
    int first = PO_PREP_MAX_BINS, last = -1;
#pragma unroll
    for (int j = 0; j < BINS_PER_LANE; ++j) {
        const int y = t * BINS_PER_LANE + j;
        const uint64_t c = h[y];
        if (c) {
            first = min(first, y);
            last = y;
            cnt += c;
            sy += c * (uint64_t)y;
            qy += c * (uint64_t)(y * y);
        }
    }
    if (last >= 0) { atomicMin(&ymin, first); atomicMax(&ymax, last); }
    PoPrepSums s;
    const uint64_t before = block_excl_scan<uint64_t>(cnt, sh, &s.n);
    block_excl_scan<uint64_t>(sy, sh, &s.sy);
    block_excl_scan<uint64_t>(qy, sh, &s.qy);
    if (s.n) {   // the lanes whose bins hold the order statistics (n - 1) / 2 and n / 2
        const uint64_t klo = (s.n - 1) / 2, khi = s.n / 2;
        uint64_t run = before;
#pragma unroll
        for (int j = 0; j < BINS_PER_LANE; ++j) {
            const int y = t * BINS_PER_LANE + j;
            const uint64_t next = run + h[y];
            if (klo >= run && klo < next) ylo = y;
            if (khi >= run && khi < next) yhi = y;
            run = next;
        }
    }
    __syncthreads();
    if (t == 0) {
        s.ymin = s.n ? ymin : 0;
        s.ymax = s.n ? ymax : 0;
        s.ylo = ylo;
        s.yhi = yhi;
        po_prep_stats st;
        po_prep_finish(s, scaling, a.lo, offset ? offset[r] : 0.0, alpha ? alpha[r] : 1.0, &st);
        stats[r] = st;
    }
    // the kept samples before each slab of the read
    uint64_t carry = 0;
    for (int64_t b = a.slab_off[r]; b < a.slab_off[r + 1]; b += TPB) {
        const int64_t i = b + t;
        const uint64_t v = i < a.slab_off[r + 1] ? (uint64_t)slab_kept[i] : 0;
        uint64_t tot;
        const uint64_t ex = block_excl_scan<uint64_t>(v, sh, &tot);
        if (i < a.slab_off[r + 1]) slab_base[i] = (int32_t)(carry + ex);
        carry += tot;
    }
}

// one workgroup: sig_off[0 .. n] = the exclusive scan of the reads' kept counts
__global__ __launch_bounds__(TPB) void prep_offsets_kernel(const po_prep_stats* __restrict__ stats, int n, int64_t* __restrict__ sig_off) {
    __shared__ int64_t sh[TPB];
    int64_t carry = 0;
    for (int b = 0; b < n; b += TPB) {
        const int i = b + threadIdx.x;
        const int64_t v = i < n ? stats[i].n : 0;
        int64_t tot;
        const int64_t ex = block_excl_scan<int64_t>(v, sh, &tot);
        if (i < n) sig_off[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) sig_off[n] = carry;
}

__global__ __launch_bounds__(TPB) void prep_write_kernel(PrepArgs a, const po_prep_stats* __restrict__ stats,
                                                         const int64_t* __restrict__ sig_off, const int32_t* __restrict__ slab_base,
                                                         float* __restrict__ out) {
    __shared__ int32_t sh[TPB];
    const int t = threadIdx.x;
    int64_t s0, s1;
    const int r = slab_range(a, blockIdx.x, &s0, &s1);
    const double sa = stats[r].a, sb = stats[r].b;
    int64_t base = sig_off[r] + slab_base[blockIdx.x];
    const int64_t c0 = s0 / PO_PREP_VEC, c1 = (s1 + PO_PREP_VEC - 1) / PO_PREP_VEC;
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        if (c0 + k * TPB >= c1) break;   // (the same for every lane)
        int x[PO_PREP_VEC];
        const unsigned mask = load_piece(a, c0 + k * TPB + t, c1, s0, s1, x);
        int32_t tot;
        int64_t pos = base + block_excl_scan<int32_t>(__popc(mask), sh, &tot);
#pragma unroll
        for (int j = 0; j < PO_PREP_VEC; ++j)
            if (mask >> j & 1u) out[pos++] = po_prep_scale(x[j], sa, sb);
        base += tot;
    }
}

}  // namespace

extern "C" size_t po_prep_workspace_bytes(int n_reads, int64_t n_slabs, int bins) {
    return al256((size_t)n_reads * bins * 4) + 2 * al256((size_t)n_slabs * 4);
}

// Enqueues the four kernels on `stream`.  Everything is device memory: raw (16-byte aligned) and raw_off as
// po_signal_prep_h's, slab_off / slab_read a PoPrepPlan's tables, offset / alpha double[n_reads] (PO_SCALE_CURRENT; NULL
// otherwise), signal with room for `total` values, sig_off int64[n_reads + 1], stats po_prep_stats[n_reads] (required: the
// kernels pass a and b through it), ws of po_prep_workspace_bytes.  The arguments are the caller's to have checked
// (po_prep_make_plan).
extern "C" int po_launch_signal_prep(const int16_t* raw, const int64_t* raw_off, int n_reads, int64_t total, const int64_t* slab_off,
                                     const int32_t* slab_read, int64_t n_slabs, int scaling, int lo, int hi, const double* offset,
                                     const double* alpha, float* signal, int64_t* sig_off, po_prep_stats* stats, void* ws,
                                     size_t ws_bytes, hipStream_t stream) {
    const int bins = hi - lo - 1;
    if (n_reads < 1 || bins < 0 || bins > PO_PREP_MAX_BINS || n_slabs < 0 || n_slabs > INT32_MAX)
        return po_fail(PO_E_ARG, "po_launch_signal_prep: n_reads " + std::to_string(n_reads) + ", bins " + std::to_string(bins) +
                       ", slabs " + std::to_string(n_slabs));
    if ((uintptr_t)raw & 15) return po_fail(PO_E_ARG, "po_launch_signal_prep: raw is not 16-byte aligned");
    if (ws_bytes < po_prep_workspace_bytes(n_reads, n_slabs, bins)) return po_fail(PO_E_CAP, "po_launch_signal_prep: workspace too small");
    if (scaling == PO_SCALE_CURRENT && (!offset || !alpha)) return po_fail(PO_E_ARG, "po_launch_signal_prep: null offset / alpha");
    uint32_t* hist = (uint32_t*)ws;
    int32_t* slab_kept = (int32_t*)((char*)ws + al256((size_t)n_reads * bins * 4));
    int32_t* slab_base = (int32_t*)((char*)slab_kept + al256((size_t)n_slabs * 4));
    PrepArgs a;
    a.raw = raw; a.raw_off = raw_off; a.slab_off = slab_off; a.slab_read = slab_read;
    a.total = total; a.lo = lo; a.hi = hi; a.bins = bins;
    if (bins > 0) PO_HIPCHK(hipMemsetAsync(hist, 0, (size_t)n_reads * bins * 4, stream));
    if (n_slabs > 0) {
        hipLaunchKernelGGL(prep_count_kernel, dim3((unsigned)n_slabs), dim3(TPB), 0, stream, a, hist, slab_kept);
        PO_HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(prep_stats_kernel, dim3((unsigned)n_reads), dim3(TPB), 0, stream, a, scaling,
                       scaling == PO_SCALE_CURRENT ? offset : nullptr, scaling == PO_SCALE_CURRENT ? alpha : nullptr, hist, slab_kept,
                       slab_base, stats);
    PO_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(prep_offsets_kernel, dim3(1), dim3(TPB), 0, stream, stats, n_reads, sig_off);
    PO_HIPCHK(hipGetLastError());
    if (n_slabs > 0) {
        hipLaunchKernelGGL(prep_write_kernel, dim3((unsigned)n_slabs), dim3(TPB), 0, stream, a, stats, sig_off, slab_base, signal);
        PO_HIPCHK(hipGetLastError());
    }
    return PO_OK;
}

extern "C" int po_signal_prep_h(const int16_t* raw_h, const int64_t* raw_off_h, int n_reads, int scaling, int lo, int hi,
                                const double* offset_h, const double* alpha_h, float* signal_h, int64_t* sig_off_h,
                                po_prep_stats* stats_h, float* ms_h) {
    const std::string me = "po_signal_prep_h: ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (n_reads < 0) return po_fail(PO_E_ARG, me + "n_reads " + std::to_string(n_reads));
    if (!raw_h || !raw_off_h || !signal_h || !sig_off_h)
        return po_fail(PO_E_ARG, me + "null argument " + (!raw_h ? "raw_h" : !raw_off_h ? "raw_off_h" : !signal_h ? "signal_h" : "sig_off_h"));
    if (scaling == PO_SCALE_CURRENT && (!offset_h || !alpha_h))
        return po_fail(PO_E_ARG, me + "null argument " + (!offset_h ? "offset_h" : "alpha_h") + " (PO_SCALE_CURRENT)");
    PoPrepPlan plan;
    std::string err;
    const int rc0 = po_prep_make_plan(raw_off_h, n_reads, scaling, lo, hi, &plan, &err);
    if (rc0 != PO_OK) return po_fail(rc0, err);
    sig_off_h[0] = 0;
    if (ms_h) *ms_h = 0.f;
    if (n_reads == 0) return PO_OK;

    hipStream_t stream = nullptr;
    const int64_t slabs = (int64_t)plan.slab_read.size();
    const size_t wsb = po_prep_workspace_bytes(n_reads, slabs, plan.bins);
    PoDev raw, raw_off, slab_off, slab_read, off, al, sig, sig_off, stats, ws;
    PO_HIPCHK(raw.up(raw_h, (size_t)plan.total * 2));
    PO_HIPCHK(raw_off.up(raw_off_h, sizeof(int64_t) * ((size_t)n_reads + 1)));
    PO_HIPCHK(slab_off.up(plan.slab_off.data(), sizeof(int64_t) * plan.slab_off.size()));
    PO_HIPCHK(slab_read.up(plan.slab_read.data(), sizeof(int32_t) * plan.slab_read.size()));
    if (scaling == PO_SCALE_CURRENT) {
        PO_HIPCHK(off.up(offset_h, sizeof(double) * n_reads));
        PO_HIPCHK(al.up(alpha_h, sizeof(double) * n_reads));
    }
    PO_HIPCHK(sig.up(nullptr, (size_t)plan.total * 4));
    PO_HIPCHK(sig_off.up(nullptr, sizeof(int64_t) * ((size_t)n_reads + 1)));
    PO_HIPCHK(stats.up(nullptr, sizeof(po_prep_stats) * (size_t)n_reads));
    PO_HIPCHK(ws.up(nullptr, wsb));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
    if (ms_h) {
        PO_HIPCHK(hipEventCreate(&ev[0]));
        PO_HIPCHK(hipEventCreate(&ev[1]));
        PO_HIPCHK(hipEventRecord(ev[0], stream));
    }
    const int rc = po_launch_signal_prep(raw, raw_off, n_reads, plan.total, slab_off, slab_read, slabs, scaling, lo, hi, off, al, sig,
                                         sig_off, stats, ws, wsb, stream);
    if (rc != PO_OK) return rc;
    if (ms_h) PO_HIPCHK(hipEventRecord(ev[1], stream));
    PO_HIPCHK(hipStreamSynchronize(stream));
    if (ms_h) PO_HIPCHK(hipEventElapsedTime(ms_h, ev[0], ev[1]));
    PO_HIPCHK(sig_off.down(sig_off_h, sizeof(int64_t) * ((size_t)n_reads + 1)));
    PO_HIPCHK(sig.down(signal_h, (size_t)sig_off_h[n_reads] * 4));
    if (stats_h) PO_HIPCHK(stats.down(stats_h, sizeof(po_prep_stats) * (size_t)n_reads));
    return PO_OK;
}
