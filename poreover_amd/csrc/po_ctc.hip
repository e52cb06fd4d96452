// The CTC loss and its gradient on tensors that lie where a model left them: po_ctc_loss.
//
// Item i: logits x [T][C] (any strides, f32 / f16 / bf16, or f64 log-probabilities), labels l [L].  lp = log_softmax(x) per
// frame in f64 (ctc_lsm_kernel's arithmetic), loss = -log P(l | lp) over the 2L + 1 states with ctc_alpha_beta_kernel's
// transitions (po_train.hip), grad[t][c] = softmax(x[t])[c] - sum_{s: label(s) = c} exp(alpha_t(s) + beta_t(s) - log Z).
//
//   ctc_offsets_kernel   one workgroup: the exclusive scan of T_i * S_i, where item i's alpha rows start in the workspace
//   ctc_loss_kernel      one workgroup per item, three phases:
//     0  the frames' log-softmax, a frame per thread, kept in the workspace (C doubles per frame, canonical column order)
//     1  alpha forward in time through two rows in LDS; every row is also written to the workspace (only with a gradient)
//     2  beta backward through the same two rows; at frame t it is joined with the stored alpha row, the occupancies are
//        reduced per class in a fixed order (a thread's own states in order, a xor tree in the wave, the waves in order
//        through LDS) and the finished gradient row of frame t is written through the gradient's item table
//   A thread owns the states tid, tid + NT, ...: K of them at most, in registers.  No floating-point atomics, nothing is
//   handed from one workgroup to another: an item's bits depend on the item alone.  The lp values and the alpha row of the
//   next step are requested one step ahead.
//
// Items are dealt to launch classes by S = 2L + 1 (po_ctc_rules.h).  The label lengths are on the device and the entry reads
// no device memory, so every class that the call's largest S admits is launched over all n items and a workgroup whose item
// belongs to another class leaves at once.  Enqueue-only: no allocation, no synchronisation.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "po_ctc_rules.h"
#include "po_device.h"
#include "po_hostbuf.h"

namespace {

constexpr int CODE_LABEL = 7, CODE_SELF = 8, CODE_SKIP_IN = 16, CODE_SKIP_OUT = 32;

struct CtcArgs {
    const po_ingest_item* items; const int64_t* row_off; const int32_t* labels; const int64_t* label_off;
    const po_ingest_item* gitems;       // NULL: loss only (phase 2 is skipped, alpha is not stored)
    int n, C, dtype, gdtype, normalize, merge;
    int s_lo, s_hi, max_states;         // this launch's class: s_lo < S <= s_hi; the caller's largest S
    int perm[8];
    int64_t total_rows, total_states;
    float* loss; int32_t* status;
    const int64_t* a_off; double* lp; double* alpha;
};

__device__ __forceinline__ double lse2(double a, double b) {   // po_train.hip's
    const double m = fmax(a, b);
    const double r = m + log1p(exp(-fabs(a - b)));
    return m == -INFINITY ? -INFINITY : r;   // (a select, not a branch: the lanes of a frame step stay together)
}

__device__ __forceinline__ int elem_bytes(int dtype) { return dtype == PO_DTYPE_F64 ? 8 : (dtype == PO_DTYPE_F32 ? 4 : 2); }

__device__ __forceinline__ double load_f64(const char* p, int dtype) {
    if (dtype == PO_DTYPE_F64) return *(const double*)p;
    if (dtype == PO_DTYPE_F32) return (double)*(const float*)p;
    if (dtype == PO_DTYPE_F16) return (double)(float)*(const _Float16*)p;
    return (double)__uint_as_float((uint32_t)*(const uint16_t*)p << 16);
}

// v rounded to float, then to the gradient's type (round to nearest even; bf16 keeps NaN a NaN)
__device__ __forceinline__ void store_grad(const po_ingest_item& it, int gdtype, int64_t t, int col, double v) {
    const float f = (float)v;
    char* p = (char*)it.base + (t * it.row_stride + col * it.col_stride) * elem_bytes(gdtype);
    if (gdtype == PO_DTYPE_F32) *(float*)p = f;
    else if (gdtype == PO_DTYPE_F16) *(_Float16*)p = (_Float16)f;
    else {
        const uint32_t u = __float_as_uint(f);
        *(uint16_t*)p = (f != f) ? (uint16_t)((u >> 16) | 0x40) : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

// does item i count, and with what sizes: the rule of both kernels.  0 = it runs; otherwise the status it gets
__device__ __forceinline__ int item_shape(const CtcArgs& a, int i, int64_t* r0, int64_t* T, int64_t* l0, int64_t* L) {
    *r0 = a.row_off[i]; *T = a.row_off[i + 1] - *r0;
    *l0 = a.label_off[i]; *L = a.label_off[i + 1] - *l0;
    if (*r0 < 0 || *T < 0 || *l0 < 0 || *L < 0 || *T > 0x7fffffff || *r0 + *T > a.total_rows) return PO_E_ARG;
    if (*L > PO_CTC_MAX_LABEL) return PO_E_UNSUPPORTED;
    if (2 * *L + 1 > a.max_states) return PO_E_CAP;
    return 0;
}

constexpr int SCAN_THREADS = 256;
// a_off[i] = sum_{j < i} T_j * S_j over the items that run (int64), one workgroup
__global__ __launch_bounds__(SCAN_THREADS) void ctc_offsets_kernel(CtcArgs a, int64_t* a_off) {
    __shared__ int64_t sh[SCAN_THREADS];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int b = 0; b < a.n; b += SCAN_THREADS) {
        const int i = b + tid;
        int64_t v = 0;
        if (i < a.n) {
            int64_t r0, T, l0, L;
            if (item_shape(a, i, &r0, &T, &l0, &L) == 0) v = T * (2 * L + 1);
        }
        sh[tid] = v;
        __syncthreads();
        for (int d = 1; d < SCAN_THREADS; d <<= 1) {
            const int64_t add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (i < a.n) a_off[i] = carry + sh[tid] - v;
        carry += sh[SCAN_THREADS - 1];
        __syncthreads();
    }
}

__device__ __forceinline__ double wave_sum(double v) {   // a fixed tree: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ void zero_grad_rows(const CtcArgs& a, int i, int64_t T, int C, int tid, int nt) {
    if (!a.gitems) return;
    const po_ingest_item g = a.gitems[i];
    for (int64_t e = tid; e < T * C; e += nt) {
        const int64_t t = e / C;
        store_grad(g, a.gdtype, t, (int)(e - t * C), 0.0);
    }
}

// NT threads, K states per thread at most, CT = C at compile time (0: a.C)
template <int NT, int K, int CT>
__global__ __launch_bounds__(NT) void ctc_loss_kernel(CtcArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ctc_lds[];
    __shared__ int s_bad, s_rep;
    constexpr int NW = NT / 64;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int C = CT ? CT : a.C;
    int64_t r0, T64, l0, L64;
    const int why = item_shape(a, i, &r0, &T64, &l0, &L64);
    if (why != 0) {   // (class 0 is launched in every call: it answers for the items that no class runs)
        if (a.s_lo != 0) return;
        if (why != PO_E_ARG) zero_grad_rows(a, i, T64, C, tid, NT);
        if (tid == 0) { a.loss[i] = NAN; if (a.status) a.status[i] = why; }
        return;
    }
    const int L = (int)L64, S = 2 * L + 1, T = (int)T64;
    if (S <= a.s_lo || S > a.s_hi) return;
    const bool grad = a.gitems != nullptr;
    const int64_t ao = grad ? a.a_off[i] : 0;
    if (grad && (ao < 0 || ao + T64 * S > a.total_states)) {
        zero_grad_rows(a, i, T64, C, tid, NT);
        if (tid == 0) { a.loss[i] = NAN; if (a.status) a.status[i] = PO_E_CAP; }
        return;
    }

    const int SP = po_ctc_row_stride(S);
    double* rows = ctc_lds;                              // [2][SP], state s at [s + 2]
    double* red = ctc_lds + 2 * SP;                      // [2][4][8]
    unsigned char* code = (unsigned char*)(red + 64);    // [S]
    if (tid == 0) { s_bad = 0; s_rep = 0; }
    __syncthreads();
    {   // the state codes; the labels are checked on the way
        const int32_t* lab = a.labels + l0;
        int bad = 0, rep = 0;
        for (int l = tid; l < L; l += NT) {
            const int v = lab[l];
            const int prev = l > 0 ? lab[l - 1] : -1, next = l + 1 < L ? lab[l + 1] : -1;
            bad |= (v < 0 || v > C - 2);
            rep += (l > 0 && v == prev);
            int cd = (v & CODE_LABEL) | (a.merge ? CODE_SELF : 0);
            if (l > 0 && (!a.merge || v != prev)) cd |= CODE_SKIP_IN;
            if (l + 1 < L && (!a.merge || v != next)) cd |= CODE_SKIP_OUT;
            code[2 * l + 1] = (unsigned char)cd;
        }
        for (int l = tid; l <= L; l += NT) code[2 * l] = (unsigned char)((C - 1) | CODE_SELF);
        if (bad) atomicOr(&s_bad, 1);
        if (rep) atomicAdd(&s_rep, rep);
        for (int k = tid; k < 4; k += NT) {   // the rows' -inf borders
            const int at = k < 2 ? k : S + k;
            rows[at] = -INFINITY; rows[SP + at] = -INFINITY;
        }
    }
    __syncthreads();
    if (s_bad) {
        zero_grad_rows(a, i, T64, C, tid, NT);
        if (tid == 0) { a.loss[i] = NAN; if (a.status) a.status[i] = PO_E_ARG; }
        return;
    }
    if (po_ctc_min_frames(L, s_rep, a.merge) > T64) {   // no path: +inf, a gradient of zeros
        zero_grad_rows(a, i, T64, C, tid, NT);
        if (tid == 0) { a.loss[i] = INFINITY; if (a.status) a.status[i] = PO_E_ENVELOPE; }
        return;
    }
    if (T == 0) {   // (then L = 0: the empty path)
        if (tid == 0) { a.loss[i] = 0.f; if (a.status) a.status[i] = 0; }
        return;
    }

    // ---- phase 0: lp[t][c] = log softmax of frame t, column perm[c] of the source
    double* lp = a.lp + r0 * C;
    {
        const po_ingest_item it = a.items[i];
        const int eb = elem_bytes(a.dtype);
        for (int t = tid; t < T; t += NT) {
            const char* p = (const char*)it.base + (int64_t)t * it.row_stride * eb;
            double x[8], mx = -INFINITY, sum = 0.0;
#pragma unroll
            for (int c = 0; c < 8; ++c) if (c < C) { x[c] = load_f64(p + a.perm[c] * it.col_stride * eb, a.dtype); mx = fmax(mx, x[c]); }
            double lz = 0.0;
            if (a.normalize) {
#pragma unroll
                for (int c = 0; c < 8; ++c) if (c < C) sum += exp(x[c] - mx);
                lz = mx + log(sum);
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) if (c < C) lp[(int64_t)t * C + c] = a.normalize ? x[c] - lz : x[c];
        }
    }
    // (a thread's state past the last one stands in for S - 1 wherever an address is made of it: the loads of the frame
    // loops are unconditional — a branch around a load costs a full wait for it — and their results unused)
    int cd[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cd[k] = code[min(tid + k * NT, S - 1)];
    __syncthreads();

    // ---- phase 1: alpha.  A state's transitions as operands chosen by its flags, the same instructions in every lane: lse2
    // is symmetric in its operands and lse2(v, -inf) is v, bit for bit, so an absent transition enters as -inf.  Without
    // merged repeats a state has two transitions at most (blank: stay, step; label: step, skip) — one lse2.
    double* A = a.alpha + ao;
    const int wave0 = tid & ~63;
    double nx[K] = {};   // lp of the next step at this thread's states
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = tid + k * NT;
        if (s < S) {
            const double v = s < 2 ? lp[cd[k] & CODE_LABEL] : -INFINITY;
            rows[s + 2] = v;
            if (grad) A[s] = v;
        }
        nx[k] = lp[(T > 1 ? C : 0) + (cd[k] & CODE_LABEL)];
    }
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        const double* prev = rows + ((t - 1) & 1) * SP;
        double* cur = rows + (t & 1) * SP;
        double now[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            now[k] = nx[k];
            nx[k] = lp[(int64_t)min(t + 1, T - 1) * C + (cd[k] & CODE_LABEL)];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (wave0 + k * NT < S) {   // (the same in every lane of a wave: a wave without states skips the step)
                const int s = tid + k * NT, sc = min(s, S - 1);
                const double p0 = prev[sc + 2], p1 = prev[sc + 1], p2 = prev[sc];
                const double skip = (cd[k] & CODE_SKIP_IN) ? p2 : -INFINITY;
                double v = lse2(p1, (cd[k] & CODE_SELF) ? p0 : skip);
                if (a.merge) v = lse2(v, skip);
                v += now[k];
                if (s < S) {
                    cur[s + 2] = v;
                    if (grad) A[(int64_t)t * S + s] = v;
                }
            }
        }
        __syncthreads();
    }
    const double* last = rows + ((T - 1) & 1) * SP;
    const double lz = S >= 2 ? lse2(last[S + 1], last[S]) : last[2];
    if (tid == 0) { a.loss[i] = (float)(-lz); if (a.status) a.status[i] = 0; }
    if (!grad) return;
    __syncthreads();   // (the last alpha row is read above; the rows are written below)

    // ---- phase 2: beta, joined with alpha.  The rows hold bt_t(s) = beta_t(s) + lp_t[label(s)]; beta_t(s) is the lse of
    // bt_{t+1} over the transitions out of s.  The row of frame T is made up: 0 in the last state and -inf elsewhere gives
    // beta_{T-1} = 0 in the last two states and -inf in the others, by the same instructions as every other frame.
    const po_ingest_item g = a.gitems[i];
    {
        double* end = rows + (T & 1) * SP;
        for (int s = tid; s < S; s += NT) end[s + 2] = s == S - 1 ? 0.0 : -INFINITY;
    }
    double al[K] = {};   // alpha and lp of the step to come, at this thread's states
#pragma unroll
    for (int k = 0; k < K; ++k) {
        al[k] = A[(int64_t)(T - 1) * S + min(tid + k * NT, S - 1)];
        nx[k] = lp[(int64_t)(T - 1) * C + (cd[k] & CODE_LABEL)];
    }
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        const double* nxt = rows + ((t + 1) & 1) * SP;
        double* cur = rows + (t & 1) * SP;
        double now[K], anow[K];
        const double mine = lp[(int64_t)t * C + min(tid, C - 1)];   // the gradient's softmax term, used after the barrier
#pragma unroll
        for (int k = 0; k < K; ++k) {
            now[k] = nx[k]; anow[k] = al[k];
            al[k] = A[(int64_t)max(t - 1, 0) * S + min(tid + k * NT, S - 1)];
            nx[k] = lp[(int64_t)max(t - 1, 0) * C + (cd[k] & CODE_LABEL)];
        }
        double occ[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) occ[c] = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (wave0 + k * NT < S) {   // (the same in every lane of a wave: a wave without states skips the step)
                const int s = tid + k * NT, sc = min(s, S - 1);
                const double p0 = nxt[sc + 2], p1 = nxt[sc + 3], p2 = nxt[sc + 4];
                const double skip = (cd[k] & CODE_SKIP_OUT) ? p2 : -INFINITY;
                double b = lse2(p1, (cd[k] & CODE_SELF) ? p0 : skip);
                if (a.merge) b = lse2(b, skip);
                const double e = s < S ? exp(anow[k] + b - lz) : 0.0;
                const int lbl = cd[k] & CODE_LABEL;
#pragma unroll
                for (int c = 0; c < 8; ++c) if (c < C) occ[c] += (lbl == c) ? e : 0.0;
                if (s < S) cur[s + 2] = b + now[k];
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < C) occ[c] = wave_sum(occ[c]);
        if (NW == 1) {
            if (tid < C) {
                double o = 0.0;
#pragma unroll
                for (int c = 0; c < 8; ++c) o = (tid == c) ? occ[c] : o;
                store_grad(g, a.gdtype, t, a.perm[tid], a.normalize ? exp(mine) - o : -o);
            }
            __syncthreads();
        } else {
            double* slot = red + (t & 1) * 32;
            if ((tid & 63) == 0) {
#pragma unroll
                for (int c = 0; c < 8; ++c) if (c < C) slot[(tid >> 6) * 8 + c] = occ[c];
            }
            __syncthreads();
            if (tid < C) {
                double o = 0.0;
                for (int w = 0; w < NW; ++w) o += slot[w * 8 + tid];
                store_grad(g, a.gdtype, t, a.perm[tid], a.normalize ? exp(mine) - o : -o);
            }
        }
    }
}

template <int CT>
void launch_class(int cls, const CtcArgs& a, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)a.n);
    if (cls == 0) hipLaunchKernelGGL((ctc_loss_kernel<64, 2, CT>), grid, dim3(64), lds, s, a);
    else if (cls == 1) hipLaunchKernelGGL((ctc_loss_kernel<256, 2, CT>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((ctc_loss_kernel<256, 10, CT>), grid, dim3(256), lds, s, a);
}

struct CtcPlan { size_t b_off, b_lp, b_alpha; size_t total() const { return b_off + b_lp + b_alpha; } };
CtcPlan ctc_plan(int n, int64_t total_rows, int64_t total_states, int C, int with_grad) {
    CtcPlan p{0, 0, 0};
    if (n <= 0) return p;
    p.b_off = al256(sizeof(int64_t) * (size_t)n);
    p.b_lp = al256(sizeof(double) * (size_t)std::max<int64_t>(total_rows, 0) * (size_t)std::max(C, 0));
    p.b_alpha = with_grad ? al256(sizeof(double) * (size_t)std::max<int64_t>(total_states, 0)) : 0;
    return p;
}

// the refusals that need sizes only (po_ctc_loss, its twin)
int ctc_check(const std::string& w, int n, int C, int dtype, int normalize, const int* perm_h, int model, int64_t total_rows,
              int64_t total_states, int max_states, bool with_grad, int grad_dtype) {
    if (model == PO_MODEL_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, w + ": the flip-flop model has no CTC loss here");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, w + ": unknown model");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (total_rows < 0 || total_states < 0 || max_states < 0) return po_fail(PO_E_ARG, w + ": negative total_rows, total_states or max_states");
    if (C < 2 || C > 8) return po_fail(PO_E_ARG, w + ": C must be 2..8");
    if (dtype < PO_DTYPE_F32 || dtype > PO_DTYPE_F64) return po_fail(PO_E_ARG, w + ": unknown dtype");
    if (with_grad && (grad_dtype < PO_DTYPE_F32 || grad_dtype > PO_DTYPE_BF16)) return po_fail(PO_E_ARG, w + ": the gradient's dtype must be f32, f16 or bf16");
    if (perm_h) {
        unsigned seen = 0;
        for (int c = 0; c < C; ++c) {
            if (perm_h[c] < 0 || perm_h[c] >= C) return po_fail(PO_E_ARG, w + ": perm entry outside [0, C)");
            seen |= 1u << perm_h[c];
        }
        if (seen != (1u << C) - 1) return po_fail(PO_E_ARG, w + ": perm must name every column once (the gradient is written through it)");
    }
    if (normalize && dtype == PO_DTYPE_F64) return po_fail(PO_E_UNSUPPORTED, w + ": normalize with float64 input (the reference normalises in the array's own precision)");
    if (max_states > PO_CTC_MAX_STATES)
        return po_fail(PO_E_UNSUPPORTED, w + ": a label of more than " + std::to_string(PO_CTC_MAX_LABEL) + " symbols (" +
                       std::to_string((max_states - 1) / 2) + " here): the lattice rows are kept in LDS");
    return PO_OK;
}
}  // namespace

extern "C" {

size_t po_ctc_loss_workspace_bytes(int n, int64_t total_rows, int64_t total_states, int C, int with_grad) {
    po_fail(PO_OK, "");
    return ctc_plan(n, total_rows, total_states, C, with_grad).total();
}

int po_ctc_loss(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, int normalize, const int* perm_h,
                const int32_t* labels, const int64_t* label_off, int model, int64_t total_rows, int64_t total_states,
                int max_states, float* loss, int32_t* status, const po_ingest_item* grad_items, int grad_dtype, void* ws,
                size_t ws_bytes, void* stream) {
    po_fail(PO_OK, "");
    const std::string w("po_ctc_loss");
    const bool with_grad = grad_items != nullptr;
    int rc = ctc_check(w, n, C, dtype, normalize, perm_h, model, total_rows, total_states, max_states, with_grad, grad_dtype);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;
    if (!items || !row_off || !labels || !label_off || !loss) return po_fail(PO_E_ARG, w + ": null items, row_off, labels, label_off or loss");
    const CtcPlan p = ctc_plan(n, total_rows, total_states, C, with_grad);
    if (!ws || ws_bytes < p.total()) return po_fail(PO_E_ARG, w + ": workspace smaller than po_ctc_loss_workspace_bytes");
    CtcArgs a = {};
    a.items = items; a.row_off = row_off; a.labels = labels; a.label_off = label_off; a.gitems = grad_items;
    a.n = n; a.C = C; a.dtype = dtype; a.gdtype = grad_dtype; a.normalize = normalize ? 1 : 0; a.merge = model == PO_MODEL_MERGE;
    a.max_states = std::max(max_states, 1);
    for (int c = 0; c < 8; ++c) a.perm[c] = (perm_h && c < C) ? perm_h[c] : (c < C ? c : 0);
    a.total_rows = total_rows; a.total_states = total_states;
    a.loss = loss; a.status = status;
    a.a_off = (const int64_t*)ws;
    a.lp = (double*)((char*)ws + p.b_off);
    a.alpha = (double*)((char*)ws + p.b_off + p.b_lp);
    hipStream_t s = (hipStream_t)stream;
    if (with_grad) hipLaunchKernelGGL(ctc_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a, (int64_t*)ws);
    for (int c = 0; c < PO_CTC_NCLASS; ++c) {
        a.s_lo = c ? PO_CTC_CLASS_HI[c - 1] : 0;
        if (c > 0 && a.max_states <= a.s_lo) break;
        a.s_hi = PO_CTC_CLASS_HI[c];
        const size_t lds = po_ctc_lds_bytes(std::min(a.s_hi, a.max_states));
        if (C == 5) launch_class<5>(c, a, lds, s); else launch_class<0>(c, a, lds, s);
    }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

int po_ctc_loss_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                  const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, int normalize,
                  const int* perm_h, const int32_t* labels_h, const int64_t* label_off_h, int model, float* loss_h,
                  int32_t* status_h, void* grad_h, int grad_dtype) {
    po_fail(PO_OK, "");
    const std::string w("po_ctc_loss_h");
    if (n > 0 && (!row_off_h || !label_off_h)) return po_fail(PO_E_ARG, w + ": null row_off or label_off");
    int64_t rows = 0, states = 0, max_states = 1;
    for (int i = 0; i < std::max(n, 0); ++i) {
        const int64_t T = row_off_h[i + 1] - row_off_h[i], L = label_off_h[i + 1] - label_off_h[i];
        if (T < 0 || L < 0 || T > 0x7fffffff || L > (1 << 29)) return po_fail(PO_E_ARG, w + ": offsets must not decrease (an item has fewer than 2^31 frames)");
        rows += T;
        states += T * (2 * L + 1);
        max_states = std::max(max_states, 2 * L + 1);
    }
    int rc = ctc_check(w, n, C, dtype, normalize, perm_h, model, rows, states, (int)max_states, grad_h != nullptr, grad_dtype);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;
    if (!loss_h || !item_off_h || !row_stride_h || !col_stride_h || (rows > 0 && !src_h) || (label_off_h[n] > label_off_h[0] && !labels_h))
        return po_fail(PO_E_ARG, w + ": null src, item table, labels or loss");
    if (row_off_h[0] != 0) return po_fail(PO_E_ARG, w + ": row_off[0] must be 0");
    const size_t eb = dtype == PO_DTYPE_F64 ? 8 : (dtype == PO_DTYPE_F32 ? 4 : 2);
    for (int i = 0; i < n; ++i) {
        const int64_t T = row_off_h[i + 1] - row_off_h[i];
        if (item_off_h[i] < 0 || row_stride_h[i] < 0 || col_stride_h[i] < 0) return po_fail(PO_E_ARG, w + ": negative offset or stride");
        if (T > 0 && (src_elems <= 0 || (T > 1 && row_stride_h[i] > (src_elems - 1) / (T - 1)) || col_stride_h[i] > (src_elems - 1) / (C - 1) ||
                      item_off_h[i] + (T - 1) * row_stride_h[i] + (C - 1) * col_stride_h[i] >= src_elems))
            return po_fail(PO_E_ARG, w + ": item " + std::to_string(i) + " reaches past src_elems");
    }
    const PoRagged lr(label_off_h, n);
    const size_t geb = grad_dtype == PO_DTYPE_F32 ? 4 : 2;
    std::vector<po_ingest_item> items(n), gitems(n);
    PoDev src, it, git, ro, lab, lo, ls, st, gr, ws;
    PO_HIPCHK(src.up(src_h, (size_t)std::max<int64_t>(src_elems, 0) * eb));
    if (grad_h) PO_HIPCHK(gr.up(nullptr, (size_t)rows * C * geb));
    for (int i = 0; i < n; ++i) {
        items[i] = {src.as<char>() + (size_t)item_off_h[i] * eb, row_stride_h[i], col_stride_h[i]};
        gitems[i] = {gr.as<char>() + (size_t)row_off_h[i] * C * geb, C, 1};   // grad_h: dense rows, the source's column order
    }
    PO_HIPCHK(it.up(items.data(), sizeof(po_ingest_item) * n));
    if (grad_h) PO_HIPCHK(git.up(gitems.data(), sizeof(po_ingest_item) * n));
    PO_HIPCHK(ro.up(row_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(lab.up(labels_h ? labels_h + lr.base : nullptr, sizeof(int32_t) * (size_t)lr.total));
    PO_HIPCHK(lo.up(lr.off.data(), lr.bytes()));
    PO_HIPCHK(ls.up(nullptr, sizeof(float) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_ctc_loss_workspace_bytes(n, rows, states, C, grad_h != nullptr);
    PO_HIPCHK(ws.up(nullptr, wsb));
    rc = po_ctc_loss(it.as<po_ingest_item>(), ro, n, C, dtype, normalize, perm_h, lab, lo, model, rows, states, (int)max_states, ls,
                     st, grad_h ? git.as<po_ingest_item>() : nullptr, grad_dtype, ws, std::max<size_t>(wsb, 256), nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ls.down(loss_h, sizeof(float) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    if (grad_h) PO_HIPCHK(gr.down(grad_h, (size_t)rows * C * geb));
    return PO_OK;
}

}  // extern "C"
