// CTC forced alignment on tensors that lie where a model left them: po_forced_align.
//
// The max-plus twin of po_ctc.hip's loss kernel.  Item i: logits x [T][C] (any strides, f32 / f16 / bf16, or f64
// log-probabilities), labels l [L].  lp = log_softmax(x) per frame in f64 (ctc_loss_kernel's phase 0), then over the 2L + 1
// states of po_ctc_loss's lattice  V_t(s) = max(V_{t-1}(s) if s loops, V_{t-1}(s - 1), V_{t-1}(s - 2) if the blank between may
// be skipped) + lp[t][col(s)],  ties to the larger predecessor (stay, then step, then skip).
//
//   falign_offsets_kernel  one workgroup: the exclusive scan of T_i * ceil(S_i / 64), where item i's bit rows start
//   falign_kernel          one workgroup per item, three phases:
//     0  the frames' log-softmax, a frame per thread, kept in the workspace (C doubles per frame, canonical column order)
//     1  V forward in time through two rows in LDS.  A cell's decision (0 stay, 1 step, 2 skip) is kept as two bit planes per
//        wave and state slot — two ballots per step, 16 bytes for 64 cells, written by one lane.  A thread owns the states
//        tid, tid + NT, ...; wave w's slot k holds the states 64 * (k * NT / 64 + w) ..., so a ballot is the word s / 64.
//     2  the trace-back, one wave.  PO_FALIGN_BLOCK = 64 frames at a time: the path's state falls by 2 a frame at most, so
//        within a block it stays in three words that are known when the block begins; lane j requests those three words of
//        frame t0 + j, all of them at once, and the walk itself reads registers only.  One memory round trip per 64 frames.
//        The states of a block are written together, and the lane that sees the path enter or leave a label state writes
//        that symbol's start or stop.
//
// No floating-point atomics, nothing is handed from one workgroup to another: an item's bits depend on the item alone.  The
// launch classes are po_ctc_rules.h's; every class that the call's largest S admits is launched over all n items and a
// workgroup whose item belongs to another class leaves at once.  Enqueue-only: no allocation, no synchronisation.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "po_device.h"
#include "po_falign_rules.h"
#include "po_hostbuf.h"

namespace {

constexpr int CODE_LABEL = 7, CODE_SELF = 8, CODE_SKIP_IN = 16;   // (po_ctc.hip's state codes)

struct FaArgs {
    const po_ingest_item* items; const int64_t* row_off; const int32_t* labels; const int64_t* label_off;
    int n, C, dtype, normalize, merge;
    int s_lo, s_hi, max_states;         // this launch's class: s_lo < S <= s_hi; the caller's largest S
    int perm[8];
    int64_t total_rows, total_words, states_stride;
    double* score; int32_t* states; int32_t* starts; int32_t* stops; int32_t* status;
    const int64_t* b_off; double* lp; uint64_t* bits;
};

__device__ __forceinline__ int elem_bytes(int dtype) { return dtype == PO_DTYPE_F64 ? 8 : (dtype == PO_DTYPE_F32 ? 4 : 2); }

__device__ __forceinline__ double load_f64(const char* p, int dtype) {
    if (dtype == PO_DTYPE_F64) return *(const double*)p;
    if (dtype == PO_DTYPE_F32) return (double)*(const float*)p;
    if (dtype == PO_DTYPE_F16) return (double)(float)*(const _Float16*)p;
    return (double)__uint_as_float((uint32_t)*(const uint16_t*)p << 16);
}

// does item i count, and with what sizes: the rule of both kernels.  0 = it runs; otherwise the status it gets
__device__ __forceinline__ int item_shape(const FaArgs& a, int i, int64_t* r0, int64_t* T, int64_t* l0, int64_t* L) {
    *r0 = a.row_off[i]; *T = a.row_off[i + 1] - *r0;
    *l0 = a.label_off[i]; *L = a.label_off[i + 1] - *l0;
    if (*r0 < 0 || *T < 0 || *l0 < 0 || *L < 0 || *T > 0x7fffffff || *r0 + *T > a.total_rows) return PO_E_ARG;
    if (*L > PO_CTC_MAX_LABEL) return PO_E_UNSUPPORTED;
    if (2 * *L + 1 > a.max_states) return PO_E_CAP;
    if (a.states && *T > a.states_stride) return PO_E_CAP;
    return 0;
}

__device__ __forceinline__ bool wants_path(const FaArgs& a) { return a.states || a.starts || a.stops; }

constexpr int SCAN_THREADS = 256;
// b_off[i] = sum_{j < i} T_j * ceil(S_j / 64) over the items that run (int64), one workgroup
__global__ __launch_bounds__(SCAN_THREADS) void falign_offsets_kernel(FaArgs a, int64_t* b_off) {
    __shared__ int64_t sh[SCAN_THREADS];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int b = 0; b < a.n; b += SCAN_THREADS) {
        const int i = b + tid;
        int64_t v = 0;
        if (i < a.n) {
            int64_t r0, T, l0, L;
            if (item_shape(a, i, &r0, &T, &l0, &L) == 0) v = T * po_falign_row_words(2 * L + 1);
        }
        sh[tid] = v;
        __syncthreads();
        for (int d = 1; d < SCAN_THREADS; d <<= 1) {
            const int64_t add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (i < a.n) b_off[i] = carry + sh[tid] - v;
        carry += sh[SCAN_THREADS - 1];
        __syncthreads();
    }
}

// an item without a path: its score and status, -1 in its whole row of states and (where its label offsets hold) in its
// starts and stops
__device__ void no_path(const FaArgs& a, int i, double score, int why, int64_t l0, int64_t L, int tid, int nt) {
    if (a.states)
        for (int64_t t = tid; t < a.states_stride; t += nt) a.states[i * a.states_stride + t] = -1;
    for (int64_t k = tid; k < L; k += nt) {
        if (a.starts) a.starts[l0 + k] = -1;
        if (a.stops) a.stops[l0 + k] = -1;
    }
    if (tid == 0) { a.score[i] = score; if (a.status) a.status[i] = why; }
}

// NT threads, K states per thread at most, CT = C at compile time (0: a.C)
template <int NT, int K, int CT>
__global__ __launch_bounds__(NT) void falign_kernel(FaArgs a) {
    extern __shared__ __attribute__((aligned(16))) double fa_lds[];
    __shared__ int s_bad, s_rep;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int C = CT ? CT : a.C;
    int64_t r0, T64, l0, L64;
    const int why = item_shape(a, i, &r0, &T64, &l0, &L64);
    if (why != 0) {   // (class 0 is launched in every call: it answers for the items that no class runs)
        if (a.s_lo != 0) return;
        // the label outputs are reached through l0 and L, and the entry is not told how many labels the caller's buffers hold: a
        // label length it would not run (offsets that decrease, more than PO_CTC_MAX_LABEL symbols) is not written through either
        const bool lab_ok = l0 >= 0 && L64 >= 0 && L64 <= PO_CTC_MAX_LABEL;
        no_path(a, i, NAN, why, l0, lab_ok ? L64 : 0, tid, NT);
        return;
    }
    const int L = (int)L64, S = 2 * L + 1, T = (int)T64;
    if (S <= a.s_lo || S > a.s_hi) return;
    const bool path = wants_path(a);
    const int W = (int)po_falign_row_words(S);
    const int64_t bo = path ? a.b_off[i] : 0;
    if (path && (bo < 0 || bo + T64 * W > a.total_words)) { no_path(a, i, NAN, PO_E_CAP, l0, L64, tid, NT); return; }

    const int SP = po_ctc_row_stride(S);
    double* rows = fa_lds;                                   // [2][SP], state s at [s + 2]
    unsigned char* code = (unsigned char*)(fa_lds + 2 * SP); // [S]
    if (tid == 0) { s_bad = 0; s_rep = 0; }
    __syncthreads();
    {   // the state codes; the labels are checked on the way
        const int32_t* lab = a.labels + l0;
        int bad = 0, rep = 0;
        for (int l = tid; l < L; l += NT) {
            const int v = lab[l];
            const int prev = l > 0 ? lab[l - 1] : -1;
            bad |= (v < 0 || v > C - 2);
            rep += (l > 0 && v == prev);
            int cd = (v & CODE_LABEL) | (a.merge ? CODE_SELF : 0);
            if (l > 0 && (!a.merge || v != prev)) cd |= CODE_SKIP_IN;
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
    if (s_bad) { no_path(a, i, NAN, PO_E_ARG, l0, L64, tid, NT); return; }
    if (po_ctc_min_frames(L, s_rep, a.merge) > T64) { no_path(a, i, -INFINITY, PO_E_ENVELOPE, l0, L64, tid, NT); return; }
    if (a.states)   // the padded frames
        for (int64_t t = T64 + tid; t < a.states_stride; t += NT) a.states[i * a.states_stride + t] = -1;
    if (T == 0) {   // (then L = 0: the empty path)
        if (tid == 0) { a.score[i] = 0.0; if (a.status) a.status[i] = 0; }
        return;
    }

    // ---- phase 0: lp[t][c] = log softmax of frame t, column perm[c] of the source (ctc_loss_kernel's arithmetic)
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
    // (a thread's state past the last one stands in for S - 1 wherever an address is made of it: the loads of the frame loop
    // are unconditional and their results unused)
    int cd[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cd[k] = code[min(tid + k * NT, S - 1)];
    __syncthreads();

    // ---- phase 1: V.  A state's transitions as operands chosen by its flags, the same instructions in every lane: an absent
    // transition enters as -inf and loses every comparison against a finite value; the comparisons are strict and run stay,
    // step, skip, so that a tie keeps the larger predecessor.
    uint64_t* B = a.bits + 2 * bo;   // frame t, word w: B[2 * (t * W + w)] the low plane, + 1 the high plane
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63), lane = tid & 63;   // (wave0 in a scalar register: tests on it are scalar)
    double nx[K] = {};   // lp of the next step at this thread's states
    // where a thread's state k is kept in a row: a state past the last one writes the row's spare cell S + 4 (S is odd, the row
    // has S + 5 cells and the borders end at S + 3), so that the store of the frame loop needs no lane mask kept over the loop
    int at[K];
#pragma unroll
    for (int k = 0; k < K; ++k) at[k] = tid + k * NT < S ? tid + k * NT + 2 : S + 4;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = tid + k * NT;
        if (s < S) rows[s + 2] = s < 2 ? lp[cd[k] & CODE_LABEL] : -INFINITY;
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
                const double stay = (cd[k] & CODE_SELF) ? p0 : -INFINITY;
                const double skip = (cd[k] & CODE_SKIP_IN) ? p2 : -INFINITY;
                const bool step_wins = p1 > stay;
                const double v1 = step_wins ? p1 : stay;
                const bool skip_wins = skip > v1;
                const double v = (skip_wins ? skip : v1) + now[k];
                cur[at[k]] = v;
                if (path) {
                    const uint64_t lo = __ballot(step_wins && !skip_wins), hi = __ballot(skip_wins);
                    if (lane == 0) {
                        uint64_t* w = B + 2 * ((int64_t)t * W + ((wave0 + k * NT) >> 6));
                        w[0] = lo; w[1] = hi;
                    }
                }
            }
        }
        __syncthreads();
    }
    const double* last = rows + ((T - 1) & 1) * SP;
    const double e1 = last[S + 1], e2 = last[S];   // states 2L and 2L - 1 (S = 1: the border, -inf)
    const bool second = e2 > e1;
    const double best = second ? e2 : e1;
    if (best == -INFINITY) { no_path(a, i, -INFINITY, PO_E_ENVELOPE, l0, L64, tid, NT); return; }
    if (tid == 0) { a.score[i] = best; if (a.status) a.status[i] = 0; }
    if (!path || tid >= 64) return;
    __threadfence_block();   // (the other waves' bit words were written before the loop's last barrier)

    // ---- phase 2: the trace-back, wave 0.  s: the path's state at the frame the walk stands at (the same in every lane).
    // A decision that a NaN made may be anything: the state is held at 0 from below and the word index inside the row, so
    // every address stays inside the item whatever the bits say.
    int s = second ? S - 2 : S - 1;
    int above = -1;   // the state of the frame after this block's last one
    for (int t0 = (T - 1) & ~(PO_FALIGN_BLOCK - 1); t0 >= 0; t0 -= PO_FALIGN_BLOCK) {
        const int jtop = min(PO_FALIGN_BLOCK - 1, T - 1 - t0);   // the block's last frame is t0 + jtop
        const int wtop = s >> 6;
        uint64_t lo[3], hi[3];   // the words wtop - 2 .. wtop of this lane's frame
        {
            const int64_t t = min(t0 + lane, T - 1);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int w = min(max(wtop - 2 + m, 0), W - 1);
                const uint64_t* p = B + 2 * (t * W + w);
                lo[m] = p[0]; hi[m] = p[1];
            }
        }
        int st = -1;   // this lane's frame's state
        for (int j = jtop; j >= 0; --j) {
            st = lane == j ? s : st;
            const int rel = (s >> 6) - wtop + 2, sh = s & 63;
            const uint64_t l = rel >= 2 ? lo[2] : (rel == 1 ? lo[1] : lo[0]);
            const uint64_t h = rel >= 2 ? hi[2] : (rel == 1 ? hi[1] : hi[0]);
            const int d = (int)((l >> sh) & 1) | ((int)((h >> sh) & 1) << 1);
            const int dj = __builtin_amdgcn_readlane(d, j);
            if (t0 + j > 0) s = max(s - dj, 0);   // (frame 0 has no decision; after the loop s is frame t0 - 1's state)
        }
        const int up_n = __shfl(st, min(lane + 1, 63), 64), dn_n = __shfl(st, max(lane - 1, 0), 64);
        const int up = lane == jtop ? above : up_n;
        const int dn = lane == 0 ? (t0 > 0 ? s : -1) : dn_n;
        if (lane <= jtop) {
            const int t = t0 + lane;
            if (a.states) a.states[i * a.states_stride + t] = st;
            if (st & 1) {
                if (a.starts && dn != st) a.starts[l0 + (st >> 1)] = t;
                if (a.stops && up != st) a.stops[l0 + (st >> 1)] = t + 1;
            }
        }
        above = __shfl(st, 0, 64);
    }
}

template <int CT>
void launch_class(int cls, const FaArgs& a, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)a.n);
    if (cls == 0) hipLaunchKernelGGL((falign_kernel<64, 2, CT>), grid, dim3(64), lds, s, a);
    else if (cls == 1) hipLaunchKernelGGL((falign_kernel<256, 2, CT>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((falign_kernel<256, 10, CT>), grid, dim3(256), lds, s, a);
}

struct FaPlan { size_t b_off, b_lp, b_bits; size_t total() const { return b_off + b_lp + b_bits; } };
FaPlan fa_plan(int n, int64_t total_rows, int64_t total_words, int C) {
    FaPlan p{0, 0, 0};
    if (n <= 0) return p;
    p.b_off = al256(sizeof(int64_t) * (size_t)n);
    p.b_lp = al256(sizeof(double) * (size_t)std::max<int64_t>(total_rows, 0) * (size_t)std::max(C, 0));
    p.b_bits = al256((size_t)PO_FALIGN_WORD_BYTES * (size_t)std::max<int64_t>(total_words, 0));
    return p;
}

// the refusals that need sizes only (po_forced_align, its twin): ctc_check's (po_ctc.hip), in its order
int fa_check(const std::string& w, int n, int C, int dtype, int normalize, const int* perm_h, int model, int64_t total_rows,
             int64_t total_words, int max_states) {
    if (model == PO_MODEL_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, w + ": the flip-flop model has no forced alignment here");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, w + ": unknown model");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (total_rows < 0 || total_words < 0 || max_states < 0) return po_fail(PO_E_ARG, w + ": negative total_rows, total_words or max_states");
    if (C < 2 || C > 8) return po_fail(PO_E_ARG, w + ": C must be 2..8");
    if (dtype < PO_DTYPE_F32 || dtype > PO_DTYPE_F64) return po_fail(PO_E_ARG, w + ": unknown dtype");
    if (perm_h) {
        unsigned seen = 0;
        for (int c = 0; c < C; ++c) {
            if (perm_h[c] < 0 || perm_h[c] >= C) return po_fail(PO_E_ARG, w + ": perm entry outside [0, C)");
            seen |= 1u << perm_h[c];
        }
        if (seen != (1u << C) - 1) return po_fail(PO_E_ARG, w + ": perm must name every column once");
    }
    if (normalize && dtype == PO_DTYPE_F64) return po_fail(PO_E_UNSUPPORTED, w + ": normalize with float64 input (the reference normalises in the array's own precision)");
    if (max_states > PO_CTC_MAX_STATES)
        return po_fail(PO_E_UNSUPPORTED, w + ": a label of more than " + std::to_string(PO_CTC_MAX_LABEL) + " symbols (" +
                       std::to_string((max_states - 1) / 2) + " here): the lattice rows are kept in LDS");
    return PO_OK;
}
}  // namespace

extern "C" {

size_t po_forced_align_workspace_bytes(int n, int64_t total_rows, int64_t total_words, int C) {
    po_fail(PO_OK, "");
    return fa_plan(n, total_rows, total_words, C).total();
}

int po_forced_align(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, int normalize,
                    const int* perm_h, const int32_t* labels, const int64_t* label_off, int model, int64_t total_rows,
                    int64_t total_words, int max_states, double* score, int32_t* states, int64_t states_stride, int32_t* starts,
                    int32_t* stops, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    po_fail(PO_OK, "");
    const std::string w("po_forced_align");
    int rc = fa_check(w, n, C, dtype, normalize, perm_h, model, total_rows, total_words, max_states);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;
    if (!items) return po_fail(PO_E_ARG, w + ": null items");
    if (!row_off) return po_fail(PO_E_ARG, w + ": null row_off");
    if (!labels) return po_fail(PO_E_ARG, w + ": null labels");
    if (!label_off) return po_fail(PO_E_ARG, w + ": null label_off");
    if (!score) return po_fail(PO_E_ARG, w + ": null score");
    if (states && (states_stride < 0 || states_stride < (total_rows + n - 1) / n))
        return po_fail(PO_E_ARG, w + ": states_stride " + std::to_string(states_stride) + " cannot hold the longest item (" +
                       std::to_string((total_rows + n - 1) / n) + " frames at least)");
    const FaPlan p = fa_plan(n, total_rows, total_words, C);
    if (!ws || ws_bytes < p.total()) return po_fail(PO_E_ARG, w + ": workspace smaller than po_forced_align_workspace_bytes");
    FaArgs a = {};
    a.items = items; a.row_off = row_off; a.labels = labels; a.label_off = label_off;
    a.n = n; a.C = C; a.dtype = dtype; a.normalize = normalize ? 1 : 0; a.merge = model == PO_MODEL_MERGE;
    a.max_states = std::max(max_states, 1);
    for (int c = 0; c < 8; ++c) a.perm[c] = (perm_h && c < C) ? perm_h[c] : (c < C ? c : 0);
    a.total_rows = total_rows; a.total_words = total_words; a.states_stride = states_stride;
    a.score = score; a.states = states; a.starts = starts; a.stops = stops; a.status = status;
    a.b_off = (const int64_t*)ws;
    a.lp = (double*)((char*)ws + p.b_off);
    a.bits = (uint64_t*)((char*)ws + p.b_off + p.b_lp);
    hipStream_t s = (hipStream_t)stream;
    if (states || starts || stops) hipLaunchKernelGGL(falign_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a, (int64_t*)ws);
    for (int c = 0; c < PO_CTC_NCLASS; ++c) {
        a.s_lo = c ? PO_CTC_CLASS_HI[c - 1] : 0;
        if (c > 0 && a.max_states <= a.s_lo) break;
        a.s_hi = PO_CTC_CLASS_HI[c];
        const size_t lds = po_falign_lds_bytes(std::min(a.s_hi, a.max_states));
        if (C == 5) launch_class<5>(c, a, lds, s); else launch_class<0>(c, a, lds, s);
    }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

int po_forced_align_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                      const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, int normalize,
                      const int* perm_h, const int32_t* labels_h, const int64_t* label_off_h, int model, double* score_h,
                      int32_t* states_h, int64_t states_stride, int32_t* starts_h, int32_t* stops_h, int32_t* status_h) {
    po_fail(PO_OK, "");
    const std::string w("po_forced_align_h");
    if (n > 0 && (!row_off_h || !label_off_h)) return po_fail(PO_E_ARG, w + ": null row_off or label_off");
    int64_t rows = 0, words = 0, max_states = 1, max_T = 0;
    for (int i = 0; i < std::max(n, 0); ++i) {
        const int64_t T = row_off_h[i + 1] - row_off_h[i], L = label_off_h[i + 1] - label_off_h[i];
        if (T < 0 || L < 0 || T > 0x7fffffff || L > (1 << 29)) return po_fail(PO_E_ARG, w + ": offsets must not decrease (an item has fewer than 2^31 frames)");
        rows += T;
        words += T * po_falign_row_words(2 * L + 1);
        max_states = std::max(max_states, 2 * L + 1);
        max_T = std::max(max_T, T);
    }
    int rc = fa_check(w, n, C, dtype, normalize, perm_h, model, rows, words, (int)max_states);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;
    if (!score_h || !item_off_h || !row_stride_h || !col_stride_h || (rows > 0 && !src_h) || (label_off_h[n] > label_off_h[0] && !labels_h))
        return po_fail(PO_E_ARG, w + ": null src, item table, labels or score");
    if (states_h && states_stride < max_T)
        return po_fail(PO_E_ARG, w + ": states_stride " + std::to_string(states_stride) + " is smaller than the longest item (" + std::to_string(max_T) + " frames)");
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
    std::vector<po_ingest_item> items(n);
    PoDev src, it, ro, lab, lo, sc, sts, sta, sto, st, ws;
    PO_HIPCHK(src.up(src_h, (size_t)std::max<int64_t>(src_elems, 0) * eb));
    for (int i = 0; i < n; ++i) items[i] = {src.as<char>() + (size_t)item_off_h[i] * eb, row_stride_h[i], col_stride_h[i]};
    PO_HIPCHK(it.up(items.data(), sizeof(po_ingest_item) * n));
    PO_HIPCHK(ro.up(row_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(lab.up(labels_h ? labels_h + lr.base : nullptr, sizeof(int32_t) * (size_t)lr.total));
    PO_HIPCHK(lo.up(lr.off.data(), lr.bytes()));
    PO_HIPCHK(sc.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t states_bytes = sizeof(int32_t) * (size_t)n * (size_t)std::max<int64_t>(states_stride, 0);
    if (states_h) PO_HIPCHK(sts.up(nullptr, states_bytes));
    if (starts_h) PO_HIPCHK(sta.up(nullptr, sizeof(int32_t) * (size_t)lr.total));
    if (stops_h) PO_HIPCHK(sto.up(nullptr, sizeof(int32_t) * (size_t)lr.total));
    const size_t wsb = po_forced_align_workspace_bytes(n, rows, words, C);
    PO_HIPCHK(ws.up(nullptr, wsb));
    rc = po_forced_align(it.as<po_ingest_item>(), ro, n, C, dtype, normalize, perm_h, lab, lo, model, rows, words, (int)max_states,
                         sc, states_h ? sts.as<int32_t>() : nullptr, states_stride, starts_h ? sta.as<int32_t>() : nullptr,
                         stops_h ? sto.as<int32_t>() : nullptr, st, ws, std::max<size_t>(wsb, 256), nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(sc.down(score_h, sizeof(double) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    if (states_h) PO_HIPCHK(sts.down(states_h, states_bytes));
    if (starts_h) PO_HIPCHK(sta.down(starts_h + lr.base, sizeof(int32_t) * (size_t)lr.total));
    if (stops_h) PO_HIPCHK(sto.down(stops_h + lr.base, sizeof(int32_t) * (size_t)lr.total));
    return PO_OK;
}

}  // extern "C"
