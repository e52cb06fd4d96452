// po_label.hip — guided, banded CTC forced alignment for make_labeled_data: the frame of every base of
// a known sequence over a whole read.  The specification is in include/poreover_hip.h (po_label_align_batch); every cell
// is one float64 addition and one comparison, so tests/_label_oracle.py (numpy) and this file agree bit for bit.
//
// Mapping: one wave per read.  State k lives at ring index (k + B + 1) mod W, W = 64 * NS >= 2B + 2: lane = index mod 64,
// slot = index / 64.  The ring of row t starts one state below the band (k = c[t] - B - 1, which is how S(-1, 0) is seen
// by a first row that does not admit state 0), so a sliding band moves no data: a lane whose state left the band at the
// bottom finds a new k = old k + W, starts from -inf and takes the new state's label code.  Everything that does not
// depend on the scores (c[t], the lane's k, whether the cell is admitted, its y value) is folded into two addends per
// cell, -inf where a move is not allowed; the dependent chain of a row is a lane rotate (wave_shr:1 + one v_readlane),
// two additions, a comparison and a select; the addends of row t + 1 are made before the chain of row t runs.
//   label_forward_kernel<NS>   NS = 1 (B <= 31), 2 (B <= 63): scores in registers; 64 rows of y (and of the guide) are
//                              staged through LDS, the next 64 requested before the current ones are walked; the label
//                              codes of the band's neighbourhood sit in a 512-byte LDS window; a row's decisions are
//                              one __ballot per slot, kept by lane (t mod 64) and stored 64 rows at a time (coalesced)
//   label_forward_general_kernel  any band (NS per read from a host-made table; band_size <= 0 or B >= L: the ring is
//                              the whole state axis): slots looped over the lanes, scores in LDS (up to 4096 states) or
//                              in the workspace
//   label_trace_kernel         walks the bits back from (T-1, L): the row addresses do not depend on k, so the wave
//                              fetches 64 rows' words at once (the next 64 while it walks), and walks them by v_readlane
// Trace-back storage: NS 64-bit words per frame.  No atomics, no hand-off between workgroups; a read's result depends
// on nothing but the read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"

#include "po_hostbuf.h"

namespace {

constexpr int LB_CH = 64;        // rows per staged chunk (= lanes: lane r keeps row r's decision words)
constexpr int LB_LABW = 512;     // label codes in the LDS window
constexpr int LB_LDSV = 4096;    // general kernel: ring states kept in LDS (more: in the workspace)
constexpr int LB_FAST_MAX_B = 63;

struct LBDesc {                  // general kernel, per read (made on the host from the offsets)
    int64_t word_off;            // first decision word
    int64_t val_off;             // first ring double in the workspace, or -1: LDS
    int32_t ns, beff, full, pad;
};

struct LBArgs {
    const double* y; const int64_t* y_off; int n, A; uint32_t alphabet;
    const char* labels; const int64_t* label_off; const int32_t* guide; int band;
    int32_t* map; double* score; int32_t* status;
    unsigned long long* bits; const LBDesc* desc; double* vals;
    int ns_fixed;                // trace kernel: NS of the register kernels, 0: take it from desc
};

__device__ __forceinline__ double lb_neg_inf() { return -__builtin_inf(); }

__device__ __forceinline__ int lb_code(uint32_t alphabet, int A, char c) {
    int code = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < A && (char)((alphabet >> (8 * i)) & 0xffu) == c) code = i;
    return code;
}

// lane i <- lane i - 1; lane 0 <- `first` (wave-uniform)
__device__ __forceinline__ double lb_shift_up(double x, double first) {
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(x), 0x138, 0xf, 0xf, false);  // wave_shr:1
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lb_readlane_d(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// Rows t0 .. t0 + 63 of y (lane + 64 j of the chunk's C * rows doubles) and of the guide into registers.  A guide value
// outside [0, L] or below its predecessor marks the read (bad) and is clamped, so that whatever follows stays in range.
__device__ __forceinline__ void lb_fetch(const double* y, const int32_t* g, int t0, int T, int L, int C, int lane,
                                         double (&yv)[5], int& cv, int& bad) {
    const int nval = min(LB_CH, T - t0) * C;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int idx = lane + 64 * j;
        yv[j] = idx < nval ? y[(int64_t)t0 * C + idx] : 0.0;
    }
    const int t = t0 + lane;
    cv = L;
    if (t < T) {
        if (g) {
            const int c = g[t], p = t > 0 ? g[t - 1] : 0;
            bad |= (c < 0) | (c > L) | (c < p);
            cv = min(max(c, 0), L);
        } else {
            cv = (int)(((int64_t)(t + 1) * L) / T);
        }
    }
}

__device__ __forceinline__ void lb_stage(double* ybuf, int* cbuf, int lane, const double (&yv)[5], int cv) {
#pragma unroll
    for (int j = 0; j < 5; ++j) ybuf[lane + 64 * j] = yv[j];
    cbuf[lane] = cv;
}

__device__ __forceinline__ int lb_label_scan(const LBArgs& a, const char* lab, int L, int lane) {
    int bad = 0;
    for (int j = lane; j < L; j += 64) bad |= (lb_code(a.alphabet, a.A, lab[j]) < 0);
    return bad;
}

__device__ __forceinline__ void lb_finish(const LBArgs& a, int i, int lane, bool bad, double score) {
    if (lane == 0) {
        const bool lost = !(score > lb_neg_inf());
        a.status[i] = bad ? PO_E_ARG : (lost ? PO_E_ENVELOPE : PO_OK);
        a.score[i] = (bad || lost) ? lb_neg_inf() : score;
    }
}

}  // namespace

template <int NS>
__global__ __launch_bounds__(64) void label_forward_kernel(LBArgs a) {
    constexpr int W = 64 * NS;
    __shared__ double ybuf[LB_CH * 5];
    __shared__ int cbuf[LB_CH];
    __shared__ unsigned char lwin[LB_LABW];
    const int lane = threadIdx.x, i = blockIdx.x;
    const int A = a.A, C = A + 1, B = a.band;
    const int64_t r0 = a.y_off[i];
    const int T = (int)(a.y_off[i + 1] - r0);
    const double* y = a.y + r0 * C;
    const char* lab = a.labels + a.label_off[i];
    const int L = (int)(a.label_off[i + 1] - a.label_off[i]);
    const int32_t* g = a.guide ? a.guide + r0 : nullptr;
    unsigned long long* bits = a.bits + r0 * NS;
    const double NINF = lb_neg_inf();

    int bad = lb_label_scan(a, lab, L, lane);
    if (T <= 0) {
        lb_finish(a, i, lane, __ballot(bad) != 0ull, L == 0 ? 0.0 : NINF);
        return;
    }
    double yv[5];
    int cv;
    lb_fetch(y, g, 0, T, L, C, lane, yv, cv, bad);

    double val[NS];
    int kcur[NS], code[NS];
    unsigned long long mybits[NS];
    int cprev = 0, wbase = 0;
    auto fill_window = [&](int base) {
        wbase = base;
        for (int j = lane; j < LB_LABW; j += 64) {
            const int k = base + j;
            lwin[j] = (k >= 1 && k <= L) ? (unsigned char)(lb_code(a.alphabet, A, lab[k - 1]) & 3) : (unsigned char)0;
        }
    };
    auto code_of = [&](int k) -> int {
        const int j = k - wbase;
        if (j >= 0 && j < LB_LABW) return lwin[j];
        if (k >= 1 && k <= L) return lb_code(a.alphabet, A, lab[k - 1]) & 3;   // a guide that outruns the window
        return 0;
    };

    for (int t0 = 0; t0 < T; t0 += LB_CH) {
        const int nrow = min(LB_CH, T - t0);
        lb_stage(ybuf, cbuf, lane, yv, cv);
        __syncthreads();
        if (t0 + LB_CH < T) lb_fetch(y, g, t0 + LB_CH, T, L, C, lane, yv, cv, bad);   // the next chunk is on its way
        const int cfirst = cbuf[0], clast = cbuf[nrow - 1];
        if (t0 == 0) {
            fill_window(cfirst - B - 1);
            __syncthreads();
            cprev = cfirst;   // row -1 sits where row 0 does: S(-1, 0) = 0, every other state -inf
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int ridx = lane + 64 * s;
                kcur[s] = cfirst - B - 1 + ((ridx - cfirst) & (W - 1));
                val[s] = kcur[s] == 0 ? 0.0 : NINF;
                code[s] = code_of(kcur[s]);
                mybits[s] = 0ull;
            }
        } else if (clast + W - B - 1 > wbase + LB_LABW) {
            __syncthreads();
            fill_window(cfirst - B - 1);
            __syncthreads();
        }
        // The chunk's guide and blank column, one row per lane: row r's come by v_readlane.  prep(r) makes the row's two
        // addends per cell (-inf where the move is not allowed); nothing in it depends on the scores, so the next row's
        // is issued before the current row's chain and its LDS reads fly underneath.
        const int cchunk = cbuf[lane];
        const double ybchunk = ybuf[min(lane, nrow - 1) * C + A];
        auto prep = [&](int r, double (&add_stay)[NS], double (&add_emit)[NS]) {
            const int c = __builtin_amdgcn_readlane(cchunk, r);
            const double yb = lb_readlane_d(ybchunk, r);
            const int lo = max(0, c - B), hi = min(L, c + B);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int ridx = lane + 64 * s;
                const int knew = c - B - 1 + ((ridx - c) & (W - 1));
                const int kleft = cprev - B - 1 + ((ridx - 1 - cprev) & (W - 1));   // the state ring index ridx - 1 held
                const bool same = (knew == kcur[s]);
                if (!same) {
                    code[s] = code_of(knew);
                    kcur[s] = knew;
                }
                const bool adm = (knew >= lo) && (knew <= hi);
                const double ye = ybuf[r * C + code[s]];
                add_stay[s] = (same && adm) ? yb : NINF;
                add_emit[s] = (kleft == knew - 1 && adm) ? ye : NINF;
            }
            cprev = c;
        };
        double add_stay[NS], add_emit[NS];
        prep(0, add_stay, add_emit);
        for (int r = 0; r < nrow; ++r) {
            double next_stay[NS], next_emit[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) next_stay[s] = next_emit[s] = NINF;
            if (r + 1 < nrow) prep(r + 1, next_stay, next_emit);
            double top[NS];   // lane 63 of each slot: lane 0 of the next slot's k - 1 neighbour
#pragma unroll
            for (int s = 0; s < NS; ++s) top[s] = lb_readlane_d(val[s], 63);
            double nv[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double left = lb_shift_up(val[s], top[(s + NS - 1) % NS]);
                const double stay = val[s] + add_stay[s];
                const double emit = left + add_emit[s];
                const bool take = emit > stay;
                nv[s] = take ? emit : stay;
                const unsigned long long bw = __ballot(take);
                if (lane == r) mybits[s] = bw;
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                val[s] = nv[s];
                add_stay[s] = next_stay[s];
                add_emit[s] = next_emit[s];
            }
        }
        if (lane < nrow) {
#pragma unroll
            for (int s = 0; s < NS; ++s) bits[(int64_t)(t0 + lane) * NS + s] = mybits[s];
        }
        __syncthreads();   // the LDS rows are rewritten at the top
    }
    // S(T-1, L): ring index (L + B + 1) mod W, if that lane's state is L
    const int ridxL = (L + B + 1) & (W - 1);
    double v = val[0];
    int kk = kcur[0];
#pragma unroll
    for (int s = 1; s < NS; ++s)
        if ((ridxL >> 6) == s) { v = val[s]; kk = kcur[s]; }
    v = lb_readlane_d(v, ridxL & 63);
    kk = __builtin_amdgcn_readlane(kk, ridxL & 63);
    lb_finish(a, i, lane, __ballot(bad) != 0ull, kk == L ? v : NINF);
}

__global__ __launch_bounds__(64) void label_forward_general_kernel(LBArgs a) {
    __shared__ double ybuf[LB_CH * 5];
    __shared__ int cbuf[LB_CH];
    __shared__ double lvals[LB_LDSV];
    const int lane = threadIdx.x, i = blockIdx.x;
    const LBDesc d = a.desc[i];
    const int A = a.A, C = A + 1, NS = d.ns, B = d.beff, Wr = 64 * NS;
    const int64_t r0 = a.y_off[i];
    const int T = (int)(a.y_off[i + 1] - r0);
    const double* y = a.y + r0 * C;
    const char* lab = a.labels + a.label_off[i];
    const int L = (int)(a.label_off[i + 1] - a.label_off[i]);
    const int32_t* g = a.guide ? a.guide + r0 : nullptr;
    unsigned long long* bits = a.bits + d.word_off;
    double* vals = d.val_off >= 0 ? a.vals + d.val_off : lvals;   // lane l touches only indices l + 64 s
    const double NINF = lb_neg_inf();

    int bad = lb_label_scan(a, lab, L, lane);
    if (T <= 0) {
        lb_finish(a, i, lane, __ballot(bad) != 0ull, L == 0 ? 0.0 : NINF);
        return;
    }
    // k of ring index ridx in the row whose guide value is c (cm = c mod Wr)
    auto k_of = [&](int ridx, int c, int cm) { int x = ridx - cm; x += (x < 0) ? Wr : 0; return c - B - 1 + x; };
    int cprev = 0, cpm = 0;
    for (int t0 = 0; t0 < T; t0 += LB_CH) {
        const int nrow = min(LB_CH, T - t0);
        double yv[5];
        int cv;
        lb_fetch(y, g, t0, T, L, C, lane, yv, cv, bad);
        __syncthreads();
        lb_stage(ybuf, cbuf, lane, yv, cv);
        __syncthreads();
        if (t0 == 0) {
            cprev = d.full ? L : cbuf[0];
            cpm = cprev % Wr;
            for (int s = 0; s < NS; ++s) vals[lane + 64 * s] = k_of(lane + 64 * s, cprev, cpm) == 0 ? 0.0 : NINF;
        }
        for (int r = 0; r < nrow; ++r) {
            // full: the ring is the whole state axis [-1, L] (storage only: it sits where c = L, B = L would put it);
            // what a row admits is always the guide's band
            const int cg = cbuf[r], c = d.full ? L : cg, cm = c % Wr;
            const double* yr = &ybuf[r * C];
            const double yb = yr[A];
            const int lo = a.band >= 1 ? max(0, cg - a.band) : 0, hi = a.band >= 1 ? min(L, cg + a.band) : L;
            double vcur = vals[lane + 64 * (NS - 1)];
            double carry = lb_readlane_d(vcur, 63);   // ring index Wr - 1: the neighbour of index 0
            for (int s = NS - 1; s >= 0; --s) {
                const int ridx = lane + 64 * s;
                const double vbelow = s > 0 ? vals[ridx - 64] : 0.0;   // slot s - 1, not yet updated
                const double first = s > 0 ? lb_readlane_d(vbelow, 63) : carry;
                const int knew = k_of(ridx, c, cm);
                const int kold = k_of(ridx, cprev, cpm);
                const int kleft = k_of(ridx == 0 ? Wr - 1 : ridx - 1, cprev, cpm);
                const bool adm = (knew >= lo) && (knew <= hi);
                const int cd = (adm && knew >= 1) ? (lb_code(a.alphabet, A, lab[knew - 1]) & 3) : 0;
                const double ye = yr[min(cd, A)];
                const double add_stay = (knew == kold && adm) ? yb : NINF;
                const double add_emit = (kleft == knew - 1 && adm) ? ye : NINF;
                const double left = lb_shift_up(vcur, first);
                const double stay = vcur + add_stay;
                const double emit = left + add_emit;
                const bool take = emit > stay;
                vals[ridx] = take ? emit : stay;
                const unsigned long long bw = __ballot(take);
                if (lane == 0) bits[(int64_t)(t0 + r) * NS + s] = bw;
                vcur = vbelow;
            }
            cprev = c;
            cpm = cm;
        }
    }
    const int ridxL = (L + B + 1) % Wr;
    const double v = lb_readlane_d(vals[lane + 64 * (ridxL >> 6)], ridxL & 63);
    const int kk = __builtin_amdgcn_readlane(k_of(lane + 64 * (ridxL >> 6), cprev, cpm), ridxL & 63);
    lb_finish(a, i, lane, __ballot(bad) != 0ull, kk == L ? v : NINF);
}

// One wave per read.  Lane j holds the decision words of row tc + j for the slot the walk is in and the one below (64
// rows move k by at most 64 states = one slot boundary); the words of the next 64 rows, for the three slots the walk
// can be in by then, are requested before the current rows are walked.
__global__ __launch_bounds__(64) void label_trace_kernel(LBArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int64_t r0 = a.y_off[i];
    const int T = (int)(a.y_off[i + 1] - r0);
    const int L = (int)(a.label_off[i + 1] - a.label_off[i]);
    int32_t* map = a.map + a.label_off[i];
    if (a.status[i] != PO_OK) {
        for (int j = lane; j < L; j += 64) map[j] = -1;
        return;
    }
    if (L == 0 || T <= 0) return;
    int NS, B;
    const unsigned long long* bits;
    if (a.ns_fixed) {
        NS = a.ns_fixed; B = a.band; bits = a.bits + r0 * NS;
    } else {
        const LBDesc d = a.desc[i];
        NS = d.ns; B = d.beff; bits = a.bits + d.word_off;
    }
    const int Wr = 64 * NS;
    int k = L, rr = (L + B + 1) % Wr;   // rr: ring index of k, stepped down with it
    int tc = ((T - 1) / LB_CH) * LB_CH;
    auto dn = [&](int s, int by) { int x = s - by; return x < 0 ? x + NS : x; };   // by <= 2; NS may be 1
    auto fetch3 = [&](int t0, int s0, unsigned long long (&w)[3]) {
        const int t = t0 + lane;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            int s = s0;
            for (int z = 0; z < q; ++z) s = dn(s, 1);
            w[q] = (t < T) ? bits[(int64_t)t * NS + s] : 0ull;
        }
    };
    int s0 = rr >> 6;           // slot of w[0]
    unsigned long long w[3], wn[3] = {0ull, 0ull, 0ull};
    fetch3(tc, s0, w);
    while (k > 0 && tc >= 0) {
        if (tc >= LB_CH) fetch3(tc - LB_CH, s0, wn);
        const int nrow = min(LB_CH, T - tc);
        const int s1 = dn(s0, 1);
        for (int j = nrow - 1; j >= 0 && k > 0; --j) {
            const int s = rr >> 6;
            const unsigned long long wsel = (s == s0) ? w[0] : w[1];
            const int half = (rr & 32) ? (int)(wsel >> 32) : (int)(wsel & 0xffffffffull);
            const int word = __builtin_amdgcn_readlane(half, j);
            if ((word >> (rr & 31)) & 1) {
                if (lane == 0) map[k - 1] = tc + j;
                --k;
                rr = rr == 0 ? Wr - 1 : rr - 1;
            }
        }
        // the slot the walk is in now is s0 or the one below it
        const int snow = rr >> 6;
        if (snow == s0) { w[0] = wn[0]; w[1] = wn[1]; }
        else { w[0] = wn[1]; w[1] = wn[2]; s0 = s1; }
        tc -= LB_CH;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
namespace {

inline bool lb_fast(int band) { return band >= 1 && band <= LB_FAST_MAX_B; }
inline int lb_fast_ns(int band) { return (2 * band + 2 <= 64) ? 1 : 2; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// slots of one read on the general kernel: the band's ring, or the whole state axis when that is no larger
inline void lb_general_shape(int64_t L, int band, int32_t* ns, int32_t* beff, int32_t* full) {
    const int64_t ns_full = cdiv(L + 2, 64);
    const int64_t ns_band = band >= 1 ? cdiv(2 * (int64_t)band + 2, 64) : ns_full + 1;
    if (band < 1 || band >= L || ns_full <= ns_band) { *ns = (int32_t)ns_full; *beff = (int32_t)L; *full = 1; }
    else { *ns = (int32_t)ns_band; *beff = band; *full = 0; }
}

// upper bound on the general kernel's decision words from the batch's totals alone
inline double lb_general_words_bound(int n, int64_t total_rows, int64_t max_rows, int64_t total_labels, int band) {
    double u = std::min((double)total_rows * (double)cdiv(total_labels + 2, 64),
                        (double)max_rows * ((double)total_labels / 64.0 + 2.0 * n));
    if (band >= 1) u = std::min(u, (double)total_rows * (double)cdiv(2 * (int64_t)band + 2, 64));
    return u;
}

}  // namespace

extern "C" {

size_t po_label_align_workspace_bytes(int n, int64_t total_rows, int64_t max_rows, int64_t total_labels, int band_size) {
    if (n < 0 || total_rows < 0 || max_rows < 0 || total_labels < 0) return 0;
    if (lb_fast(band_size)) return al256((size_t)total_rows * lb_fast_ns(band_size) * 8) + 256;
    const double words = lb_general_words_bound(n, total_rows, max_rows, total_labels, band_size);
    return al256((size_t)(words * 8.0) + 8) + al256(32 * (size_t)total_labels) + al256(sizeof(LBDesc) * (size_t)n) + 256;
}

int po_label_align_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int band_size,
                         const char* labels, const int64_t* label_off, const int32_t* guide, int32_t* map, double* score,
                         int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    po_set_error("");
    if (n < 0 || !y_off || !label_off || (n > 0 && (!y || !labels || !map || !score || !status || !ws)))
        return po_fail(PO_E_ARG, "po_label_align_batch: null argument");
    const char* alpha = alphabet ? alphabet : "ACGT";
    const size_t A = std::strlen(alpha);
    if (A < 1 || A > 4) return po_fail(PO_E_ARG, "po_label_align_batch: alphabet must have 1..4 symbols");
    if (C != (int)A + 1) return po_fail(PO_E_ARG, "po_label_align_batch: C must be len(alphabet) + 1 (the plain ctc model)");
    if (n == 0) return PO_OK;
    hipStream_t s = (hipStream_t)stream;
    LBArgs a = {};
    a.y = y; a.y_off = y_off; a.n = n; a.A = (int)A; a.labels = labels; a.label_off = label_off; a.guide = guide;
    a.band = std::min(band_size, 1 << 30); a.map = map; a.score = score; a.status = status;
    for (size_t i = 0; i < A; ++i) a.alphabet |= (uint32_t)(unsigned char)alpha[i] << (8 * i);
    if (lb_fast(band_size)) {
        // The register kernels take no table from the host (NS words per row at y_off[i] * NS).  Only the total row
        // count is read back (one blocking 8-byte copy per call, as the neighbours' batch_maxima) to refuse a workspace
        // that is too small; the offsets themselves are the caller's to keep non-decreasing, reads below 2^31 frames.
        int64_t rows = 0;
        PO_HIPCHK(hipMemcpyAsync(&rows, y_off + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PO_HIPCHK(hipStreamSynchronize(s));
        const int ns = lb_fast_ns(band_size);
        if (ws_bytes < (size_t)rows * ns * 8) return po_fail(PO_E_CAP, "po_label_align_batch: workspace too small");
        a.bits = (unsigned long long*)ws;
        a.ns_fixed = ns;
        if (ns == 1) hipLaunchKernelGGL(label_forward_kernel<1>, dim3(n), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(label_forward_kernel<2>, dim3(n), dim3(64), 0, s, a);
    } else {
        std::vector<int64_t> h(2 * (size_t)(n + 1));
        PO_HIPCHK(po_read_tables(y_off, label_off, n, s, h.data()));
        std::vector<LBDesc> desc((size_t)n);
        int64_t words = 0, nvals = 0;
        for (int i = 0; i < n; ++i) {
            const int64_t T = h[i + 1] - h[i], L = h[n + 1 + i + 1] - h[n + 1 + i];
            if (T < 0 || L < 0 || T >= ((int64_t)1 << 31) || L >= ((int64_t)1 << 30))
                return po_fail(PO_E_ARG, "po_label_align_batch: offsets must not decrease, reads must be shorter than 2^31 frames");
            LBDesc& d = desc[i];
            lb_general_shape(L, band_size, &d.ns, &d.beff, &d.full);
            d.word_off = words;
            words += T * d.ns;
            const int64_t wr = 64 * (int64_t)d.ns;
            d.val_off = -1;
            if (wr > LB_LDSV) { d.val_off = nvals; nvals += wr; }
            d.pad = 0;
        }
        const size_t b_bits = al256((size_t)words * 8 + 8), b_vals = al256((size_t)nvals * 8), b_desc = al256(sizeof(LBDesc) * (size_t)n);
        if (ws_bytes < b_bits + b_vals + b_desc) return po_fail(PO_E_CAP, "po_label_align_batch: workspace too small");
        a.bits = (unsigned long long*)ws;
        a.vals = (double*)((char*)ws + b_bits);
        a.desc = (const LBDesc*)((char*)ws + b_bits + b_vals);
        PO_HIPCHK(hipMemcpyAsync((void*)a.desc, desc.data(), sizeof(LBDesc) * (size_t)n, hipMemcpyHostToDevice, s));
        PO_HIPCHK(hipStreamSynchronize(s));   // desc lives on this stack
        a.ns_fixed = 0;
        hipLaunchKernelGGL(label_forward_general_kernel, dim3(n), dim3(64), 0, s, a);
    }
    hipLaunchKernelGGL(label_trace_kernel, dim3(n), dim3(64), 0, s, a);
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

int po_label_align_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int band_size,
                           const char* labels_h, const int64_t* label_off_h, const int32_t* guide_h, int32_t* map_h,
                           double* score_h, int32_t* status_h) {
    po_set_error("");
    if (n <= 0) return n < 0 ? po_fail(PO_E_ARG, "po_label_align_batch_h: negative n") : PO_OK;
    if (!y_off_h || !label_off_h || !score_h || !status_h) return po_fail(PO_E_ARG, "po_label_align_batch_h: null argument");
    const PoRagged r(y_off_h, n, true), l(label_off_h, n, true);
    if (!r.ordered || !l.ordered) return po_fail(PO_E_ARG, "po_label_align_batch_h: offsets must not decrease");
    if ((r.total > 0 && !y_h) || (l.total > 0 && (!labels_h || !map_h))) return po_fail(PO_E_ARG, "po_label_align_batch_h: null argument");
    PoRows y, lb;
    PoDev gd, mp, sc, st, ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(lb.up(labels_h, l, 1));
    if (guide_h) PO_HIPCHK(gd.up(guide_h + r.base, sizeof(int32_t) * r.total));   // one state per frame, at the read's rows
    PO_HIPCHK(mp.up(nullptr, sizeof(int32_t) * l.total));
    PO_HIPCHK(sc.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_label_align_workspace_bytes(n, r.total, r.max, l.total, band_size);
    PO_HIPCHK(ws.up(nullptr, wsb));
    const int rc = po_label_align_batch(y.data, y.off, n, C, alphabet, band_size, lb.data, lb.off, gd, mp, sc, st, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(mp.down(map_h + l.base, sizeof(int32_t) * l.total));   // one frame per base, at the label's place in the caller's table
    PO_HIPCHK(sc.down(score_h, sizeof(double) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

}  // extern "C"
