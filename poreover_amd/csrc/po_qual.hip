// po_qual.hip — per-base log-odds of a called sequence (decode --fastq): a guided, banded forward-backward
// lattice over a whole read.  The specification is in include/poreover_hip.h (po_qual_batch); tests/_qual_oracle.py is
// its numpy restatement.
//
// Rows are indexed by u = 0 .. T, "after frame u - 1".  Row 0 admits state 0, row u >= 1 the band of frame u - 1.
// One wave per read, two passes:
//   pass 1  the backward lattice, row T down to row 0; every row goes to the workspace (W doubles, 2 W for the merge
//           model's blank and label states), logp = beta(0, 0)
//   pass 2  the forward lattice, frame 0 up to T - 1, streamed through LDS; frame t joins alpha(row t) with the stored
//           beta(row t + 1) into the five accumulators of every label position the band holds
// Ring: state k lives at index k mod W, W = 2B + 2: the storage window of a row is [c - B - 1, c + B], one state below
// the band.  The accumulators (and the merge model's four substitution runs) of position p live at the index of state
// p + 1 and stay there while that state is in the window; every term of position p needs state p + 1 (substitution)
// or p + 2 (deletion) admitted in row t + 1, so p + 1 is in that row's window whenever there is something to add.  When
// the guide moves the window past a state, its index takes the next state (k + W) and the finished position is written
// out.  A band at least as wide as the label (or no band) keeps the whole state axis: W = L + 1.
// Everything is log-space float64 (logaddexp); no atomics, no hand-off between workgroups; a read's result depends on
// nothing but the read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"

#include "po_hostbuf.h"

namespace {

constexpr int QL_LDS_MAX = 6144;   // doubles of state one read may keep in LDS (48 KiB); more: in the workspace

struct QDesc {                     // per read (made on the host from the offsets)
    int64_t beta_off;              // first double of the read's stored rows
    int64_t st_off;                // first double of its state in the workspace, or -1: LDS
    int32_t wr, full;
    int32_t read, pad;             // the read (the table is sorted by the size of the state, one launch per class)
};

struct QArgs {
    const double* y; const int64_t* y_off; int n, A; uint32_t alphabet; int merge;
    const char* labels; const int64_t* label_off; const int32_t* guide; int band;
    double* odds; double* logp; int32_t* status;
    double* beta; const QDesc* desc; double* st;
    int first;                     // first entry of desc of this launch
};

__device__ __forceinline__ double q_ninf() { return -__builtin_inf(); }

__device__ __forceinline__ int q_code(uint32_t alphabet, int A, char c) {
    int code = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < A && (char)((alphabet >> (8 * i)) & 0xffu) == c) code = i;
    return code;
}

// log(exp(a) + exp(b)); -inf for two -inf
__device__ __forceinline__ double q_lae(double a, double b) {
    const double m = fmax(a, b), d = fmin(a, b) - m;
    return (d > -745.0) ? m + log1p(exp(d)) : m;   // d is NaN for two -inf, -inf for one: m
}

struct QRow { int base, bm, lo, hi; };   // storage window [base, base + W), admitted [lo, hi]

}  // namespace

__global__ __launch_bounds__(64) void qual_kernel(QArgs a) {
    extern __shared__ double q_lds[];
    const int lane = threadIdx.x;
    const QDesc d = a.desc[a.first + blockIdx.x];
    const int i = d.read;
    const int A = a.A, C = A + 1, B = a.band;
    const int64_t W = d.wr;   // int64: b * W + ridx and the row offsets are formed in 64 bits
    const bool merge = a.merge != 0, full = d.full != 0;
    const int64_t r0 = a.y_off[i];
    const int T = (int)(a.y_off[i + 1] - r0);
    const double* y = a.y + r0 * C;
    const char* lab = a.labels + a.label_off[i];
    const int L = (int)(a.label_off[i + 1] - a.label_off[i]);
    const int32_t* g = a.guide ? a.guide + r0 : nullptr;
    double* odds = a.odds + a.label_off[i] * 5;
    const double NINF = q_ninf();

    // ---- arguments: label characters, guide ----
    int bad = 0;
    for (int j = lane; j < L; j += 64) bad |= (q_code(a.alphabet, A, lab[j]) < 0);
    if (g)
        for (int t = lane; t < T; t += 64) {
            const int c = g[t], p = t > 0 ? g[t - 1] : 0;
            bad |= (c < 0) | (c > L) | (c < p);
        }
    bad = __ballot(bad) != 0ull;
    for (int64_t j = lane; j < (int64_t)L * 5; j += 64) odds[j] = 0.0;
    if (bad || L == 0 || T <= 0) {
        if (lane == 0) {
            double bs = 0.0;
            if (!bad && L == 0)
                for (int t = 0; t < T; ++t) bs = bs + y[(int64_t)t * C + A];
            const bool ok = !bad && L == 0;
            a.status[i] = bad ? PO_E_ARG : (ok ? PO_OK : PO_E_ENVELOPE);
            a.logp[i] = ok ? bs : NINF;
        }
        return;
    }

    auto code_at = [&](int k) -> int { return q_code(a.alphabet, A, lab[k]) & 3; };   // 0 <= k < L
    // row u = 0 .. T
    auto row_of = [&](int u) -> QRow {
        const int t = u > 0 ? u - 1 : 0;
        const int c = g ? g[t] : (int)(((int64_t)(t + 1) * L) / T);
        QRow r;
        r.base = full ? 0 : c - B - 1;
        int bm = r.base % (int)W;
        r.bm = bm < 0 ? bm + W : bm;
        r.lo = B >= 1 ? max(0, c - B) : 0;
        r.hi = B >= 1 ? min(L, c + B) : L;
        if (u == 0) r.lo = r.hi = 0;
        return r;
    };
    auto k_of = [&](int ridx, const QRow& r) -> int { int x = ridx - r.bm; x += (x < 0) ? W : 0; return r.base + x; };
    auto adm = [&](int k, const QRow& r) -> bool { return k >= r.lo && k <= r.hi; };
    auto up = [&](int ridx) -> int { return ridx + 1 == W ? 0 : ridx + 1; };
    auto down = [&](int ridx) -> int { return ridx == 0 ? W - 1 : ridx - 1; };

    const int nb = merge ? 2 : 1, nbx = nb - 1;
    double* st = d.st_off >= 0 ? a.st + d.st_off : q_lds;
    double* beta = a.beta + d.beta_off;          // row u: beta[(u * nb + which) * W + ridx]
    double* buf0 = st;                           // [nb][W]
    double* buf1 = st + (size_t)nb * W;
    double* acc = st + (size_t)2 * nb * W;       // [5][W]
    double* run = acc + (size_t)5 * W;           // [4][W] (merge)
    int* kst = (int*)(run + (size_t)(merge ? 4 : 0) * W);   // [W] the state whose label codes cpk holds
    int* cpk = kst + W;                          // [W] s[k-2] | s[k-1] << 4 | s[k] << 8 (15: there is none)
    // Nothing the chain of a row waits for comes from global memory at the moment it is needed: the guide value and the
    // y row of the next step are requested one step ahead (uniform loads), so are the stored rows of the first 64 ring
    // indices, and the label codes around a ring index's state are kept in LDS and read again only when the window
    // moves that index to another state.  kst / cpk [i] are touched by lane i mod 64 alone.
    for (int ridx = lane; ridx < W; ridx += 64) kst[ridx] = -0x7fffffff;
    auto pack_of = [&](int ridx, int k) -> int {
        if (kst[ridx] != k) {
            const int c2 = (k >= 2 && k - 2 < L) ? code_at(k - 2) : 15;
            const int c1 = (k >= 1 && k - 1 < L) ? code_at(k - 1) : 15;
            const int c0 = (k >= 0 && k < L) ? code_at(k) : 15;
            cpk[ridx] = c2 | (c1 << 4) | (c0 << 8);
            kst[ridx] = k;
        }
        return cpk[ridx];
    };
    auto load_y = [&](int t, double (&ye)[4], double& yb) {
        const double* yr = y + (int64_t)t * C;
#pragma unroll
        for (int b = 0; b < 4; ++b) ye[b] = b < A ? yr[b] : NINF;
        yb = yr[A];
    };
    auto ysel = [&](const double (&ye)[4], int c) -> double { return c == 0 ? ye[0] : (c == 1 ? ye[1] : (c == 2 ? ye[2] : ye[3])); };

    // ---- pass 1: backward ----
    {
        double* prev = buf0;   // row u + 1
        double* cur = buf1;
        QRow rn = row_of(T);
        for (int ridx = lane; ridx < W; ridx += 64) {
            const int k = k_of(ridx, rn);
            const double v = (k == L && adm(k, rn)) ? 0.0 : NINF;
            prev[ridx] = v;
            beta[((int64_t)T * nb) * W + ridx] = v;
            if (merge) {
                prev[W + ridx] = v;
                beta[((int64_t)T * nb + 1) * W + ridx] = v;
            }
        }
        __syncthreads();
        QRow r = row_of(T - 1);
        double ye[4], yb;
        load_y(T - 1, ye, yb);
        for (int u = T - 1; u >= 0; --u) {
            QRow rm = r;
            double yem[4] = {NINF, NINF, NINF, NINF}, ybm = NINF;
            if (u > 0) {
                rm = row_of(u - 1);
                load_y(u - 1, yem, ybm);
            }
            for (int ridx = lane; ridx < W; ridx += 64) {
                const int k = k_of(ridx, r);
                double vB = NINF, vX = NINF;
                if (adm(k, r)) {
                    const int pk = pack_of(ridx, k);
                    const int c0 = (pk >> 8) & 15, c1 = (pk >> 4) & 15;   // s[k], s[k-1]
                    const int ru = up(ridx);
                    const bool same = k_of(ridx, rn) == k, right = k_of(ru, rn) == k + 1 && k < L;
                    if (!merge) {
                        const double stay = same ? prev[ridx] + yb : NINF;
                        const double emit = right ? prev[ru] + ysel(ye, c0) : NINF;
                        vB = q_lae(stay, emit);
                    } else {
                        const double toB = same ? prev[ridx] + yb : NINF;
                        const double nxt = right ? prev[W + ru] + ysel(ye, c0) : NINF;
                        if (k > 0 || u == 0) vB = q_lae(toB, nxt);
                        if (k > 0) {
                            const double rep = same ? prev[W + ridx] + ysel(ye, c1) : NINF;
                            const bool dif = k < L && c0 != c1;
                            vX = q_lae(q_lae(toB, rep), dif ? nxt : NINF);
                        }
                    }
                }
                cur[ridx] = vB;
                beta[((int64_t)u * nb) * W + ridx] = vB;
                if (merge) {
                    cur[W + ridx] = vX;
                    beta[((int64_t)u * nb + 1) * W + ridx] = vX;
                }
            }
            __syncthreads();
            double* tmp = prev; prev = cur; cur = tmp;
            rn = r;
            r = rm;
#pragma unroll
            for (int b = 0; b < 4; ++b) ye[b] = yem[b];
            yb = ybm;
        }
    }
    // F = beta(0, 0), if row 0 holds state 0
    const QRow rz = row_of(0);
    double F = NINF;
    {
        int x = -rz.base;   // state 0's offset in the window
        if (x >= 0 && x < W) {
            int ridx = rz.bm + x;
            ridx -= ridx >= W ? W : 0;
            F = beta[ridx];   // written by this block before the last barrier
        }
    }
    if (!(F > NINF)) {
        if (lane == 0) { a.status[i] = PO_E_ENVELOPE; a.logp[i] = NINF; }
        return;
    }
    if (lane == 0) { a.status[i] = PO_OK; a.logp[i] = F; }

    // ---- pass 2: forward, joins ----
    auto flush = [&](int ridx, int p) {   // position p's accumulators leave index ridx
        if (p < 0 || p >= L) return;
        const int own = code_at(p);
#pragma unroll
        for (int b = 0; b < 4; ++b) odds[(int64_t)p * 5 + b] = (b == own) ? 0.0 : (b < A ? acc[b * W + ridx] - F : NINF);
        odds[(int64_t)p * 5 + 4] = acc[4 * W + ridx] - F;
    };
    double* prev = buf0;   // row t
    double* cur = buf1;    // row t + 1
    QRow rp = rz;
    for (int ridx = lane; ridx < W; ridx += 64) {
        const int k = k_of(ridx, rp);
        prev[ridx] = k == 0 ? 0.0 : NINF;
        if (merge) prev[W + ridx] = NINF;
#pragma unroll
        for (int b = 0; b < 5; ++b) acc[b * W + ridx] = NINF;
        if (merge)
#pragma unroll
            for (int b = 0; b < 4; ++b) run[b * W + ridx] = NINF;
    }
    __syncthreads();
    QRow rn = row_of(1);
    double ye[4], yb;
    load_y(0, ye, yb);
    const int lane_up = up(lane < W ? lane : 0);
    double pf_own = NINF, pf_nb = NINF;   // row t + 1 at ring index lane, and its upper neighbour's (merge: label state)
    if (lane < W) {
        pf_own = beta[((int64_t)1 * nb) * W + lane];
        pf_nb = beta[((int64_t)1 * nb + nbx) * W + lane_up];
    }
    for (int t = 0; t < T; ++t) {
        QRow rnn = rn;
        double yen[4] = {NINF, NINF, NINF, NINF}, ybn = NINF, nx_own = NINF, nx_nb = NINF;
        if (t + 1 < T) {
            rnn = row_of(t + 2);
            load_y(t + 1, yen, ybn);
            if (lane < W) {
                nx_own = beta[((int64_t)(t + 2) * nb) * W + lane];
                nx_nb = beta[((int64_t)(t + 2) * nb + nbx) * W + lane_up];
            }
        }
        const double* bn = beta + ((int64_t)(t + 1) * nb) * W;   // row t + 1
        for (int ridx = lane; ridx < W; ridx += 64) {
            const bool first = ridx == lane;
            const int kn = k_of(ridx, rn), ko = k_of(ridx, rp);
            const int rl = down(ridx), ru = up(ridx);
            const bool same = ko == kn, left = k_of(rl, rp) == kn - 1, right = k_of(ru, rn) == kn + 1;
            if (!same) {
                flush(ridx, ko - 1);
#pragma unroll
                for (int b = 0; b < 5; ++b) acc[b * W + ridx] = NINF;
                if (merge)
#pragma unroll
                    for (int b = 0; b < 4; ++b) run[b * W + ridx] = NINF;
            }
            const int p = kn - 1;
            const bool here = adm(kn, rn);
            const bool pos = p >= 0 && p < L;
            const int pk = pos ? pack_of(ridx, kn) : 0xfff;
            const int c0 = (pk >> 8) & 15, c2 = pk & 15;
            const int cn = c0 == 15 ? -1 : c0;         // s[p+1]
            const int cq = c2 == 15 ? -1 : c2;         // s[p-1]
            const int cs = pos ? ((pk >> 4) & 15) : 0;   // s[p] = the base that enters state kn
            const double b_own = first ? pf_own : (pos ? bn[ridx] : NINF);
            const double b_nb = first ? pf_nb : ((pos && right) ? bn[nbx * W + ru] : NINF);
            double nB = NINF, nX = NINF;
            if (!merge) {
                const double a_same = same ? prev[ridx] : NINF;
                const double a_left = left ? prev[rl] : NINF;
                if (pos && a_left > NINF) {
                    const double gsub = a_left + b_own;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (b < A) acc[b * W + ridx] = q_lae(acc[b * W + ridx], gsub + ye[b]);
                    if (cn >= 0 && right) acc[4 * W + ridx] = q_lae(acc[4 * W + ridx], a_left + ysel(ye, cn) + b_nb);
                }
                if (here) nB = q_lae(a_same + yb, pos ? a_left + ysel(ye, cs) : NINF);
            } else {
                const double aB_same = same ? prev[ridx] : NINF, aX_same = same ? prev[W + ridx] : NINF;
                const double aB_left = left ? prev[rl] : NINF, aX_left = left ? prev[W + rl] : NINF;
                if (pos) {
                    const double bXr = right ? b_nb : NINF;
                    const double Pb = yb + b_own;
                    const double Qn = cn >= 0 ? ysel(ye, cn) + bXr : NINF;
                    const double PQ = q_lae(Pb, Qn);
                    const double e0 = aB_left, e1 = q_lae(aB_left, aX_left);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (b >= A) continue;
                        const double r = run[b * W + ridx];
                        if (r > NINF) acc[b * W + ridx] = q_lae(acc[b * W + ridx], r + (b == cn ? Pb : PQ));
                        run[b * W + ridx] = here ? q_lae(r, b == cq ? e0 : e1) + ye[b] : NINF;
                    }
                    if (cn >= 0) acc[4 * W + ridx] = q_lae(acc[4 * W + ridx], (cq == cn ? e0 : e1) + ysel(ye, cn) + bXr);
                }
                if (here) {
                    // the blank state of position 0 exists in row 0 only (the tree's root)
                    if (kn > 0) nB = q_lae(aB_same, aX_same) + yb;
                    if (pos) nX = q_lae(q_lae(aX_same, aB_left), (cq >= 0 && cq != cs) ? aX_left : NINF) + ysel(ye, cs);
                }
            }
            cur[ridx] = nB;
            if (merge) cur[W + ridx] = nX;
        }
        __syncthreads();
        double* tmp = prev; prev = cur; cur = tmp;
        rp = rn;
        rn = rnn;
#pragma unroll
        for (int b = 0; b < 4; ++b) ye[b] = yen[b];
        yb = ybn;
        pf_own = nx_own;
        pf_nb = nx_nb;
    }
    // row T: the substitution run and the deletion of the last position end with the read
    for (int ridx = lane; ridx < W; ridx += 64) {
        const int k = k_of(ridx, rp);
        const int p = k - 1;
        if (p == L - 1) {
            const int rl = down(ridx);
            const bool left = k_of(rl, rp) == p;
            if (!merge) {
                acc[4 * W + ridx] = left ? prev[rl] : NINF;
            } else {
                acc[4 * W + ridx] = left ? q_lae(prev[rl], prev[W + rl]) : NINF;
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b * W + ridx] = q_lae(acc[b * W + ridx], run[b * W + ridx]);
            }
        }
        flush(ridx, p);
    }
}

// ---- qual_reg_kernel: qual_kernel's lattice for a ring of at most 64 indices, the state in registers.
// Lane = ring index.  The row of pass 1, prev / cur of pass 2, the five accumulators and the merge model's four runs are
// registers of the lane; the upper and the lower neighbour's values come from a lane read (__shfl) whose index is formed
// mod W.  No LDS, no barrier.  The stored rows keep qual_kernel's layout.  Every cell's operands enter the same q_lae calls
// in the same order as in qual_kernel; where qual_kernel branches around a term, the term is computed and selected away
// (q_lae(x, -inf) is x, bit for bit), so odds, logp and status are qual_kernel's bits.  The guide value is requested two
// steps ahead, the y row, the label codes around the lane's state and the stored row one step ahead, all of them
// unconditionally (clamped addresses): no load waits under a branch inside a frame loop.
template <bool MERGE>
__global__ __launch_bounds__(64) void qual_reg_kernel(QArgs a) {
    const int lane = threadIdx.x;
    const QDesc d = a.desc[a.first + blockIdx.x];
    const int i = d.read;
    const int A = a.A, C = A + 1, B = a.band;
    const int W = d.wr;   // <= 64
    const bool full = d.full != 0;
    const int64_t r0 = a.y_off[i];
    const int T = (int)(a.y_off[i + 1] - r0);
    const double* y = a.y + r0 * C;
    const char* lab = a.labels + a.label_off[i];
    const int L = (int)(a.label_off[i + 1] - a.label_off[i]);
    const int32_t* g = a.guide ? a.guide + r0 : nullptr;
    double* odds = a.odds + a.label_off[i] * 5;
    const double NINF = q_ninf();

    // ---- arguments: label characters, guide (qual_kernel's) ----
    int bad = 0;
    for (int j = lane; j < L; j += 64) bad |= (q_code(a.alphabet, A, lab[j]) < 0);
    if (g)
        for (int t = lane; t < T; t += 64) {
            const int c = g[t], p = t > 0 ? g[t - 1] : 0;
            bad |= (c < 0) | (c > L) | (c < p);
        }
    bad = __ballot(bad) != 0ull;
    for (int64_t j = lane; j < (int64_t)L * 5; j += 64) odds[j] = 0.0;
    if (bad || L == 0 || T <= 0) {
        if (lane == 0) {
            double bs = 0.0;
            if (!bad && L == 0)
                for (int t = 0; t < T; ++t) bs = bs + y[(int64_t)t * C + A];
            const bool ok = !bad && L == 0;
            a.status[i] = bad ? PO_E_ARG : (ok ? PO_OK : PO_E_ENVELOPE);
            a.logp[i] = ok ? bs : NINF;
        }
        return;
    }

    const bool act = lane < W;
    const int ridx = act ? lane : 0;
    const int ru = ridx + 1 == W ? 0 : ridx + 1, rl = ridx == 0 ? W - 1 : ridx - 1;
    // the band centre of row u = 0 .. T (rows outside are clamped: a prefetch for a step that does not come)
    auto centre = [&](int u) -> int {
        int t = u > 0 ? u - 1 : 0;
        t = t < T ? t : T - 1;
        return g ? g[t] : (int)(((int64_t)(t + 1) * L) / T);
    };
    auto row_at = [&](int u, int c) -> QRow {
        QRow r;
        r.base = full ? 0 : c - B - 1;
        int bm = r.base % W;
        r.bm = bm < 0 ? bm + W : bm;
        r.lo = B >= 1 ? max(0, c - B) : 0;
        r.hi = B >= 1 ? min(L, c + B) : L;
        if (u == 0) r.lo = r.hi = 0;
        return r;
    };
    auto k_of = [&](int rx, const QRow& r) -> int { int x = rx - r.bm; x += (x < 0) ? W : 0; return r.base + x; };
    auto adm = [&](int k, const QRow& r) -> bool { return k >= r.lo && k <= r.hi; };
    // s[k-2] | s[k-1] << 4 | s[k] << 8 (15: there is none), qual_kernel's pack_of without its cache: three byte loads
    auto pack_at = [&](int k) -> int {
        int v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = k - 2 + j;
            const bool in = q >= 0 && q < L;
            const int c = q_code(a.alphabet, A, lab[in ? q : 0]) & 3;
            v |= (in ? c : 15) << (4 * j);
        }
        return v;
    };
    auto load_y = [&](int t, double (&ye)[4], double& yb) {
        t = t < 0 ? 0 : (t < T ? t : T - 1);
        const double* yr = y + (int64_t)t * C;
#pragma unroll
        for (int b = 0; b < 4; ++b) ye[b] = b < A ? yr[b] : NINF;
        yb = yr[A];
    };
    auto ysel = [&](const double (&ye)[4], int c) -> double { return c == 0 ? ye[0] : (c == 1 ? ye[1] : (c == 2 ? ye[2] : ye[3])); };

    constexpr int nb = MERGE ? 2 : 1, nbx = nb - 1;
    double* beta = a.beta + d.beta_off;          // row u: beta[(u * nb + which) * W + ridx]

    // ---- pass 1: backward ----
    double pB, pX = NINF;   // row u + 1 at this lane's ring index
    {
        QRow rn = row_at(T, centre(T));
        {
            const int k = k_of(ridx, rn);
            pB = (k == L && adm(k, rn)) ? 0.0 : NINF;
            if (MERGE) pX = pB;
            if (act) {
                beta[((int64_t)T * nb) * W + ridx] = pB;
                if (MERGE) beta[((int64_t)T * nb + 1) * W + ridx] = pB;
            }
        }
        QRow r = row_at(T - 1, centre(T - 1));
        int cm = centre(T - 2);            // the centre of row u - 1, a step before its row is made
        int pk = pack_at(k_of(ridx, r));
        double ye[4], yb;
        load_y(T - 1, ye, yb);
        for (int u = T - 1; u >= 0; --u) {
            const QRow rm = row_at(u - 1 > 0 ? u - 1 : 0, cm);   // (u == 0: not used)
            const int cmm = centre(u - 2 > 0 ? u - 2 : 0);
            const int pkm = pack_at(k_of(ridx, rm));
            double yem[4], ybm;
            load_y(u - 1, yem, ybm);
            const int k = k_of(ridx, r);
            const bool in = adm(k, r);
            const int c0 = (pk >> 8) & 15, c1 = (pk >> 4) & 15;   // s[k], s[k-1]
            const bool same = k_of(ridx, rn) == k, right = k_of(ru, rn) == k + 1 && k < L;
            const double upB = __shfl(pB, ru);
            double vB = NINF, vX = NINF;
            if (!MERGE) {
                const double stay = same ? pB + yb : NINF;
                const double emit = right ? upB + ysel(ye, c0) : NINF;
                const double v = q_lae(stay, emit);
                vB = in ? v : NINF;
            } else {
                const double upX = __shfl(pX, ru);
                const double toB = same ? pB + yb : NINF;
                const double nxt = right ? upX + ysel(ye, c0) : NINF;
                const double v = q_lae(toB, nxt);
                vB = (in && (k > 0 || u == 0)) ? v : NINF;
                const double rep = same ? pX + ysel(ye, c1) : NINF;
                const bool dif = k < L && c0 != c1;
                const double x = q_lae(q_lae(toB, rep), dif ? nxt : NINF);
                vX = (in && k > 0) ? x : NINF;
            }
            if (act) {
                beta[((int64_t)u * nb) * W + ridx] = vB;
                if (MERGE) beta[((int64_t)u * nb + 1) * W + ridx] = vX;
            }
            pB = vB;
            pX = vX;
            rn = r;
            r = rm;
            cm = cmm;
            pk = pkm;
#pragma unroll
            for (int b = 0; b < 4; ++b) ye[b] = yem[b];
            yb = ybm;
        }
    }
    __syncthreads();   // the stored rows are read back by other lanes than wrote them: once, between the passes
    // F = beta(0, 0), if row 0 holds state 0 (pB is row 0 now)
    const QRow rz = row_at(0, centre(0));
    double F = NINF;
    {
        const int x = -rz.base;   // state 0's offset in the window
        int rx = rz.bm + (x >= 0 && x < W ? x : 0);
        rx -= rx >= W ? W : 0;
        const double f = __shfl(pB, rx);
        if (x >= 0 && x < W) F = f;
    }
    if (!(F > NINF)) {
        if (lane == 0) { a.status[i] = PO_E_ENVELOPE; a.logp[i] = NINF; }
        return;
    }
    if (lane == 0) { a.status[i] = PO_OK; a.logp[i] = F; }

    // ---- pass 2: forward, joins ----
    double acc[5], run[4];
    auto flush = [&](int p) {   // position p's accumulators leave this lane
        if (!act || p < 0 || p >= L) return;
        const int own = q_code(a.alphabet, A, lab[p]) & 3;
#pragma unroll
        for (int b = 0; b < 4; ++b) odds[(int64_t)p * 5 + b] = (b == own) ? 0.0 : (b < A ? acc[b] - F : NINF);
        odds[(int64_t)p * 5 + 4] = acc[4] - F;
    };
    QRow rp = rz;
    double aB = k_of(ridx, rp) == 0 ? 0.0 : NINF, aX = NINF;   // row t at this lane's ring index
#pragma unroll
    for (int b = 0; b < 5; ++b) acc[b] = NINF;
#pragma unroll
    for (int b = 0; b < 4; ++b) run[b] = NINF;
    QRow rn = row_at(1, centre(1));
    int cnn = centre(2);                 // the centre of row t + 2, a step before its row is made
    int pk = pack_at(k_of(ridx, rn));
    double ye[4], yb;
    load_y(0, ye, yb);
    double pf_own = beta[((int64_t)1 * nb) * W + ridx];          // row t + 1 at this ring index, and its upper neighbour's
    double pf_nb = beta[((int64_t)1 * nb + nbx) * W + ru];      // (merge: label state)
    for (int t = 0; t < T; ++t) {
        const int un = t + 2 < T ? t + 2 : T;                     // (the last step: row T again, not used)
        const QRow rnn = row_at(un, cnn);
        const int cnnn = centre(t + 3);
        const int pkn = pack_at(k_of(ridx, rnn));
        double yen[4], ybn;
        load_y(t + 1, yen, ybn);
        const double nx_own = beta[((int64_t)un * nb) * W + ridx];
        const double nx_nb = beta[((int64_t)un * nb + nbx) * W + ru];
        const int kn = k_of(ridx, rn), ko = k_of(ridx, rp);
        const bool same = ko == kn, left = k_of(rl, rp) == kn - 1, right = k_of(ru, rn) == kn + 1;
        if (!same) {
            flush(ko - 1);
#pragma unroll
            for (int b = 0; b < 5; ++b) acc[b] = NINF;
#pragma unroll
            for (int b = 0; b < 4; ++b) run[b] = NINF;
        }
        const int p = kn - 1;
        const bool here = adm(kn, rn);
        const bool pos = p >= 0 && p < L;
        const int pq = pos ? pk : 0xfff;
        const int c0 = (pq >> 8) & 15, c2 = pq & 15;
        const int cn = c0 == 15 ? -1 : c0;         // s[p+1]
        const int cq = c2 == 15 ? -1 : c2;         // s[p-1]
        const int cs = pos ? ((pq >> 4) & 15) : 0;   // s[p] = the base that enters state kn
        const double b_own = pf_own, b_nb = pf_nb;
        const double lB = __shfl(aB, rl);
        double nB = NINF, nX = NINF;
        if (!MERGE) {
            const double a_same = same ? aB : NINF;
            const double a_left = left ? lB : NINF;
            const bool add = pos && a_left > NINF;
            const double gsub = a_left + b_own;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double v = q_lae(acc[b], gsub + ye[b]);
                acc[b] = (add && b < A) ? v : acc[b];
            }
            const double dv = q_lae(acc[4], a_left + ysel(ye, cn) + b_nb);
            acc[4] = (add && cn >= 0 && right) ? dv : acc[4];
            const double v = q_lae(a_same + yb, pos ? a_left + ysel(ye, cs) : NINF);
            nB = here ? v : NINF;
        } else {
            const double lX = __shfl(aX, rl);
            const double aB_same = same ? aB : NINF, aX_same = same ? aX : NINF;
            const double aB_left = left ? lB : NINF, aX_left = left ? lX : NINF;
            const double bXr = right ? b_nb : NINF;
            const double Pb = yb + b_own;
            const double Qn = cn >= 0 ? ysel(ye, cn) + bXr : NINF;
            const double PQ = q_lae(Pb, Qn);
            const double e0 = aB_left, e1 = q_lae(aB_left, aX_left);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double r = run[b];
                const double v = q_lae(acc[b], r + (b == cn ? Pb : PQ));
                acc[b] = (pos && b < A && r > NINF) ? v : acc[b];
                const double w = q_lae(r, b == cq ? e0 : e1) + ye[b];
                run[b] = (pos && b < A) ? (here ? w : NINF) : r;
            }
            const double dv = q_lae(acc[4], (cq == cn ? e0 : e1) + ysel(ye, cn) + bXr);
            acc[4] = (pos && cn >= 0) ? dv : acc[4];
            // the blank state of position 0 exists in row 0 only (the tree's root)
            const double vb = q_lae(aB_same, aX_same) + yb;
            nB = (here && kn > 0) ? vb : NINF;
            const double vx = q_lae(q_lae(aX_same, aB_left), (cq >= 0 && cq != cs) ? aX_left : NINF) + ysel(ye, cs);
            nX = (here && pos) ? vx : NINF;
        }
        aB = nB;
        aX = nX;
        rp = rn;
        rn = rnn;
        cnn = cnnn;
        pk = pkn;
#pragma unroll
        for (int b = 0; b < 4; ++b) ye[b] = yen[b];
        yb = ybn;
        pf_own = nx_own;
        pf_nb = nx_nb;
    }
    // row T: the substitution run and the deletion of the last position end with the read
    {
        const int k = k_of(ridx, rp);
        const int p = k - 1;
        const bool left = k_of(rl, rp) == p;
        const double lB = __shfl(aB, rl);
        const double lX = MERGE ? __shfl(aX, rl) : NINF;
        if (p == L - 1) {
            if (!MERGE) {
                acc[4] = left ? lB : NINF;
            } else {
                acc[4] = left ? q_lae(lB, lX) : NINF;
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b] = q_lae(acc[b], run[b]);
            }
        }
        flush(p);
    }
}

// ------------------------------------------------------------------------------------------------------------ host
namespace {

inline int q_per_state(int model) { return model == PO_MODEL_MERGE ? 14 : 8; }   // doubles of state per ring index (the last: two ints)
inline int q_nb(int model) { return model == PO_MODEL_MERGE ? 2 : 1; }

// ring width of one read: the band's window, or the whole state axis when that is no larger
inline int64_t q_ring(int64_t L, int band, int32_t* full) {
    const int64_t wb = band >= 1 ? 2 * (int64_t)band + 2 : L + 2;
    if (band < 1 || wb >= L + 1) { *full = 1; return L + 1; }
    *full = 0;
    return wb;
}

}  // namespace

extern "C" {

size_t po_qual_workspace_bytes(int n, int64_t total_rows, int64_t max_rows, int64_t total_labels, int band_size, int model) {
    if (n < 0 || total_rows < 0 || max_rows < 0 || total_labels < 0) return 0;
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return 0;
    // sum over the reads of (T + 1) * W with W <= L + 1 and, with a band, W <= 2B + 2
    double cells = ((double)max_rows + 1.0) * ((double)total_labels + (double)n);
    if (band_size >= 1) cells = std::min(cells, ((double)total_rows + (double)n) * (2.0 * band_size + 2.0));
    const double beta = cells * q_nb(model) * 8.0;
    const double st = ((double)total_labels + (double)n) * q_per_state(model) * 8.0;
    return al256((size_t)beta + 8) + al256((size_t)st + 8) + al256(sizeof(QDesc) * (size_t)n) + 256;
}

// which route the entries on resident tables (po_fastq_tables, po_pair_qual) pass: process-wide like po_set_align_route.
// PO_QUAL_ROUTE_AUTO is the default; PO_QUAL_ROUTE_REG is for the tests and the bench
static std::atomic<int> g_qual_route{PO_QUAL_ROUTE_AUTO};
static std::atomic<long long> g_qual_reg_reads{0};
int po_set_qual_route(int route) {
    if (route != PO_QUAL_ROUTE_GENERAL && route != PO_QUAL_ROUTE_AUTO && route != PO_QUAL_ROUTE_REG)
        return po_fail(PO_E_ARG, "po_set_qual_route: route " + std::to_string(route));
    g_qual_route.store(route);
    return PO_OK;
}
int po_qual_entry_route() { return g_qual_route.load(); }
long long po_debug_qual_reg_reads(int reset) {
    return reset ? g_qual_reg_reads.exchange(0) : g_qual_reg_reads.load();
}

int po_qual_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int model, const char* labels,
                  const int64_t* label_off, const int32_t* guide, int band_size, double* odds, double* logp,
                  int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    return po_qual_batch_route(y, y_off, n, C, alphabet, model, labels, label_off, guide, band_size, odds, logp, status, ws, ws_bytes,
                               stream, PO_QUAL_ROUTE_GENERAL);
}

// po_qual_batch with the choice of kernel.  PO_QUAL_ROUTE_GENERAL launches what po_qual_batch always launched, and so does
// PO_QUAL_ROUTE_AUTO: no instantiation of qual_reg_kernel is on the automatic route (both read spilled scalar
// registers back inside their frame loops).  PO_QUAL_ROUTE_REG sends the reads whose ring holds at most 64 indices to it
int po_qual_batch_route(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int model, const char* labels,
                        const int64_t* label_off, const int32_t* guide, int band_size, double* odds, double* logp,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream, int route) {
    po_set_error("");
    if (model == PO_MODEL_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, "po_qual_batch: the flip-flop model has no quality lattice");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, "po_qual_batch: unknown model");
    if (n < 0 || !y_off || !label_off || (n > 0 && (!y || !labels || !odds || !logp || !status || !ws)))
        return po_fail(PO_E_ARG, "po_qual_batch: null argument");
    const char* alpha = alphabet ? alphabet : "ACGT";
    const size_t A = std::strlen(alpha);
    if (A < 1 || A > 4) return po_fail(PO_E_ARG, "po_qual_batch: alphabet must have 1..4 symbols");
    if (C != (int)A + 1) return po_fail(PO_E_ARG, "po_qual_batch: C must be len(alphabet) + 1");
    if (n == 0) return PO_OK;
    hipStream_t s = (hipStream_t)stream;
    QArgs a = {};
    a.y = y; a.y_off = y_off; a.n = n; a.A = (int)A; a.merge = model == PO_MODEL_MERGE; a.labels = labels;
    a.label_off = label_off; a.guide = guide; a.band = std::max(0, std::min(band_size, 1 << 29));
    a.odds = odds; a.logp = logp; a.status = status;
    for (size_t i = 0; i < A; ++i) a.alphabet |= (uint32_t)(unsigned char)alpha[i] << (8 * i);

    std::vector<int64_t> h(2 * (size_t)(n + 1));
    PO_HIPCHK(po_read_tables(y_off, label_off, n, s, h.data()));
    std::vector<QDesc> desc((size_t)n);
    const int per = q_per_state(model), nb = q_nb(model);
    // launch classes: state in LDS of at most 4, 16, 48 KiB, state in the workspace — a read's dynamic LDS is its class's
    // largest, so one wide read does not take the occupancy of the narrow ones launched with it
    // (and, on PO_QUAL_ROUTE_REG, a fifth behind them: a ring of at most 64 indices, state in registers, no LDS)
    constexpr int NCLS = 4, REG = NCLS;
    const int64_t cls_cap[NCLS - 1] = {512, 2048, QL_LDS_MAX};
    int64_t nbeta = 0, nst = 0, lds[NCLS] = {0, 0, 0, 0};
    std::vector<int> cls((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int64_t T = h[i + 1] - h[i], L = h[n + 1 + i + 1] - h[n + 1 + i];
        if (T < 0 || L < 0 || T >= ((int64_t)1 << 31) - 1 || L >= ((int64_t)1 << 26))
            return po_fail(PO_E_ARG, "po_qual_batch: offsets must not decrease, reads must be shorter than 2^31 - 1 frames and 2^26 bases");
        QDesc& d = desc[i];
        const int64_t w = q_ring(L, a.band, &d.full);
        d.wr = (int32_t)w;
        d.beta_off = nbeta;
        nbeta += (T + 1) * w * nb;
        d.read = i;
        d.pad = 0;
        if (route == PO_QUAL_ROUTE_REG && w <= 64) {
            d.st_off = -1;
            cls[i] = REG;
        } else if (w * per <= QL_LDS_MAX) {
            d.st_off = -1;
            int c = 0;
            while (w * per > cls_cap[c]) ++c;
            cls[i] = c;
            lds[c] = std::max(lds[c], w * per);
        } else {
            d.st_off = nst;
            nst += w * per;
            cls[i] = NCLS - 1;
        }
    }
    std::vector<QDesc> sorted;
    sorted.reserve((size_t)n);
    int first[NCLS + 2] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c <= NCLS; ++c) {
        for (int i = 0; i < n; ++i)
            if (cls[i] == c) sorted.push_back(desc[i]);
        first[c + 1] = (int)sorted.size();
    }
    const size_t b_beta = al256((size_t)nbeta * 8 + 8), b_st = al256((size_t)nst * 8 + 8), b_desc = al256(sizeof(QDesc) * (size_t)n);
    if (ws_bytes < b_beta + b_st + b_desc) return po_fail(PO_E_CAP, "po_qual_batch: workspace too small");
    a.beta = (double*)ws;
    a.st = (double*)((char*)ws + b_beta);
    a.desc = (const QDesc*)((char*)ws + b_beta + b_st);
    PO_HIPCHK(hipMemcpyAsync((void*)a.desc, sorted.data(), sizeof(QDesc) * (size_t)n, hipMemcpyHostToDevice, s));
    PO_HIPCHK(hipStreamSynchronize(s));   // the table lives on this stack
    for (int c = 0; c < NCLS; ++c) {
        if (first[c + 1] == first[c]) continue;
        a.first = first[c];
        hipLaunchKernelGGL(qual_kernel, dim3(first[c + 1] - first[c]), dim3(64), (size_t)lds[c] * 8, s, a);
    }
    if (first[REG + 1] > first[REG]) {
        g_qual_reg_reads += first[REG + 1] - first[REG];
        a.first = first[REG];
        if (a.merge) hipLaunchKernelGGL(qual_reg_kernel<true>, dim3(first[REG + 1] - first[REG]), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(qual_reg_kernel<false>, dim3(first[REG + 1] - first[REG]), dim3(64), 0, s, a);
    }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

int po_qual_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int model,
                    const char* labels_h, const int64_t* label_off_h, const int32_t* guide_h, int band_size, double* odds_h,
                    double* logp_h, int32_t* status_h) {
    po_set_error("");
    if (model == PO_MODEL_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, "po_qual_batch_h: the flip-flop model has no quality lattice");
    if (model != PO_MODEL_CTC && model != PO_MODEL_MERGE) return po_fail(PO_E_ARG, "po_qual_batch_h: unknown model");
    if (n <= 0) return n < 0 ? po_fail(PO_E_ARG, "po_qual_batch_h: negative n") : PO_OK;
    if (!y_off_h || !label_off_h || !logp_h || !status_h) return po_fail(PO_E_ARG, "po_qual_batch_h: null argument");
    const PoRagged r(y_off_h, n, true), l(label_off_h, n, true);
    if (!r.ordered || !l.ordered) return po_fail(PO_E_ARG, "po_qual_batch_h: offsets must not decrease");
    if ((r.total > 0 && !y_h) || (l.total > 0 && (!labels_h || !odds_h))) return po_fail(PO_E_ARG, "po_qual_batch_h: null argument");
    PoRows y, lb;
    PoDev gd, od, lp, st, ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(lb.up(labels_h, l, 1));
    if (guide_h) PO_HIPCHK(gd.up(guide_h + r.base, sizeof(int32_t) * r.total));   // one state per frame, at the read's rows
    PO_HIPCHK(od.up(nullptr, sizeof(double) * 5 * l.total));
    PO_HIPCHK(lp.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_qual_workspace_bytes(n, r.total, r.max, l.total, band_size, model);
    PO_HIPCHK(ws.up(nullptr, wsb));
    const int rc = po_qual_batch(y.data, y.off, n, C, alphabet, model, lb.data, lb.off, gd, band_size, od, lp, st, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(od.down(odds_h + l.base * 5, sizeof(double) * 5 * l.total));   // five odds per base, at the label's place in the caller's table
    PO_HIPCHK(lp.down(logp_h, sizeof(double) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

}  // extern "C"
