// po_map.hip — the read mapper behind `benchmark`: minimap2's map-ont seeds and scores reduced to a
// fixed, fully ordered integer specification, so that the CPU restatement (tests/_map_oracle.py) and this file agree
// bit for bit.  Every per-read stage runs here:
//   sketch   map_hash_kernel (code + hash per position), map_minflag_kernel (the window-minimum test), a count -> scan ->
//            write emit, so minimizers come out in position order without appending atomics;
//   anchors  map_anchor_count_kernel (lower/upper bound on the sorted 30-bit hashes), scan, map_anchor_write_kernel;
//   sort     map_sort_kernel: one workgroup per read, bitonic on the unique key (2c + rev, x, y), in LDS up to 2048
//            anchors and in a global scratch slice beyond;
//   chain    map_chain_kernel: one wave per read; the 64 predecessors are the 64 lanes (a register ring shifted by one
//            lane per anchor), each step one wave max-reduce in which the nearest predecessor wins ties;
//   align    map_align_kernel: one wave per read, 8 band columns per lane, the previous row's H and F in LDS (ping-pong,
//            one barrier per row), E as an exclusive prefix maximum of max(0, diag, F) + 2c across the row (exact in any
//            order: a cell whose H came from E never opens a better gap), 4 trace-back bits per cell = one dword per lane
//            per row, 256 B per row stored coalesced;
//   trace    map_trace_kernel: one thread per read walks the bits back from the best cell and writes one op byte per
//            alignment column.
// No float arithmetic, no float atomics, no hand-off between workgroups.  Reads go in batches under a device-memory
// budget, longest first; a read too large for the budget runs in a batch of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"
#include "po_hostbuf.h"

#include "po_internal.h"

namespace {

constexpr int MK = 15, MW = 10;
constexpr int BAND = 512, MAX_GAP = 5000, MAX_DD = 500, MIN_CNT = 3, MIN_SCORE = 40;
constexpr int SC_MATCH = 2, SC_MISMATCH = -4, SC_AMBIG = -1, GAP_O = 4, GAP_E = 2;
constexpr uint32_t NOKMER = 0xffffffffu;
constexpr int NEG = -(1 << 30);
constexpr int SORT_LDS = 2048;
constexpr int TPB = 256;
constexpr int TILE = 4 * TPB;
// device bytes per read base in a batch (sequence, hashes, strands, flags, scans, minimizers, band starts, 64 trace-back
// dwords per row); anchors (16 B each, plus 12 B of chain state) are sized after they are counted
constexpr int64_t BYTES_PER_BASE = 1 + 4 + 1 + 4 + 8 + (4 + 4 + 1 + 4 + 4 + 8 + 8) + 4 + 256;
constexpr int64_t BYTES_PER_READ = 128;

struct Anc {
    uint64_t key;  // (2 * contig + rev) << 32 | x
    uint32_t y;
    uint32_t pad;
};

struct ChainOut {
    int32_t n_chain, score, grp, ok;
    int64_t dmin, dmax;
};

struct BestOut {
    int32_t score, y;
    int64_t j;
};

__device__ __forceinline__ uint32_t base2(unsigned char c) {
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

__device__ __forceinline__ uint64_t hash64(uint64_t key) {
    const uint64_t m = (1ull << 30) - 1;
    key = (~key + (key << 21)) & m;
    key = key ^ key >> 24;
    key = ((key + (key << 3)) + (key << 8)) & m;
    key = key ^ key >> 14;
    key = ((key + (key << 2)) + (key << 4)) & m;
    key = key ^ key >> 28;
    key = (key + (key << 31)) & m;
    return key;
}

// the sequence holding position p: the largest s < n with off[s] <= p (an empty sequence shares its offset with the next)
__device__ __forceinline__ int seq_of(const int64_t* off, int n, int64_t p) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int64_t floordiv(int64_t a, int64_t b) {  // b > 0, rounds toward -inf
    int64_t q = a / b;
    if ((a % b) != 0 && a < 0) --q;
    return q;
}

// ---------------------------------------------------------------------------------------------------- scan (int64)

// workgroup-wide exclusive scan of one value per thread; returns the exclusive prefix, *total the sum
__device__ int64_t block_excl_scan(int64_t v, int64_t* sh, int64_t* total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < TPB; o <<= 1) {
        const int64_t u = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += u;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[TPB - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(TPB) void scan_tile_sum_kernel(const uint32_t* in, int64_t n, int64_t* tsum) {
    __shared__ int64_t sh[TPB];
    const int64_t b = (int64_t)blockIdx.x * TILE + threadIdx.x * 4;
    int64_t s = 0;
    for (int e = 0; e < 4; ++e)
        if (b + e < n) s += in[b + e];
    int64_t tot;
    block_excl_scan(s, sh, &tot);
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of nt tile sums in place, the grand total into t[nt]
__global__ __launch_bounds__(TPB) void scan_tiles_kernel(int64_t* t, int64_t nt) {
    __shared__ int64_t sh[TPB];
    int64_t carry = 0;
    for (int64_t b = 0; b < nt; b += TPB) {
        const int64_t i = b + threadIdx.x;
        const int64_t v = i < nt ? t[i] : 0;
        int64_t tot;
        const int64_t ex = block_excl_scan(v, sh, &tot);
        if (i < nt) t[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) t[nt] = carry;
}

__global__ __launch_bounds__(TPB) void scan_tile_write_kernel(const uint32_t* in, int64_t n, const int64_t* toff,
                                                              int64_t nt, int64_t* out) {
    __shared__ int64_t sh[TPB];
    const int64_t b = (int64_t)blockIdx.x * TILE + threadIdx.x * 4;
    uint32_t v[4];
    int64_t s = 0;
    for (int e = 0; e < 4; ++e) {
        v[e] = b + e < n ? in[b + e] : 0u;
        s += v[e];
    }
    int64_t tot;
    int64_t run = toff[blockIdx.x] + block_excl_scan(s, sh, &tot);
    for (int e = 0; e < 4; ++e) {
        if (b + e < n) out[b + e] = run;
        run += v[e];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = toff[nt];
}

// ---------------------------------------------------------------------------------------------------- sketch

__global__ __launch_bounds__(TPB) void map_hash_kernel(const char* seq, const int64_t* off, int n, int64_t P,
                                                       uint32_t* hs, uint8_t* ss) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= P) return;
    const int s = seq_of(off, n, p);
    const int64_t i = p - off[s], len = off[s + 1] - off[s];
    uint32_t h = NOKMER;
    uint8_t st = 0;
    if (i + MK <= len) {
        uint64_t f = 0, r = 0;
        bool ok = true;
        for (int t = 0; t < MK; ++t) {
            const uint32_t c = base2((unsigned char)seq[p + t]);
            ok = ok && c < 4;
            f = (f << 2) | (c & 3u);
            r |= (uint64_t)(3u - (c & 3u)) << (2 * t);
        }
        if (ok) {
            h = (uint32_t)hash64(f < r ? f : r);
            st = f < r ? 0 : 1;
        }
    }
    hs[p] = h;
    ss[p] = st;
}

// p is a minimizer when a window of w existing k-mers of its run has p as its smallest hash (ties: smallest position),
// or when its run has fewer than w k-mers and p is the run's minimum
__global__ __launch_bounds__(TPB) void map_minflag_kernel(const int64_t* off, int n, int64_t P, const uint32_t* hs,
                                                          uint32_t* flag) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= P) return;
    const uint32_t h = hs[p];
    uint32_t out = 0;
    if (h != NOKMER) {
        const int s = seq_of(off, n, p);
        const int64_t i = p - off[s], nk = off[s + 1] - off[s] - MK + 1;
        int L = 0, R = 0;
        bool lb = false, rb = false;
        for (int d = 1; d < MW; ++d) {
            if (i - d < 0 || hs[p - d] == NOKMER) { lb = true; break; }
            if (hs[p - d] > h) ++L; else break;
        }
        for (int d = 1; d < MW; ++d) {
            if (i + d >= nk || hs[p + d] == NOKMER) { rb = true; break; }
            if (hs[p + d] >= h) ++R; else break;
        }
        out = (L + R + 1 >= MW || (lb && rb)) ? 1u : 0u;
    }
    flag[p] = out;
}

__global__ __launch_bounds__(TPB) void map_emit_kernel(const int64_t* off, int n, int64_t P, const uint32_t* hs,
                                                       const uint8_t* ss, const uint32_t* flag, const int64_t* scan,
                                                       uint32_t* mh, int32_t* mpos, uint8_t* mst, int32_t* mseq) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= P || !flag[p]) return;
    const int s = seq_of(off, n, p);
    const int64_t k = scan[p];
    mh[k] = hs[p];
    mpos[k] = (int32_t)(p - off[s]);
    mst[k] = ss[p];
    if (mseq) mseq[k] = s;
}

// per-sequence offsets into the minimizers (or anchors): out[s] = scan[idx[s]], s = 0..n
__global__ __launch_bounds__(TPB) void map_gather_off_kernel(const int64_t* idx, int n, const int64_t* scan, int64_t* out) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s <= n) out[s] = scan[idx[s]];
}

// ---------------------------------------------------------------------------------------------------- anchors

__device__ __forceinline__ int64_t bound_u32(const uint32_t* a, int64_t n, uint32_t v, bool upper) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (upper ? a[mid] <= v : a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TPB) void map_anchor_count_kernel(const uint32_t* mh, int64_t M, const uint32_t* ih,
                                                               int64_t ni, uint32_t* cnt, int64_t* lbo) {
    const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (m >= M) return;
    const int64_t lo = bound_u32(ih, ni, mh[m], false);
    const int64_t hi = bound_u32(ih, ni, mh[m], true);
    cnt[m] = (uint32_t)(hi - lo);
    lbo[m] = lo;
}

__global__ __launch_bounds__(TPB) void map_anchor_write_kernel(const int64_t* off, int64_t M, const int32_t* mpos,
                                                               const uint8_t* mst, const int32_t* mseq,
                                                               const uint32_t* cnt, const int64_t* lbo,
                                                               const int64_t* aoff, const uint32_t* ipos,
                                                               const uint32_t* ics, Anc* A) {
    const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (m >= M) return;
    const int s = mseq[m];
    const int64_t len = off[s + 1] - off[s], i = mpos[m];
    const uint32_t sq = mst[m];
    const int64_t b = aoff[m], e0 = lbo[m];
    for (uint32_t e = 0; e < cnt[m]; ++e) {
        const uint32_t cs = ics[e0 + e];
        const uint32_t rev = sq != (cs & 1u) ? 1u : 0u;
        const uint64_t x = (uint64_t)ipos[e0 + e] + MK - 1;
        Anc a;
        a.key = ((uint64_t)((cs >> 1) * 2u + rev) << 32) | x;
        a.y = (uint32_t)(rev ? len - 1 - i : i + MK - 1);
        a.pad = 0;
        A[b + e] = a;
    }
}

__device__ __forceinline__ bool anc_less(const Anc& a, const Anc& b) {
    return a.key < b.key || (a.key == b.key && a.y < b.y);
}

__global__ __launch_bounds__(TPB) void map_sort_kernel(Anc* A, const int64_t* raoff, Anc* scratch, const int64_t* soff) {
    __shared__ Anc sh[SORT_LDS];
    const int r = blockIdx.x;
    const int64_t b = raoff[r];
    const int64_t n = raoff[r + 1] - b;
    if (n <= 1) return;
    int64_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    Anc* buf = np2 <= SORT_LDS ? sh : scratch + soff[r];
    const Anc sent = {~0ull, ~0u, 0u};
    for (int64_t i = threadIdx.x; i < np2; i += TPB) buf[i] = i < n ? A[b + i] : sent;
    __syncthreads();
    for (int64_t k = 2; k <= np2; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < np2; i += TPB) {
                const int64_t ixj = i ^ j;
                if (ixj > i) {
                    const Anc a = buf[i], c = buf[ixj];
                    const bool asc = (i & k) == 0;
                    if (asc ? anc_less(c, a) : anc_less(a, c)) { buf[i] = c; buf[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int64_t i = threadIdx.x; i < n; i += TPB) A[b + i] = buf[i];
}

// ---------------------------------------------------------------------------------------------------- chain

__global__ __launch_bounds__(64) void map_chain_kernel(const Anc* A, const int64_t* raoff, int32_t* fout, int32_t* pout,
                                                       int32_t* chain, ChainOut* co) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int64_t b = raoff[r];
    const int n = (int)(raoff[r + 1] - b);
    // lane l holds anchor i - 1 - l
    long long rx = 0, ry = 0;
    unsigned rg = 0xffffffffu;
    int rf = NEG;
    int bestf = -1, besti = -1;
    for (int i = 0; i < n; ++i) {
        const Anc a = A[b + i];
        const unsigned gi = (unsigned)(a.key >> 32);
        const long long xi = (long long)(a.key & 0xffffffffull), yi = a.y;
        int cand = NEG;
        if (lane < i && rg == gi) {
            const long long dx = xi - rx, dy = yi - ry;
            if (dx <= MAX_GAP && dx != 0 && dy > 0 && dy <= MAX_GAP) {
                const long long dd = dx > dy ? dx - dy : dy - dx;
                if (dd <= MAX_DD) {
                    const int m = (int)(dx < dy ? (dx < MK ? dx : MK) : (dy < MK ? dy : MK));
                    const int pen = dd ? (int)(dd * MK / 100) + ((31 - __clz((unsigned)dd)) >> 1) : 0;
                    cand = rf + m - pen;
                }
            }
        }
        unsigned long long key = ((unsigned long long)(unsigned)(cand - NEG) << 32) | (unsigned)(63 - lane);
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long u = __shfl_xor(key, o);
            key = u > key ? u : key;
        }
        const int bc = (int)(key >> 32) + NEG;
        const int bl = 63 - (int)(key & 0xffu);
        int fi = MK, pi = -1;
        if (bc > MK) { fi = bc; pi = i - 1 - bl; }
        if (lane == 0) { fout[b + i] = fi; pout[b + i] = pi; }
        if (fi > bestf) { bestf = fi; besti = i; }
        rx = __shfl_up(rx, 1); ry = __shfl_up(ry, 1); rg = __shfl_up(rg, 1); rf = __shfl_up(rf, 1);
        if (lane == 0) { rx = xi; ry = yi; rg = gi; rf = fi; }
    }
    if (lane != 0) return;
    ChainOut c = {0, n ? bestf : 0, 0, 0, 0, 0};
    if (n) {
        int cnt = 0;
        for (int i = besti; i >= 0; i = pout[b + i]) ++cnt;
        int k = cnt;
        long long dmin = 0, dmax = 0;
        for (int i = besti; i >= 0; i = pout[b + i]) {
            chain[b + --k] = i;
            const long long d = (long long)(A[b + i].key & 0xffffffffull) - (long long)A[b + i].y;
            if (k == cnt - 1 || d < dmin) dmin = d;
            if (k == cnt - 1 || d > dmax) dmax = d;
        }
        c.n_chain = cnt;
        c.grp = (int)(A[b + besti].key >> 32);
        c.ok = cnt >= MIN_CNT && bestf >= MIN_SCORE;
        c.dmin = dmin;
        c.dmax = dmax;
    }
    co[r] = c;
}

// ---------------------------------------------------------------------------------------------------- align

__device__ __forceinline__ uint32_t qbase(const char* rd, int64_t len, int64_t y, int rev) {
    if (!rev) return base2((unsigned char)rd[y]);
    const uint32_t c = base2((unsigned char)rd[len - 1 - y]);
    return c < 4 ? 3u - c : 4u;
}

struct AlignArgs {
    const int32_t* list;
    const char* seq;
    const int64_t* off;
    const Anc* A;
    const int64_t* raoff;
    const int32_t* chain;
    const ChainOut* co;
    const char* ctg;
    const int64_t* ctg_off;
    int32_t* band_lo;
    uint32_t* tb;
    BestOut* best;
};

__global__ __launch_bounds__(64) void map_align_kernel(AlignArgs g) {
    __shared__ int Hs[2][BAND], Fs[2][BAND];
    const int r = g.list[blockIdx.x], lane = threadIdx.x;
    const int64_t pos0 = g.off[r], len = g.off[r + 1] - pos0;
    const char* rd = g.seq + pos0;
    const ChainOut co = g.co[r];
    const int c = co.grp >> 1, rev = co.grp & 1;
    const char* R = g.ctg + g.ctg_off[c];
    const int64_t rlen = g.ctg_off[c + 1] - g.ctg_off[c];
    const int32_t* ci = g.chain + g.raoff[r];
    const Anc* Ar = g.A + g.raoff[r];
    const int nch = co.n_chain;
    auto ax = [&](int t) { return (int64_t)(Ar[ci[t]].key & 0xffffffffull); };
    auto ay = [&](int t) { return (int64_t)Ar[ci[t]].y; };
    int t = 0;
    int64_t ya = ay(0), Da = ax(0) - ya, yb = 0, Db = 0;
    if (nch > 1) { yb = ay(1); Db = ax(1) - yb; }
    const int64_t y0 = ya, D0 = Da, ylast = ay(nch - 1), Dlast = ax(nch - 1) - ylast;
    const int c0 = lane * 8;
    int64_t lop = 0;
    int bH = 0, by = 0;
    int64_t bj = 0;
    for (int64_t y = 0; y < len; ++y) {
        while (t + 1 < nch && y >= yb) {
            ++t;
            ya = yb; Da = Db;
            if (t + 1 < nch) { yb = ay(t + 1); Db = ax(t + 1) - yb; }
        }
        int64_t D;
        if (y <= y0) D = D0;
        else if (y >= ylast) D = Dlast;
        else D = Da + floordiv((Db - Da) * (y - ya), yb - ya);
        const int64_t lo = y + D - BAND / 2;
        const int64_t shift = lo - lop;
        const int cur = (int)(y & 1), prv = cur ^ 1;
        const uint32_t qb = qbase(rd, len, y, rev);
        int G[8], dg[8], F[8], run = NEG, incl[8];
        uint32_t fo = 0, vmask = 0;
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            const int cc = c0 + tt;
            const int64_t j = lo + cc;
            const bool valid = j >= 0 && j < rlen;
            int Hu = 0, Fu = NEG, Hd = 0;
            if (y > 0) {
                const int64_t ip = cc + shift;
                if (ip >= 0 && ip < BAND) { Hu = Hs[prv][ip]; Fu = Fs[prv][ip]; }
                if (ip - 1 >= 0 && ip - 1 < BAND) Hd = Hs[prv][ip - 1];
            }
            const uint32_t rb = valid ? base2((unsigned char)R[j]) : 4u;
            const int s = (rb > 3 || qb > 3) ? SC_AMBIG : (rb == qb ? SC_MATCH : SC_MISMATCH);
            const int fo_ = Hu - GAP_O - GAP_E, fe_ = Fu - GAP_E;
            F[tt] = fo_ > fe_ ? fo_ : fe_;
            fo |= (fo_ >= fe_ ? 1u : 0u) << tt;
            dg[tt] = Hd + s;
            int gg = dg[tt] > 0 ? dg[tt] : 0;
            gg = gg > F[tt] ? gg : F[tt];
            G[tt] = valid ? gg : 0;
            vmask |= (valid ? 1u : 0u) << tt;
            const int v = G[tt] + 2 * cc;
            run = run > v ? run : v;
            incl[tt] = run;
        }
        // exclusive prefix maximum of the lanes' totals
        int sc = run;
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(sc, o);
            if (lane >= o) sc = sc > u ? sc : u;
        }
        int excl = __shfl_up(sc, 1);
        if (lane == 0) excl = NEG;
        int H[8], E[8];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            const int cc = c0 + tt;
            int epre = excl;
            if (tt > 0) epre = epre > incl[tt - 1] ? epre : incl[tt - 1];
            E[tt] = epre == NEG ? NEG : epre - GAP_O - 2 * cc;
            const int hh = G[tt] > E[tt] ? G[tt] : E[tt];
            H[tt] = (vmask >> tt & 1u) ? hh : 0;
        }
        int Hl = __shfl_up(H[7], 1), El = __shfl_up(E[7], 1);
        if (lane == 0) { Hl = 0; El = NEG; }
        uint32_t word = 0;
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            const int cc = c0 + tt;
            const int hl = tt ? H[tt - 1] : Hl, el = tt ? E[tt - 1] : El;
            const uint32_t eo = (hl - GAP_O - GAP_E) >= (el - GAP_E) ? 1u : 0u;
            const uint32_t src = H[tt] == 0 ? 0u : H[tt] == dg[tt] ? 1u : H[tt] == E[tt] ? 2u : 3u;
            word |= (src | eo << 2 | (fo >> tt & 1u) << 3) << (4 * tt);
            if (H[tt] > bH) { bH = H[tt]; by = (int)y; bj = lo + cc; }
            Hs[cur][cc] = H[tt];
            Fs[cur][cc] = (vmask >> tt & 1u) ? F[tt] : NEG;
        }
        g.tb[(pos0 + y) * 64 + lane] = word;
        if (lane == 0) g.band_lo[pos0 + y] = (int32_t)lo;
        lop = lo;
        __syncthreads();
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const int oH = __shfl_xor(bH, o), oy = __shfl_xor(by, o);
        const long long oj = __shfl_xor((long long)bj, o);
        if (oH > bH || (oH == bH && (oy < by || (oy == by && oj < bj)))) { bH = oH; by = oy; bj = oj; }
    }
    if (lane == 0) g.best[r] = BestOut{bH, by, bj};
}

// ---------------------------------------------------------------------------------------------------- trace-back

struct TraceArgs {
    const int32_t* list;
    int nlist;
    const char* seq;
    const int64_t* off;
    const ChainOut* co;
    const char* ctg;
    const int64_t* ctg_off;
    const int32_t* band_lo;
    const uint32_t* tb;
    const BestOut* best;
    const int64_t* opoff;
    uint8_t* ops;
    po_map_hit* hits;
};

__global__ __launch_bounds__(64) void map_trace_kernel(TraceArgs g) {
    const int li = blockIdx.x * 64 + threadIdx.x;
    if (li >= g.nlist) return;
    const int r = g.list[li];
    const int64_t pos0 = g.off[r], len = g.off[r + 1] - pos0;
    const char* rd = g.seq + pos0;
    const ChainOut co = g.co[r];
    const int c = co.grp >> 1, rev = co.grp & 1;
    const char* R = g.ctg + g.ctg_off[c];
    const BestOut bo = g.best[r];
    po_map_hit h = g.hits[r];
    h.score = bo.score;
    if (bo.score < MIN_SCORE) { g.hits[r] = h; return; }
    uint8_t* ops = g.ops + g.opoff[r];
    const int64_t cap = g.opoff[r + 1] - g.opoff[r];
    int64_t y = bo.y, j = bo.j, qs = bo.y, rs = bo.j, nops = 0;
    int state = 0;  // 0 H, 1 E, 2 F
    int cnt[4] = {0, 0, 0, 0};
    while (y >= 0 && nops < cap) {
        const int64_t cc = j - g.band_lo[pos0 + y];
        if (cc < 0 || cc >= BAND) break;
        const uint32_t nib = (g.tb[(pos0 + y) * 64 + (cc >> 3)] >> (4 * (cc & 7))) & 15u;
        if (state == 0) {
            const uint32_t src = nib & 3u;
            if (src == 0) break;
            if (src == 1) {
                const uint32_t qb = qbase(rd, len, y, rev), rb = base2((unsigned char)R[j]);
                const uint8_t op = (qb < 4 && rb < 4 && qb == rb) ? 0 : 1;
                ops[nops++] = op; ++cnt[op];
                qs = y; rs = j; --y; --j;
                continue;
            }
            state = src == 2 ? 1 : 2;
        }
        if (state == 1) {
            ops[nops++] = 3; ++cnt[3];
            state = (nib >> 2 & 1u) ? 0 : 1;
            --j;
        } else {
            ops[nops++] = 2; ++cnt[2];
            state = (nib >> 3 & 1u) ? 0 : 2;
            --y;
        }
    }
    for (int64_t a = 0, b = nops - 1; a < b; ++a, --b) { const uint8_t t = ops[a]; ops[a] = ops[b]; ops[b] = t; }
    const int64_t qe = bo.y + 1;
    h.mapped = 1;
    h.ctg = c;
    h.strand = rev ? -1 : 1;
    h.r_st = rs;
    h.r_en = bo.j + 1;
    h.q_st = (int32_t)(rev ? len - qe : qs);
    h.q_en = (int32_t)(rev ? len - qs : qe);
    h.mlen = cnt[0];
    h.blen = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    h.nm = cnt[1] + cnt[2] + cnt[3];
    h.n_ops = (int32_t)nops;
    g.hits[r] = h;
}

// ---------------------------------------------------------------------------------------------------- pairs (§14)

// One index segment per target read, built here: the key of a target minimizer is hash << 32 | pos << 1 | strand
// (pos < 2^31 is unique inside a target, so ascending keys are the (hash, pos) order of a one-contig index).
constexpr int SEG_LDS = 4096;

// one workgroup per target: bitonic sort of its keys, in LDS up to SEG_LDS and in a global scratch slice beyond
__global__ __launch_bounds__(TPB) void pairs_segsort_kernel(const uint32_t* mh, const int32_t* mpos, const uint8_t* mst,
                                                            const int64_t* tmoff, uint64_t* key, uint64_t* scratch,
                                                            const int64_t* soff) {
    __shared__ uint64_t sh[SEG_LDS];
    const int t = blockIdx.x;
    const int64_t b = tmoff[t];
    const int64_t n = tmoff[t + 1] - b;
    if (n <= 0) return;
    int64_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    uint64_t* buf = np2 <= SEG_LDS ? sh : scratch + soff[t];
    for (int64_t i = threadIdx.x; i < np2; i += TPB)
        buf[i] = i < n ? ((uint64_t)mh[b + i] << 32 | (uint64_t)(uint32_t)mpos[b + i] << 1 | (uint64_t)(mst[b + i] & 1u))
                       : ~0ull;
    __syncthreads();
    for (int64_t k = 2; k <= np2; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < np2; i += TPB) {
                const int64_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = buf[i], c = buf[ixj];
                    const bool asc = (i & k) == 0;
                    if (asc ? c < a : a < c) { buf[i] = c; buf[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int64_t i = threadIdx.x; i < n; i += TPB) key[b + i] = buf[i];
}

// first index in key[0..n) whose hash is >= h
__device__ __forceinline__ int64_t seg_bound(const uint64_t* key, int64_t n, uint64_t h) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((key[mid] >> 32) < h) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ int64_t block_max(int64_t v, int64_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (t < o && sh[t + o] > sh[t]) sh[t] = sh[t + o];
        __syncthreads();
    }
    const int64_t m = sh[0];
    __syncthreads();
    return m;
}

// one workgroup per target: the occurrence count of every distinct hash (runc, at the first entry of its run, 0
// elsewhere) and §12's max_occ over them: the count at rank min(n - 1, int((1 - 2e-4) n)) of the n ascending counts,
// found as the smallest v with at least rank + 1 counts <= v (integer counting: no order to depend on)
__global__ __launch_bounds__(TPB) void pairs_maxocc_kernel(const uint64_t* key, const int64_t* tmoff, uint32_t* runc,
                                                           int32_t* max_occ) {
    __shared__ int64_t sh[TPB];
    const int t = blockIdx.x;
    const int64_t b = tmoff[t];
    const int64_t n = tmoff[t + 1] - b;
    const uint64_t* kp = key + b;
    int64_t nd = 0, mx = 0;
    for (int64_t i = threadIdx.x; i < n; i += TPB) {
        const uint64_t h = kp[i] >> 32;
        uint32_t c = 0;
        if (i == 0 || (kp[i - 1] >> 32) != h) {
            c = (uint32_t)seg_bound(kp + i, n - i, h + 1);
            ++nd;
            mx = mx > c ? mx : (int64_t)c;
        }
        runc[b + i] = c;
    }
    int64_t tot;
    block_excl_scan(nd, sh, &tot);
    nd = tot;
    mx = block_max(mx, sh);
    int64_t q = 0;
    if (nd > 0) {
        int64_t rank = (int64_t)((1.0 - 2e-4) * (double)nd);
        if (rank > nd - 1) rank = nd - 1;
        if (rank == nd - 1) {
            q = mx;
        } else {
            // (every thread reads back only the run counts it wrote itself: the same strided walk)
            int64_t lo = 1, hi = mx;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                int64_t le = 0;
                for (int64_t i = threadIdx.x; i < n; i += TPB) {
                    const uint32_t c = runc[b + i];
                    le += (c != 0 && c <= mid) ? 1 : 0;
                }
                block_excl_scan(le, sh, &tot);
                if (tot >= rank + 1) hi = mid; else lo = mid + 1;
            }
            q = lo;
        }
    }
    if (threadIdx.x == 0) max_occ[t] = (int32_t)(q < 10 ? 10 : q > 1000000 ? 1000000 : q);
}

// the lookup of one query minimizer, confined to the segment of its candidate's target
__global__ __launch_bounds__(TPB) void pairs_anchor_count_kernel(const uint32_t* mh, const int32_t* mseq, int64_t M,
                                                                 const int32_t* cand_tgt, const uint64_t* key,
                                                                 const int64_t* tmoff, const int32_t* max_occ,
                                                                 uint32_t* cnt, int64_t* lbo) {
    const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (m >= M) return;
    const int t = cand_tgt[mseq[m]];
    const int64_t b = tmoff[t], n = tmoff[t + 1] - b;
    const uint64_t h = mh[m];
    const int64_t lo = seg_bound(key + b, n, h);
    const int64_t hi = lo + seg_bound(key + b + lo, n - lo, h + 1);
    const int64_t c = hi - lo;
    cnt[m] = c > max_occ[t] ? 0u : (uint32_t)c;
    lbo[m] = b + lo;
}

__global__ __launch_bounds__(TPB) void pairs_anchor_write_kernel(const int64_t* off, int64_t M, const int32_t* mpos,
                                                                 const uint8_t* mst, const int32_t* mseq,
                                                                 const uint32_t* cnt, const int64_t* lbo,
                                                                 const int64_t* aoff, const int32_t* cand_tgt,
                                                                 const uint64_t* key, Anc* A) {
    const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (m >= M) return;
    const int s = mseq[m];
    const int64_t len = off[s + 1] - off[s], i = mpos[m];
    const uint32_t sq = mst[m];
    const uint64_t grp = (uint64_t)(uint32_t)cand_tgt[s] * 2u;
    const int64_t b = aoff[m], e0 = lbo[m];
    for (uint32_t e = 0; e < cnt[m]; ++e) {
        const uint64_t k = key[e0 + e];
        const uint32_t rev = sq != (uint32_t)(k & 1u) ? 1u : 0u;
        const uint64_t x = ((k >> 1) & 0x7fffffffull) + MK - 1;
        Anc a;
        a.key = ((grp + rev) << 32) | x;
        a.y = (uint32_t)(rev ? len - 1 - i : i + MK - 1);
        a.pad = 0;
        A[b + e] = a;
    }
}

// ---------------------------------------------------------------------------------------------------- host

// a grow-only device buffer
struct DBuf {
    void* p = nullptr;
    size_t n = 0;
    hipError_t need(int64_t bytes) {
        if (bytes <= (int64_t)n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        const size_t b = std::max<size_t>((size_t)bytes, 256);
        hipError_t e = hipMalloc(&p, b);
        if (e == hipSuccess) n = b;
        return e;
    }
    template <class T> T* as() const { return (T*)p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

inline unsigned blocks(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

// exclusive scan of in[0..n) into out[0..n] (out[n] = the total); tmp holds blocks(n, TILE) + 1 int64
int scan_u32(const uint32_t* in, int64_t n, int64_t* out, int64_t* tmp) {
    if (n == 0) {
        PO_HIPCHK(hipMemset(out, 0, sizeof(int64_t)));
        return PO_OK;
    }
    const int64_t nt = (n + TILE - 1) / TILE;
    scan_tile_sum_kernel<<<(unsigned)nt, TPB>>>(in, n, tmp);
    scan_tiles_kernel<<<1, TPB>>>(tmp, nt);
    scan_tile_write_kernel<<<(unsigned)nt, TPB>>>(in, n, tmp, nt, out);
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

struct Sketch {  // device buffers of one sketch pass
    DBuf seq, off, hs, ss, flag, scan, tmp, mh, mpos, mst, mseq, moff;
    void release() { for (DBuf* b : {&seq, &off, &hs, &ss, &flag, &scan, &tmp, &mh, &mpos, &mst, &mseq, &moff}) b->release(); }
};

// sketch n sequences already in s.seq / s.off (P bases): minimizers into s.mh/mpos/mst/mseq, per-sequence offsets s.moff
int run_sketch(Sketch& s, int n, int64_t P, bool with_seq) {
    PO_HIPCHK(s.hs.need(P * 4)); PO_HIPCHK(s.ss.need(P)); PO_HIPCHK(s.flag.need(P * 4)); PO_HIPCHK(s.scan.need((P + 1) * 8));
    PO_HIPCHK(s.tmp.need((blocks(P, TILE) + 1) * 8));
    PO_HIPCHK(s.mh.need(P * 4)); PO_HIPCHK(s.mpos.need(P * 4)); PO_HIPCHK(s.mst.need(P));
    if (with_seq) PO_HIPCHK(s.mseq.need(P * 4));
    PO_HIPCHK(s.moff.need((n + 1) * 8));
    if (P > 0) {
        map_hash_kernel<<<blocks(P, TPB), TPB>>>(s.seq.as<char>(), s.off.as<int64_t>(), n, P, s.hs.as<uint32_t>(),
                                                 s.ss.as<uint8_t>());
        map_minflag_kernel<<<blocks(P, TPB), TPB>>>(s.off.as<int64_t>(), n, P, s.hs.as<uint32_t>(), s.flag.as<uint32_t>());
    }
    int rc = scan_u32(s.flag.as<uint32_t>(), P, s.scan.as<int64_t>(), s.tmp.as<int64_t>());
    if (rc) return rc;
    if (P > 0)
        map_emit_kernel<<<blocks(P, TPB), TPB>>>(s.off.as<int64_t>(), n, P, s.hs.as<uint32_t>(), s.ss.as<uint8_t>(),
                                                 s.flag.as<uint32_t>(), s.scan.as<int64_t>(), s.mh.as<uint32_t>(),
                                                 s.mpos.as<int32_t>(), s.mst.as<uint8_t>(),
                                                 with_seq ? s.mseq.as<int32_t>() : nullptr);
    map_gather_off_kernel<<<blocks(n + 1, TPB), TPB>>>(s.off.as<int64_t>(), n, s.scan.as<int64_t>(), s.moff.as<int64_t>());
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

}  // namespace

struct po_map_index {
    int n_ctg = 0;
    int64_t n_entries = 0;
    DBuf ctg, ctg_off, ih, ipos, ics;
    // per-batch workspace (grow-only)
    Sketch sk;
    DBuf cnt, lbo, aoff, raoff, A, scratch, soff, f, p, chain, co, list, band_lo, tb, best, opoff, ops, hits;
    hipEvent_t ev[6] = {};
};

extern "C" {

size_t po_map_workspace_bytes(int64_t bases, int n_reads) {
    if (bases < 0 || n_reads < 0) return 0;
    return (size_t)(bases * BYTES_PER_BASE + (int64_t)n_reads * BYTES_PER_READ);
}

int po_map_sketch_h(const char* seq_h, const int64_t* off_h, int n, uint32_t* hash_h, int32_t* pos_h, uint8_t* strand_h,
                    int64_t* moff_h) {
    po_set_error("");
    if (n < 0 || (n > 0 && (!off_h || !moff_h))) return po_fail(PO_E_ARG, "po_map_sketch_h: bad arguments");
    if (n == 0) return PO_OK;
    const int64_t P = off_h[n];
    if (off_h[0] != 0) return po_fail(PO_E_ARG, "po_map_sketch_h: offsets must start at 0");
    for (int i = 0; i < n; ++i)
        if (off_h[i + 1] < off_h[i]) return po_fail(PO_E_ARG, "po_map_sketch_h: offsets must not decrease");
    Sketch s;
    auto body = [&]() -> int {
        PO_HIPCHK(s.seq.need(P + 1)); PO_HIPCHK(s.off.need((n + 1) * 8));
        if (P) PO_HIPCHK(hipMemcpy(s.seq.p, seq_h, P, hipMemcpyHostToDevice));
        PO_HIPCHK(hipMemcpy(s.off.p, off_h, (n + 1) * 8, hipMemcpyHostToDevice));
        const int r = run_sketch(s, n, P, false);
        if (r) return r;
        PO_HIPCHK(hipMemcpy(moff_h, s.moff.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        const int64_t M = moff_h[n];
        if (M) {
            PO_HIPCHK(hipMemcpy(hash_h, s.mh.p, M * 4, hipMemcpyDeviceToHost));
            PO_HIPCHK(hipMemcpy(pos_h, s.mpos.p, M * 4, hipMemcpyDeviceToHost));
            PO_HIPCHK(hipMemcpy(strand_h, s.mst.p, M, hipMemcpyDeviceToHost));
        }
        return PO_OK;
    };
    const int rc = body();
    s.release();
    return rc;
}

po_map_index* po_map_index_create(const char* ctg_h, const int64_t* ctg_off_h, int n_ctg, const uint32_t* hash_h,
                                  const uint32_t* pos_h, const uint32_t* ctg_strand_h, int64_t n_entries) {
    po_set_error("");
    if (n_ctg < 1 || !ctg_off_h || n_entries < 0 || ctg_off_h[0] != 0) {
        po_fail(PO_E_ARG, "po_map_index_create: bad arguments");
        return nullptr;
    }
    for (int i = 0; i < n_ctg; ++i)
        if (ctg_off_h[i + 1] < ctg_off_h[i] || ctg_off_h[i + 1] - ctg_off_h[i] >= ((int64_t)1 << 31)) {
            po_fail(PO_E_ARG, "po_map_index_create: contig offsets must not decrease and contigs must be < 2^31 bases");
            return nullptr;
        }
    po_map_index* ix = new po_map_index;
    ix->n_ctg = n_ctg;
    ix->n_entries = n_entries;
    const int64_t G = ctg_off_h[n_ctg];
    auto body = [&]() -> int {
        PO_HIPCHK(ix->ctg.need(G + 1)); PO_HIPCHK(ix->ctg_off.need((n_ctg + 1) * 8));
        PO_HIPCHK(ix->ih.need(n_entries * 4 + 4)); PO_HIPCHK(ix->ipos.need(n_entries * 4 + 4)); PO_HIPCHK(ix->ics.need(n_entries * 4 + 4));
        if (G) PO_HIPCHK(hipMemcpy(ix->ctg.p, ctg_h, G, hipMemcpyHostToDevice));
        PO_HIPCHK(hipMemcpy(ix->ctg_off.p, ctg_off_h, (n_ctg + 1) * 8, hipMemcpyHostToDevice));
        if (n_entries) {
            PO_HIPCHK(hipMemcpy(ix->ih.p, hash_h, n_entries * 4, hipMemcpyHostToDevice));
            PO_HIPCHK(hipMemcpy(ix->ipos.p, pos_h, n_entries * 4, hipMemcpyHostToDevice));
            PO_HIPCHK(hipMemcpy(ix->ics.p, ctg_strand_h, n_entries * 4, hipMemcpyHostToDevice));
        }
        for (auto& e : ix->ev) PO_HIPCHK(hipEventCreate(&e));
        return PO_OK;
    };
    if (body() != PO_OK) {
        po_map_index_destroy(ix);
        return nullptr;
    }
    return ix;
}

void po_map_index_destroy(po_map_index* ix) {
    if (!ix) return;
    (void)hipDeviceSynchronize();
    for (DBuf* b : {&ix->ctg, &ix->ctg_off, &ix->ih, &ix->ipos, &ix->ics, &ix->cnt, &ix->lbo, &ix->aoff, &ix->raoff, &ix->A,
                    &ix->scratch, &ix->soff, &ix->f, &ix->p, &ix->chain, &ix->co, &ix->list, &ix->band_lo, &ix->tb,
                    &ix->best, &ix->opoff, &ix->ops, &ix->hits})
        b->release();
    ix->sk.release();
    for (auto& e : ix->ev)
        if (e) (void)hipEventDestroy(e);
    delete ix;
}

}  // extern "C"

namespace {

// what a batch of candidates adds to a batch of reads (device pointers, but qry): the target slot of every read of the
// batch, the targets' sorted keys with their segment offsets and max_occ, and the targets themselves as the contigs
struct PairCtx {
    const int32_t* qry;  // HOST: the sequence each read of the batch is
    const int32_t* cand_tgt;
    const uint64_t* key;
    const int64_t* tmoff;
    const int32_t* max_occ;
    const char* ctg;
    const int64_t* ctg_off;
};

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = 0.f;
    return ms;
}

// one batch: reads ids (indices into the caller's arrays); hits into hits_h, op bytes appended to ops_all; debug arrays
// at the caller's offsets
// pc (pairs, §14): read ids[i] is sequence pc->qry[ids[i]] of seq_h and is looked up in the segment of its own target alone
int run_batch(po_map_index* ix, const char* seq_h, const int64_t* off_h, const std::vector<int>& ids, po_map_hit* hits_h,
              std::vector<uint8_t>& ops_all, const int64_t* aoff_h, const int64_t* choff_h, po_map_debug* dbg,
              double* stats, const PairCtx* pc = nullptr) {
    const int nb = (int)ids.size();
    auto src = [&](int i) { return pc ? pc->qry[ids[i]] : ids[i]; };
    std::vector<int64_t> off(nb + 1, 0);
    for (int i = 0; i < nb; ++i) off[i + 1] = off[i] + (off_h[src(i) + 1] - off_h[src(i)]);
    const int64_t P = off[nb];
    std::vector<char> hseq(P + 1, 0);
    for (int i = 0; i < nb; ++i) memcpy(hseq.data() + off[i], seq_h + off_h[src(i)], off[i + 1] - off[i]);
    Sketch& s = ix->sk;
    PO_HIPCHK(s.seq.need(P + 1)); PO_HIPCHK(s.off.need((nb + 1) * 8));
    PO_HIPCHK(hipMemcpy(s.seq.p, hseq.data(), P + 1, hipMemcpyHostToDevice));
    PO_HIPCHK(hipMemcpy(s.off.p, off.data(), (nb + 1) * 8, hipMemcpyHostToDevice));
    PO_HIPCHK(hipEventRecord(ix->ev[0], 0));
    int rc = run_sketch(s, nb, P, true);
    if (rc) return rc;
    PO_HIPCHK(hipEventRecord(ix->ev[1], 0));
    // anchors: count, scan, per-read offsets
    std::vector<int64_t> mo(nb + 1);
    PO_HIPCHK(hipMemcpy(mo.data(), s.moff.p, (nb + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t M = mo[nb];
    PO_HIPCHK(ix->cnt.need(M * 4 + 4)); PO_HIPCHK(ix->lbo.need(M * 8 + 8)); PO_HIPCHK(ix->aoff.need((M + 1) * 8));
    PO_HIPCHK(ix->raoff.need((nb + 1) * 8));
    if (M && pc)
        pairs_anchor_count_kernel<<<blocks(M, TPB), TPB>>>(s.mh.as<uint32_t>(), s.mseq.as<int32_t>(), M, pc->cand_tgt,
                                                           pc->key, pc->tmoff, pc->max_occ, ix->cnt.as<uint32_t>(),
                                                           ix->lbo.as<int64_t>());
    else if (M)
        map_anchor_count_kernel<<<blocks(M, TPB), TPB>>>(s.mh.as<uint32_t>(), M, ix->ih.as<uint32_t>(), ix->n_entries,
                                                         ix->cnt.as<uint32_t>(), ix->lbo.as<int64_t>());
    PO_HIPCHK(s.tmp.need((blocks(M, TILE) + 1) * 8));
    rc = scan_u32(ix->cnt.as<uint32_t>(), M, ix->aoff.as<int64_t>(), s.tmp.as<int64_t>());
    if (rc) return rc;
    map_gather_off_kernel<<<blocks(nb + 1, TPB), TPB>>>(s.moff.as<int64_t>(), nb, ix->aoff.as<int64_t>(),
                                                        ix->raoff.as<int64_t>());
    PO_HIPCHK(hipGetLastError());
    std::vector<int64_t> raoff(nb + 1);
    PO_HIPCHK(hipMemcpy(raoff.data(), ix->raoff.p, (nb + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t NA = raoff[nb];
    std::vector<int64_t> soff(nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
        int64_t n = raoff[i + 1] - raoff[i], np2 = 1;
        while (np2 < n) np2 <<= 1;
        soff[i + 1] = soff[i] + (np2 > SORT_LDS ? np2 : 0);
    }
    PO_HIPCHK(ix->A.need((NA + 1) * (int64_t)sizeof(Anc))); PO_HIPCHK(ix->scratch.need((soff[nb] + 1) * (int64_t)sizeof(Anc)));
    PO_HIPCHK(ix->soff.need((nb + 1) * 8));
    PO_HIPCHK(hipMemcpy(ix->soff.p, soff.data(), (nb + 1) * 8, hipMemcpyHostToDevice));
    if (M && pc)
        pairs_anchor_write_kernel<<<blocks(M, TPB), TPB>>>(s.off.as<int64_t>(), M, s.mpos.as<int32_t>(), s.mst.as<uint8_t>(),
                                                           s.mseq.as<int32_t>(), ix->cnt.as<uint32_t>(), ix->lbo.as<int64_t>(),
                                                           ix->aoff.as<int64_t>(), pc->cand_tgt, pc->key, ix->A.as<Anc>());
    else if (M)
        map_anchor_write_kernel<<<blocks(M, TPB), TPB>>>(s.off.as<int64_t>(), M, s.mpos.as<int32_t>(), s.mst.as<uint8_t>(),
                                                         s.mseq.as<int32_t>(), ix->cnt.as<uint32_t>(), ix->lbo.as<int64_t>(),
                                                         ix->aoff.as<int64_t>(), ix->ipos.as<uint32_t>(),
                                                         ix->ics.as<uint32_t>(), ix->A.as<Anc>());
    map_sort_kernel<<<nb, TPB>>>(ix->A.as<Anc>(), ix->raoff.as<int64_t>(), ix->scratch.as<Anc>(), ix->soff.as<int64_t>());
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipEventRecord(ix->ev[2], 0));
    // chain
    PO_HIPCHK(ix->f.need(NA * 4 + 4)); PO_HIPCHK(ix->p.need(NA * 4 + 4)); PO_HIPCHK(ix->chain.need(NA * 4 + 4));
    PO_HIPCHK(ix->co.need(nb * (int64_t)sizeof(ChainOut)));
    map_chain_kernel<<<nb, 64>>>(ix->A.as<Anc>(), ix->raoff.as<int64_t>(), ix->f.as<int32_t>(), ix->p.as<int32_t>(),
                                 ix->chain.as<int32_t>(), ix->co.as<ChainOut>());
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipEventRecord(ix->ev[3], 0));
    std::vector<ChainOut> co(nb);
    PO_HIPCHK(hipMemcpy(co.data(), ix->co.p, nb * sizeof(ChainOut), hipMemcpyDeviceToHost));
    // align the reads whose chain passes; an op byte per alignment column: at most 2 len + (max D - min D) + 512
    std::vector<int32_t> list;
    std::vector<int64_t> opoff(nb + 1, 0);
    double cells = 0;
    for (int i = 0; i < nb; ++i) {
        int64_t capi = 0;
        if (co[i].ok) {
            list.push_back(i);
            const int64_t len = off[i + 1] - off[i];
            capi = 2 * len + (co[i].dmax - co[i].dmin) + BAND;
            cells += (double)len * BAND;
        }
        opoff[i + 1] = opoff[i] + capi;
    }
    std::vector<po_map_hit> hb(nb);
    for (int i = 0; i < nb; ++i) {
        po_map_hit h;
        memset(&h, 0, sizeof(h));
        h.n_anchors = (int32_t)(raoff[i + 1] - raoff[i]);
        h.n_chain = co[i].n_chain;
        h.chain_score = co[i].score;
        hb[i] = h;
    }
    const int nl = (int)list.size();
    PO_HIPCHK(ix->hits.need(nb * (int64_t)sizeof(po_map_hit)));
    PO_HIPCHK(hipMemcpy(ix->hits.p, hb.data(), nb * sizeof(po_map_hit), hipMemcpyHostToDevice));
    PO_HIPCHK(ix->band_lo.need(P * 4 + 4)); PO_HIPCHK(ix->tb.need(P * 256 + 256)); PO_HIPCHK(ix->best.need(nb * (int64_t)sizeof(BestOut)));
    PO_HIPCHK(ix->opoff.need((nb + 1) * 8)); PO_HIPCHK(ix->ops.need(opoff[nb] + 1)); PO_HIPCHK(ix->list.need(nl * 4 + 4));
    PO_HIPCHK(hipMemcpy(ix->opoff.p, opoff.data(), (nb + 1) * 8, hipMemcpyHostToDevice));
    if (nl) PO_HIPCHK(hipMemcpy(ix->list.p, list.data(), nl * 4, hipMemcpyHostToDevice));
    PO_HIPCHK(hipEventRecord(ix->ev[4], 0));
    if (nl) {
        const char* ctg = pc ? pc->ctg : ix->ctg.as<char>();
        const int64_t* ctg_off = pc ? pc->ctg_off : ix->ctg_off.as<int64_t>();
        AlignArgs a{ix->list.as<int32_t>(), s.seq.as<char>(), s.off.as<int64_t>(), ix->A.as<Anc>(), ix->raoff.as<int64_t>(),
                    ix->chain.as<int32_t>(), ix->co.as<ChainOut>(), ctg, ctg_off,
                    ix->band_lo.as<int32_t>(), ix->tb.as<uint32_t>(), ix->best.as<BestOut>()};
        map_align_kernel<<<nl, 64>>>(a);
        TraceArgs t{ix->list.as<int32_t>(), nl, s.seq.as<char>(), s.off.as<int64_t>(), ix->co.as<ChainOut>(),
                    ctg, ctg_off, ix->band_lo.as<int32_t>(), ix->tb.as<uint32_t>(),
                    ix->best.as<BestOut>(), ix->opoff.as<int64_t>(), ix->ops.as<uint8_t>(), ix->hits.as<po_map_hit>()};
        map_trace_kernel<<<blocks(nl, 64), 64>>>(t);
        PO_HIPCHK(hipGetLastError());
    }
    PO_HIPCHK(hipEventRecord(ix->ev[5], 0));
    PO_HIPCHK(hipMemcpy(hb.data(), ix->hits.p, nb * sizeof(po_map_hit), hipMemcpyDeviceToHost));
    std::vector<uint8_t> ops(opoff[nb]);
    if (opoff[nb]) PO_HIPCHK(hipMemcpy(ops.data(), ix->ops.p, opoff[nb], hipMemcpyDeviceToHost));
    if (stats) {
        stats[0] += elapsed(ix->ev[0], ix->ev[1]);
        stats[1] += elapsed(ix->ev[1], ix->ev[2]);
        stats[2] += elapsed(ix->ev[2], ix->ev[3]);
        stats[3] += elapsed(ix->ev[4], ix->ev[5]);
        stats[4] += cells;
        stats[5] += 1;
    }
    for (int i = 0; i < nb; ++i) {
        po_map_hit h = hb[i];
        h.op_off = (int64_t)ops_all.size();
        if (h.mapped) ops_all.insert(ops_all.end(), ops.begin() + opoff[i], ops.begin() + opoff[i] + h.n_ops);
        else h.n_ops = 0;
        hits_h[ids[i]] = h;
    }
    if (dbg) {
        std::vector<Anc> A(NA);
        std::vector<int32_t> ch(NA);
        if (NA) {
            PO_HIPCHK(hipMemcpy(A.data(), ix->A.p, NA * sizeof(Anc), hipMemcpyDeviceToHost));
            PO_HIPCHK(hipMemcpy(ch.data(), ix->chain.p, NA * 4, hipMemcpyDeviceToHost));
        }
        std::vector<int32_t> bl(P);
        if (P) PO_HIPCHK(hipMemcpy(bl.data(), ix->band_lo.p, P * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < nb; ++i) {
            const int r = ids[i];
            for (int64_t e = raoff[i]; e < raoff[i + 1]; ++e) {
                if (dbg->anchor_key) dbg->anchor_key[aoff_h[r] + e - raoff[i]] = A[e].key;
                if (dbg->anchor_y) dbg->anchor_y[aoff_h[r] + e - raoff[i]] = A[e].y;
            }
            if (dbg->chain)
                for (int e = 0; e < co[i].n_chain; ++e) dbg->chain[choff_h[r] + e] = ch[raoff[i] + e];
            if (dbg->band_lo && co[i].ok) memcpy(dbg->band_lo + off_h[r], bl.data() + off[i], (off[i + 1] - off[i]) * 4);
        }
    }
    return PO_OK;
}

}  // namespace

extern "C" int po_map_batch_h(po_map_index* ix, const char* seq_h, const int64_t* off_h, int n, int64_t budget,
                              po_map_hit* hits_h, uint8_t* ops_h, int64_t ops_cap, int64_t* ops_len, po_map_debug* dbg,
                              double* stats_h) {
    po_set_error("");
    if (!ix || n < 0 || (n > 0 && (!off_h || !hits_h)) || ops_cap < 0)
        return po_fail(PO_E_ARG, "po_map_batch_h: bad arguments");
    if (stats_h)
        for (int i = 0; i < 6; ++i) stats_h[i] = 0;
    if (n == 0) {
        if (ops_len) *ops_len = 0;
        return PO_OK;
    }
    if (off_h[0] != 0) return po_fail(PO_E_ARG, "po_map_batch_h: offsets must start at 0");
    for (int i = 0; i < n; ++i)
        if (off_h[i + 1] < off_h[i] || off_h[i + 1] - off_h[i] >= ((int64_t)1 << 31))
            return po_fail(PO_E_ARG, "po_map_batch_h: offsets must not decrease and reads must be < 2^31 bases");
    if (budget <= 0) budget = (int64_t)std::min<size_t>((size_t)8 << 30, po_dev_info().mem / 16);
    // the debug arrays are laid out by the counts a previous call with the same reads left in hits_h
    std::vector<int64_t> aoff_h(n + 1, 0), choff_h(n + 1, 0);
    if (dbg)
        for (int i = 0; i < n; ++i) {
            aoff_h[i + 1] = aoff_h[i] + hits_h[i].n_anchors;
            choff_h[i + 1] = choff_h[i] + hits_h[i].n_chain;
        }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return off_h[a + 1] - off_h[a] > off_h[b + 1] - off_h[b];
    });
    std::vector<uint8_t> ops_all;
    for (size_t i = 0; i < order.size();) {
        std::vector<int> ids;
        int64_t bytes = 0;
        while (i < order.size()) {
            const int r = order[i];
            const int64_t b = (off_h[r + 1] - off_h[r]) * BYTES_PER_BASE + BYTES_PER_READ;
            if (!ids.empty() && bytes + b > budget) break;
            ids.push_back(r);
            bytes += b;
            ++i;
        }
        const int rc = run_batch(ix, seq_h, off_h, ids, hits_h, ops_all, aoff_h.data(), choff_h.data(), dbg, stats_h);
        if (rc) return rc;
    }
    if (ops_len) *ops_len = (int64_t)ops_all.size();
    if ((int64_t)ops_all.size() > ops_cap || (!ops_h && !ops_all.empty()))
        return po_fail(PO_E_CAP, "po_map_batch_h: ops_cap " + std::to_string(ops_cap) + " < " +
                       std::to_string(ops_all.size()) + " alignment columns");
    if (!ops_all.empty()) memcpy(ops_h, ops_all.data(), ops_all.size());
    return PO_OK;
}

// ---------------------------------------------------------------------------------------------------- pairs: host

namespace {

// device bytes per target base of a batch: sequence, hashes, strands, flags, scan, minimizers, and per minimizer (at most
// one per base) the key, its sort scratch (two slots: the next power of two) and the run count
constexpr int64_t TGT_BYTES_PER_BASE = 1 + 4 + 1 + 4 + 8 + (4 + 4 + 1) + 8 + 16 + 4;

struct PairWork {
    Sketch ts;
    DBuf key, scratch, soff, runc, max_occ, cand_tgt;
    hipEvent_t ev[3] = {};
    void release() {
        ts.release();
        for (DBuf* b : {&key, &scratch, &soff, &runc, &max_occ, &cand_tgt}) b->release();
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// one batch of candidates: sketch the distinct targets they name, sort each target's minimizers inside its own segment,
// take its max_occ, then the read pipeline with the lookup confined to each candidate's segment
int run_pairs_batch(po_map_index* ix, PairWork& w, const char* tgt_h, const int64_t* tgt_off_h, const char* qry_h,
                    const int64_t* qry_off_h, const int32_t* cand_h, const std::vector<int>& ids,
                    std::vector<int32_t>& slot_of, po_map_hit* hits_h, std::vector<uint8_t>& ops_all, double* stats) {
    const int nb = (int)ids.size();
    std::vector<int32_t> tgts, cand_tgt(nb);
    for (int i = 0; i < nb; ++i) {
        const int32_t t = cand_h[2 * (int64_t)ids[i] + 1];
        if (slot_of[t] < 0) {
            slot_of[t] = (int32_t)tgts.size();
            tgts.push_back(t);
        }
        cand_tgt[i] = slot_of[t];
    }
    for (int32_t t : tgts) slot_of[t] = -1;
    const int nt = (int)tgts.size();
    std::vector<int64_t> toff(nt + 1, 0);
    for (int i = 0; i < nt; ++i) toff[i + 1] = toff[i] + (tgt_off_h[tgts[i] + 1] - tgt_off_h[tgts[i]]);
    const int64_t PT = toff[nt];
    std::vector<char> tseq(PT + 1, 0);
    for (int i = 0; i < nt; ++i) memcpy(tseq.data() + toff[i], tgt_h + tgt_off_h[tgts[i]], toff[i + 1] - toff[i]);
    Sketch& ts = w.ts;
    PO_HIPCHK(ts.seq.need(PT + 1)); PO_HIPCHK(ts.off.need((nt + 1) * 8)); PO_HIPCHK(w.cand_tgt.need(nb * 4 + 4));
    PO_HIPCHK(hipMemcpy(ts.seq.p, tseq.data(), PT + 1, hipMemcpyHostToDevice));
    PO_HIPCHK(hipMemcpy(ts.off.p, toff.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
    PO_HIPCHK(hipMemcpy(w.cand_tgt.p, cand_tgt.data(), nb * 4, hipMemcpyHostToDevice));
    PO_HIPCHK(hipEventRecord(w.ev[0], 0));
    int rc = run_sketch(ts, nt, PT, false);
    if (rc) return rc;
    PO_HIPCHK(hipEventRecord(w.ev[1], 0));
    std::vector<int64_t> tmoff(nt + 1);
    PO_HIPCHK(hipMemcpy(tmoff.data(), ts.moff.p, (nt + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t MT = tmoff[nt];
    std::vector<int64_t> soff(nt + 1, 0);
    for (int i = 0; i < nt; ++i) {
        int64_t n = tmoff[i + 1] - tmoff[i], np2 = 1;
        while (np2 < n) np2 <<= 1;
        soff[i + 1] = soff[i] + (np2 > SEG_LDS ? np2 : 0);
    }
    PO_HIPCHK(w.key.need(MT * 8 + 8)); PO_HIPCHK(w.runc.need(MT * 4 + 4)); PO_HIPCHK(w.max_occ.need(nt * 4 + 4));
    PO_HIPCHK(w.scratch.need(soff[nt] * 8 + 8)); PO_HIPCHK(w.soff.need((nt + 1) * 8));
    PO_HIPCHK(hipMemcpy(w.soff.p, soff.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
    pairs_segsort_kernel<<<nt, TPB>>>(ts.mh.as<uint32_t>(), ts.mpos.as<int32_t>(), ts.mst.as<uint8_t>(),
                                      ts.moff.as<int64_t>(), w.key.as<uint64_t>(), w.scratch.as<uint64_t>(),
                                      w.soff.as<int64_t>());
    pairs_maxocc_kernel<<<nt, TPB>>>(w.key.as<uint64_t>(), ts.moff.as<int64_t>(), w.runc.as<uint32_t>(),
                                     w.max_occ.as<int32_t>());
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipEventRecord(w.ev[2], 0));
    // the batch's reads are its candidates' queries, numbered 0 .. nb - 1
    std::vector<int> local(nb);
    std::vector<int32_t> qry(nb);
    for (int i = 0; i < nb; ++i) { qry[i] = cand_h[2 * (int64_t)ids[i]]; local[i] = i; }
    const PairCtx pc{qry.data(), w.cand_tgt.as<int32_t>(), w.key.as<uint64_t>(), ts.moff.as<int64_t>(),
                     w.max_occ.as<int32_t>(), ts.seq.as<char>(), ts.off.as<int64_t>()};
    std::vector<po_map_hit> hb(nb);
    rc = run_batch(ix, qry_h, qry_off_h, local, hb.data(), ops_all, nullptr, nullptr, nullptr, stats, &pc);
    if (rc) return rc;
    for (int i = 0; i < nb; ++i) {
        hb[i].ctg = cand_h[2 * (int64_t)ids[i] + 1];
        hits_h[ids[i]] = hb[i];
    }
    if (stats) {
        stats[0] += elapsed(w.ev[0], w.ev[1]);
        stats[6] += elapsed(w.ev[1], w.ev[2]);
        stats[7] += nt;
    }
    return PO_OK;
}

}  // namespace

extern "C" int po_map_pairs_h(const char* tgt_h, const int64_t* tgt_off_h, int n_tgt, const char* qry_h,
                              const int64_t* qry_off_h, int n_qry, const int32_t* cand_h, int n_cand, int64_t budget,
                              po_map_hit* hits_h, uint8_t* ops_h, int64_t ops_cap, int64_t* ops_len, double* stats_h) {
    po_set_error("");
    if (n_tgt < 0 || n_qry < 0 || n_cand < 0 || ops_cap < 0 || (n_tgt > 0 && !tgt_off_h) || (n_qry > 0 && !qry_off_h) ||
        (n_cand > 0 && (!cand_h || !hits_h)))
        return po_fail(PO_E_ARG, "po_map_pairs_h: bad arguments");
    if (stats_h)
        for (int i = 0; i < 8; ++i) stats_h[i] = 0;
    if (ops_len) *ops_len = 0;
    for (int s = 0; s < 2; ++s) {
        const int64_t* off = s ? qry_off_h : tgt_off_h;
        const int n = s ? n_qry : n_tgt;
        if (n > 0 && off[0] != 0) return po_fail(PO_E_ARG, "po_map_pairs_h: offsets must start at 0");
        for (int i = 0; i < n; ++i)
            if (off[i + 1] < off[i] || off[i + 1] - off[i] >= ((int64_t)1 << 31))
                return po_fail(PO_E_ARG, "po_map_pairs_h: offsets must not decrease and sequences must be < 2^31 bases");
    }
    for (int64_t c = 0; c < n_cand; ++c)
        if (cand_h[2 * c] < 0 || cand_h[2 * c] >= n_qry || cand_h[2 * c + 1] < 0 || cand_h[2 * c + 1] >= n_tgt)
            return po_fail(PO_E_ARG, "po_map_pairs_h: candidate " + std::to_string(c) + " names a sequence out of range");
    if (n_cand == 0) return PO_OK;
    if (budget <= 0) budget = (int64_t)std::min<size_t>((size_t)8 << 30, po_dev_info().mem / 16);
    auto qlen = [&](int c) { return qry_off_h[cand_h[2 * (int64_t)c] + 1] - qry_off_h[cand_h[2 * (int64_t)c]]; };
    auto tlen = [&](int c) { return tgt_off_h[cand_h[2 * (int64_t)c + 1] + 1] - tgt_off_h[cand_h[2 * (int64_t)c + 1]]; };
    std::vector<int> order(n_cand);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return qlen(a) > qlen(b); });
    po_map_index* ix = new po_map_index;  // the batch workspace only: no contigs, no entries
    PairWork w;
    std::vector<uint8_t> ops_all;
    std::vector<int32_t> slot_of(n_tgt, -1);
    std::vector<char> in_batch(n_tgt, 0);
    auto body = [&]() -> int {
        for (auto& e : ix->ev) PO_HIPCHK(hipEventCreate(&e));
        for (auto& e : w.ev) PO_HIPCHK(hipEventCreate(&e));
        for (size_t i = 0; i < order.size();) {
            std::vector<int> ids;
            int64_t bytes = 0;
            while (i < order.size()) {
                const int c = order[i];
                const int32_t t = cand_h[2 * (int64_t)c + 1];
                int64_t b = qlen(c) * BYTES_PER_BASE + BYTES_PER_READ;
                if (!in_batch[t]) b += tlen(c) * TGT_BYTES_PER_BASE + BYTES_PER_READ;
                if (!ids.empty() && bytes + b > budget) break;
                in_batch[t] = 1;
                ids.push_back(c);
                bytes += b;
                ++i;
            }
            for (int c : ids) in_batch[cand_h[2 * (int64_t)c + 1]] = 0;
            const int rc = run_pairs_batch(ix, w, tgt_h, tgt_off_h, qry_h, qry_off_h, cand_h, ids, slot_of, hits_h, ops_all,
                                           stats_h);
            if (rc) return rc;
        }
        return PO_OK;
    };
    const int rc = body();
    w.release();
    po_map_index_destroy(ix);
    if (rc) return rc;
    if (ops_len) *ops_len = (int64_t)ops_all.size();
    if ((int64_t)ops_all.size() > ops_cap || (!ops_h && !ops_all.empty()))
        return po_fail(PO_E_CAP, "po_map_pairs_h: ops_cap " + std::to_string(ops_cap) + " < " +
                       std::to_string(ops_all.size()) + " alignment columns");
    if (!ops_all.empty()) memcpy(ops_h, ops_all.data(), ops_all.size());
    return PO_OK;
}
