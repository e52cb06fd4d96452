// The kernels under tensors.edit_alignment (the rules are po_aln_rules.h's, which tools/aln_check.cpp holds
// against the full table and the naive walk).  They sit beside po_acc.hip's edit_stats_kernel and keep its design:
//
//   edit_align_kernel     one wave per pair, edit_stats_kernel's layout and its two launches (K <= 8 | K >= 16 and the
//                         refusals): the packed key's rows with, per row, each cell's op packed 2 bits a cell into the item's
//                         trace region, one store per lane (K >= 16: K / 16 adjacent words a row; K < 16: one word every 16 / K
//                         rows).  Then d, m and the ops' length m + d.  An item whose room is short stores nothing.
//   edit_walk_kernel      one wave per pair, behind it on the stream: from (L, S) back to (0, 0), the ops written from position
//                         m + d - 1 down, 64 at a time with one coalesced store.  The 64 lanes hold the trace words of the next
//                         64 rows around the diagonal (two adjacent words each); a cell outside them fetches the block anew.
//   edit_confusion_kernel one wave per pair over the finished ops, 64 columns a step: a ballot and a popcount below the lane
//                         give each column's hypothesis and truth index, the 25 counts are kept per lane and reduced at the end.
//
// The walk is a kernel of its own and no tail of edit_align_kernel: there is one copy of it and not one per launch, the launch
// boundary orders the trace's stores before its loads without a fence, it runs in a few dozen registers where the K = 64 rows
// need all of them, and the forward pass and the walk can be timed apart.
// No atomics, no LDS, one writer per value, nothing depends on the launch geometry or the batch position.  po_edit_align is
// enqueue-only: no allocation, no synchronisation, no host read of device memory.  po_edit_align_h reaches it from host arrays.
#include <string>
#include <vector>

#include "po_aln_rules.h"
#include "po_hostbuf.h"

static_assert(PO_ACC_MAX_LONG == PO_EDIT_STATS_MAX_LONG, "the header's cap is the rules'");
static_assert(PO_ALN_CELLS == PO_EDIT_ALIGN_CELLS, "the header's confusion table is the rules'");

struct PoAlignArgs {
    const uint8_t* a; const int64_t* a_off; const int32_t* a_len;
    const uint8_t* b; const int64_t* b_off; const int32_t* b_len;
    uint32_t* trace; const int64_t* trace_off;
    uint8_t* ops; int64_t ops_stride; int32_t* ops_len;
    int32_t* dist; int32_t* matches; int32_t* confusion; int32_t* status;
};

namespace {

// a lane's words of one row: adjacent, 4-byte aligned (an item's region starts at any word)
template <int W>
struct __attribute__((aligned(4))) TraceWords { uint32_t v[W]; };

// po_acc.hip's wave_excl_min: the exclusive prefix minimum of the lanes' totals, a move per step
__device__ __forceinline__ int32_t wave_excl_min(int32_t v) {
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x138, 0xf, 0xf, false);               // wave_shr:1
}

// the inclusive sum over the wave, in every lane
__device__ __forceinline__ int32_t wave_sum(int32_t v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8: lane 15 of each row holds the row's sum
    return __builtin_amdgcn_readlane(v, 15) + __builtin_amdgcn_readlane(v, 31) + __builtin_amdgcn_readlane(v, 47) +
           __builtin_amdgcn_readlane(v, 63);
}

// stats_wave (po_acc.hip) with the ops: the key of lo[0..L) against sh[0..S) in the lane that holds column S, and, where tr is
// no null pointer, the item's trace (po_aln_words(K, L) words from tr on)
template <int K>
__device__ __forceinline__ int32_t align_wave(const uint8_t* __restrict__ lo, int L, const uint8_t* __restrict__ sh, int S, int lane,
                                              bool cols_hyp, uint32_t* __restrict__ tr) {
    constexpr int W = (K + 15) / 16, R = K < 16 ? 16 / K : 1;
    int32_t row[K];
    uint32_t sym[(K + 3) / 4];
    po_ev_load_symbols<K>(sym, sh, S, lane);
    po_acc_row_init<K>(row, lane);
    int32_t diag = po_acc_diag_init<K>(lane);
    const uint32_t tie_left = cols_hyp ? ~0u : 0u;
    uint32_t acc = 0;   // K < 16: the word of the R rows in flight
    for (int i0 = 0; i0 < L; i0 += PO_EV_WAVE) {
        const int xs = i0 + lane < L ? (int)lo[i0 + lane] : 0;
        const int m = L - i0 < PO_EV_WAVE ? L - i0 : PO_EV_WAVE;
        for (int r = 0; r < m; ++r) {
            const int x = __builtin_amdgcn_readlane(xs, r);
            const int i = i0 + r + 1;
            uint32_t st[W], code[W];
            const int32_t total = po_aln_row_local<K>(row, st, sym, diag, x, i, tie_left, lane);
            diag = po_aln_row_finish<K>(row, code, st, wave_excl_min(total), tie_left, lane);
            if constexpr (K >= 16) {
                if (tr) {
                    TraceWords<W> out;
                    PO_EV_UNROLL
                    for (int q = 0; q < W; ++q) out.v[q] = code[q];
                    *(TraceWords<W>*)(tr + ((int64_t)(i - 1) * PO_EV_WAVE + lane) * W) = out;
                }
            } else {
                const int sub = (i - 1) & (R - 1);
                acc |= (code[0] & ((1u << (2 * K)) - 1)) << (sub * 2 * K);
                if (sub == R - 1 || i == L) {
                    if (tr) tr[(int64_t)((i - 1) / R) * PO_EV_WAVE + lane] = acc;
                    acc = 0;
                }
            }
        }
    }
    return po_ev_row_pick<K>(row, S);
}

template <bool WIDE>
__device__ __forceinline__ int32_t align_any(int K, const uint8_t* lo, int L, const uint8_t* sh, int S, int lane, bool cols_hyp,
                                             uint32_t* tr) {
    if constexpr (WIDE) {
        switch (K) {
            case 16: return align_wave<16>(lo, L, sh, S, lane, cols_hyp, tr);
            case 32: return align_wave<32>(lo, L, sh, S, lane, cols_hyp, tr);
            default: return align_wave<PO_EV_MAX_SLOTS>(lo, L, sh, S, lane, cols_hyp, tr);
        }
    } else {
        switch (K) {
            case 1: return align_wave<1>(lo, L, sh, S, lane, cols_hyp, tr);
            case 2: return align_wave<2>(lo, L, sh, S, lane, cols_hyp, tr);
            case 4: return align_wave<4>(lo, L, sh, S, lane, cols_hyp, tr);
            default: return align_wave<8>(lo, L, sh, S, lane, cols_hyp, tr);
        }
    }
}

}  // namespace

// WIDE as in edit_stats_kernel.  The item's trace is stored only where its room holds it and m + d fits the ops' row; where
// la + lb exceeds the row (so that only the answer tells), a first pass without stores finds m + d.
template <bool WIDE>
__global__ __launch_bounds__(64) void edit_align_kernel(PoAlignArgs g) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t ao = g.a_off[p], bo = g.b_off[p];
    const int64_t la64 = g.a_len ? (int64_t)g.a_len[p] : g.a_off[p + 1] - ao;
    const int64_t lb64 = g.b_len ? (int64_t)g.b_len[p] : g.b_off[p + 1] - bo;
    const int64_t S64 = la64 <= lb64 ? la64 : lb64, L64 = la64 <= lb64 ? lb64 : la64;
    if (S64 < 0 || S64 > PO_EDIT_MAX_SHORT || L64 > PO_ACC_MAX_LONG) {
        if (WIDE && lane == 0) { g.dist[p] = -1; g.matches[p] = -1; g.ops_len[p] = -1; g.status[p] = S64 < 0 ? PO_E_ARG : PO_E_CAP; }
        return;
    }
    const bool cols_hyp = la64 <= lb64;   // the shorter string takes the lanes; the ops are the item's whichever it is
    const uint8_t* sh = cols_hyp ? g.a + ao : g.b + bo;
    const uint8_t* lo = cols_hyp ? g.b + bo : g.a + ao;
    const int S = (int)S64, L = (int)L64;
    const int K = po_ev_slot_class(po_ev_slots(S));
    if ((K > 8) != WIDE) return;
    const int64_t to = g.trace_off[p];
    const bool fits = g.trace_off[p + 1] - to >= po_aln_words(K, L);
    const bool sure = la64 + lb64 <= g.ops_stride;      // m + d <= la + lb
    int32_t d = 0, m = 0;
    for (int pass = fits && !sure ? 0 : 1; pass < 2; ++pass) {
        // what a pass starts from is opaque to the compiler here: otherwise it lifts the symbols' loads and every column's
        // constants of all three instantiations out of this loop and spills them
        int S_ = S, L_ = L, lane_ = lane;
        asm volatile("" : "+s"(S_), "+s"(L_), "+v"(lane_));
        const int32_t key = __builtin_amdgcn_readlane(align_any<WIDE>(K, lo, L_, sh, S_, lane_, cols_hyp, pass == 1 && fits ? g.trace + to : nullptr), S / K);
        d = po_acc_distance(key);
        m = po_acc_matches(key);
        if ((int64_t)m + d > g.ops_stride) break;
    }
    const bool ok = fits && (int64_t)m + d <= g.ops_stride;
    if (lane == 0) { g.dist[p] = d; g.matches[p] = m; g.ops_len[p] = ok ? m + d : -1; g.status[p] = ok ? PO_OK : PO_E_CAP; }
}

// One wave per pair whose ops_len says that its trace is there.  i, j, pos and the block's anchor are the same in every lane.
__global__ __launch_bounds__(64) void edit_walk_kernel(PoAlignArgs g) {
    const int p = blockIdx.x, lane = threadIdx.x;
    int pos = g.ops_len[p];
    if (pos <= 0) return;
    const int64_t la64 = g.a_len ? (int64_t)g.a_len[p] : g.a_off[p + 1] - g.a_off[p];
    const int64_t lb64 = g.b_len ? (int64_t)g.b_len[p] : g.b_off[p + 1] - g.b_off[p];
    const bool cols_hyp = la64 <= lb64;
    const int S = (int)(cols_hyp ? la64 : lb64), L = (int)(cols_hyp ? lb64 : la64);
    const po_aln_geom gm = po_aln_geometry(po_ev_slot_class(po_ev_slots(S)));
    const uint32_t* __restrict__ tr = g.trace + g.trace_off[p];
    uint8_t* out = g.ops + (int64_t)p * g.ops_stride;
    int i = L, j = S, i0 = 0, j0 = 0;     // i0 == 0: no block yet
    uint32_t w0 = 0, w1 = 0;
    while (pos > 0) {
        const int cnt = pos < PO_EV_WAVE ? pos : PO_EV_WAVE;
        uint32_t mine = 0;
        for (int q = 0; q < cnt; ++q) {
            uint32_t dir;
            if (i <= 0) dir = PO_ALN_DIR_LEFT;
            else if (j <= 0) dir = PO_ALN_DIR_UP;
            else {
                int ln = 0, which = 0, bit = 0;
                if (i0 == 0 || !po_aln_block_find(gm, i0, j0, i, j, &ln, &which, &bit)) {
                    i0 = i; j0 = j;
                    const int64_t at = po_aln_block_word(gm, i0, j0, lane);   // both words lie in the rows' groups: < po_aln_words
                    w0 = at >= 0 ? tr[at] : 0;
                    w1 = at >= 0 ? tr[at + 1] : 0;
                    po_aln_block_find(gm, i0, j0, i, j, &ln, &which, &bit);   // the anchor lies in its own block
                }
                const uint32_t w = which ? __builtin_amdgcn_readlane(w1, ln) : __builtin_amdgcn_readlane(w0, ln);
                dir = (w >> bit) & 3u;
            }
            po_aln_step(dir, &i, &j);
            if (lane == q) mine = po_aln_op(dir, cols_hyp);
        }
        if (lane < cnt) out[pos - 1 - lane] = (uint8_t)mine;   // 0 <= pos - 1 - lane < ops_len <= ops_stride
        pos -= cnt;
    }
}

__global__ __launch_bounds__(64) void edit_confusion_kernel(PoAlignArgs g) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n = g.ops_len[p];
    if (n < 0) return;
    const int64_t ao = g.a_off[p], bo = g.b_off[p];
    const int64_t la = g.a_len ? (int64_t)g.a_len[p] : g.a_off[p + 1] - ao;
    const int64_t lb = g.b_len ? (int64_t)g.b_len[p] : g.b_off[p + 1] - bo;
    const uint8_t* __restrict__ a = g.a + ao;
    const uint8_t* __restrict__ b = g.b + bo;
    const uint8_t* __restrict__ ops = g.ops + (int64_t)p * g.ops_stride;
    int32_t cnt[PO_ALN_CELLS];
    PO_EV_UNROLL
    for (int c = 0; c < PO_ALN_CELLS; ++c) cnt[c] = 0;
    int ha = 0, hb = 0;   // the symbols the columns before this step consumed
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int c0 = 0; c0 < n; c0 += PO_EV_WAVE) {
        const bool valid = c0 + lane < n;
        const uint32_t code = valid ? ops[c0 + lane] : 0u;
        const bool ua = valid && code != PO_ALN_D, ub = valid && code != PO_ALN_I;
        const uint64_t ma = __ballot(ua), mb = __ballot(ub);
        const int64_t ia = ha + po_ev_popc(ma & below), ib = hb + po_ev_popc(mb & below);
        const int x = ua && ia < la ? (int)a[ia] : 0xff, y = ub && ib < lb ? (int)b[ib] : 0xff;
        const int cell = valid ? po_aln_cell(code, x, y) : -1;
        PO_EV_UNROLL
        for (int c = 0; c < PO_ALN_CELLS; ++c) cnt[c] += cell == c ? 1 : 0;
        ha += po_ev_popc(ma);
        hb += po_ev_popc(mb);
    }
    int32_t mine = 0;
    PO_EV_UNROLL
    for (int c = 0; c < PO_ALN_CELLS; ++c) {
        const int32_t total = wave_sum(cnt[c]);
        if (lane == c) mine = total;
    }
    if (lane < PO_ALN_CELLS) g.confusion[(int64_t)p * PO_ALN_CELLS + lane] = mine;
}

extern "C" {

size_t po_edit_align_trace_words(int64_t la_max, int64_t lb_max) { return (size_t)po_aln_trace_words(la_max, lb_max); }

int po_edit_align(const uint8_t* a, const int64_t* a_off, const int32_t* a_len, const uint8_t* b, const int64_t* b_off,
                  const int32_t* b_len, int n, uint32_t* trace, const int64_t* trace_off, uint8_t* ops, int64_t ops_stride,
                  int32_t* ops_len, int32_t* dist, int32_t* matches, int32_t* confusion, int32_t* status, void* stream) {
    po_fail(PO_OK, "");
    const std::string w("po_edit_align");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (ops_stride < 0) return po_fail(PO_E_ARG, w + ": negative ops_stride");
    if (n == 0) return PO_OK;
    if (!a || !a_off || !b || !b_off || !trace || !trace_off || !ops || !ops_len || !dist || !matches || !status)
        return po_fail(PO_E_ARG, w + ": null a, a_off, b, b_off, trace, trace_off, ops, ops_len, dist, matches or status");
    const PoAlignArgs g = {a, a_off, a_len, b, b_off, b_len, trace, trace_off, ops, ops_stride, ops_len, dist, matches, confusion, status};
    hipLaunchKernelGGL(edit_align_kernel<false>, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    hipLaunchKernelGGL(edit_align_kernel<true>, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    hipLaunchKernelGGL(edit_walk_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    if (confusion) hipLaunchKernelGGL(edit_confusion_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// ------------------------------------------------------------------------------------------------------------ host buffers
// ops_h (n rows of ops_stride bytes) and confusion_h go up as they are, so that what the kernels leave untouched comes back
// as the caller had it; the trace is sized from the lengths and lives for the call.
int po_edit_align_h(const uint8_t* a_h, const int64_t* a_off_h, const int32_t* a_len_h, const uint8_t* b_h, const int64_t* b_off_h,
                    const int32_t* b_len_h, int n, uint8_t* ops_h, int64_t ops_stride, int32_t* ops_len_h, int32_t* dist_h,
                    int32_t* matches_h, int32_t* confusion_h, int32_t* status_h) {
    po_fail(PO_OK, "");
    const std::string w("po_edit_align_h");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (ops_stride < 0) return po_fail(PO_E_ARG, w + ": negative ops_stride");
    if (n == 0) return PO_OK;
    if (!a_off_h || !b_off_h || !ops_len_h || !dist_h || !matches_h || !status_h || (ops_stride > 0 && !ops_h))
        return po_fail(PO_E_ARG, w + ": null a_off, b_off, ops, ops_len, dist, matches or status");
    const PoRagged ra(a_off_h, n, true), rb(b_off_h, n, true);
    if (!ra.ordered || !rb.ordered) return po_fail(PO_E_ARG, w + ": " + (ra.ordered ? "b_off" : "a_off") + " decreases somewhere");
    for (int i = 0; i < n; ++i)   // a length table names a part of the item's room
        if ((a_len_h && (a_len_h[i] < 0 || a_len_h[i] > ra.off[i + 1] - ra.off[i])) || (b_len_h && (b_len_h[i] < 0 || b_len_h[i] > rb.off[i + 1] - rb.off[i])))
            return po_fail(PO_E_ARG, w + ": pair " + std::to_string(i) + " has a length outside its offsets' room");
    if ((ra.total > 0 && !a_h) || (rb.total > 0 && !b_h)) return po_fail(PO_E_ARG, w + ": null a or b");
    std::vector<int64_t> toff((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int64_t la = a_len_h ? a_len_h[i] : ra.off[i + 1] - ra.off[i], lb = b_len_h ? b_len_h[i] : rb.off[i + 1] - rb.off[i];
        const bool capped = std::min(la, lb) > PO_EDIT_MAX_SHORT || std::max(la, lb) > PO_ACC_MAX_LONG;
        toff[(size_t)i + 1] = toff[(size_t)i] + (capped ? 0 : po_aln_trace_words(la, lb));
    }
    const size_t M = (size_t)n * (size_t)ops_stride;
    PoRows a, b;
    PoDev al, bl, tr, to, op, ol, ds, mt, cf, st;
    PO_HIPCHK(a.up(a_h, ra, 1));
    PO_HIPCHK(b.up(b_h, rb, 1));
    if (a_len_h) PO_HIPCHK(al.up(a_len_h, sizeof(int32_t) * n));
    if (b_len_h) PO_HIPCHK(bl.up(b_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(tr.up(nullptr, sizeof(uint32_t) * (size_t)toff[(size_t)n]));
    PO_HIPCHK(to.up(toff.data(), sizeof(int64_t) * ((size_t)n + 1)));
    PO_HIPCHK(op.up(ops_h, M));
    PO_HIPCHK(ol.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(ds.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(mt.up(nullptr, sizeof(int32_t) * n));
    if (confusion_h) PO_HIPCHK(cf.up(confusion_h, sizeof(int32_t) * PO_ALN_CELLS * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    int rc = po_edit_align(a.data, a.off, a_len_h ? al.as<int32_t>() : nullptr, b.data, b.off, b_len_h ? bl.as<int32_t>() : nullptr, n,
                           tr, to, op, ops_stride, ol, ds, mt, confusion_h ? cf.as<int32_t>() : nullptr, st, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(op.down(ops_h, M));
    PO_HIPCHK(ol.down(ops_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(ds.down(dist_h, sizeof(int32_t) * n));
    PO_HIPCHK(mt.down(matches_h, sizeof(int32_t) * n));
    if (confusion_h) PO_HIPCHK(cf.down(confusion_h, sizeof(int32_t) * PO_ALN_CELLS * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

}  // extern "C"
