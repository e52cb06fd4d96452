// The two kernels under tensors.accuracy (the rules are po_acc_rules.h's, which tools/acc_check.cpp holds
// against brute force).  They sit beside po_eval.hip's and keep its design:
//
//   logits_path_kernel   one wave per item, 64 frames a step: the class of the first maximum of the frame's 5 raw values, read
//                        where they lie (po_ingest_item tables, any strides, f32 / f16 / bf16 / f64), the codes of the
//                        emitting frames compacted in frame order by a ballot and a carried count.  For the bonito kind a
//                        frame also sees its left neighbour's class, lane 0 the class carried over the block's edge.
//   edit_stats_kernel    one wave per pair: edit_distance_kernel's layout on the packed key d * 4096 - m, so that the
//                        matches m of the best alignment of minimum distance d come out with d.  The shorter string's columns
//                        on the lanes, K = 1, 2, 4 .. 64 columns per lane in registers, in two kernels (K <= 8, K >= 16).
//
// No atomics, no LDS, one writer per value, nothing depends on the launch geometry or the batch position.  The entries are
// enqueue-only: no allocation, no synchronisation, no host read of device memory.  The *_h twins reach them from host arrays.
#include <string>
#include <vector>

#include "po_acc_rules.h"
#include "po_hostbuf.h"

static_assert(PO_ACC_F32 == PO_DTYPE_F32 && PO_ACC_F16 == PO_DTYPE_F16 && PO_ACC_BF16 == PO_DTYPE_BF16 && PO_ACC_F64 == PO_DTYPE_F64,
              "po_acc_rules.h's dtypes are the header's");
static_assert(PO_ACC_POREOVER == PO_KIND_POREOVER && PO_ACC_BONITO == PO_KIND_BONITO, "po_acc_rules.h's kinds are the header's");
static_assert(PO_ACC_MAX_LONG == PO_EDIT_STATS_MAX_LONG, "the header's cap is the rules'");

struct PoPathArgs {
    const po_ingest_item* items; const int64_t* row_off; int dtype, kind;
    int perm[PO_ACC_CLASSES];
    uint8_t* pred; int64_t pred_stride; int32_t* pred_len;
};

__global__ __launch_bounds__(64) void logits_path_kernel(PoPathArgs g) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int64_t T = g.row_off[w + 1] - g.row_off[w];
    if (T < 0 || T > g.pred_stride) {   // the row cannot hold the item: nothing of it is written
        if (lane == 0) g.pred_len[w] = -1;
        return;
    }
    const po_ingest_item it = g.items[w];
    uint8_t* out = g.pred + (int64_t)w * g.pred_stride;
    int carry = 0, edge = PO_ACC_NO_PREV;
    for (int64_t t0 = 0; t0 < T; t0 += PO_EV_WAVE) {
        const int64_t t = t0 + lane;
        const int c = t < T ? po_acc_frame_class(it.base, it.row_stride, it.col_stride, t, g.dtype, g.perm) : PO_ACC_BLANK;
        const int prev = __builtin_amdgcn_update_dpp(edge, c, 0x138, 0xf, 0xf, false);   // wave_shr:1; lane 0 keeps `edge`
        const uint64_t keep = __ballot(po_acc_emit(g.kind, c, prev));
        int pos;
        if (po_ev_path_slot(keep, lane, carry, &pos)) out[pos] = (uint8_t)c;   // pos < the frames seen so far <= T <= pred_stride
        carry += po_ev_popc(keep);
        edge = __builtin_amdgcn_readlane(c, PO_EV_WAVE - 1);   // (read only where a next block exists: lane 63 held a frame then)
    }
    if (lane == 0) g.pred_len[w] = carry;
}

namespace {

// po_ev_wave_excl_min, a move per step (po_eval.hip's); a lane without a source keeps the identity.  Every lane is active.
__device__ __forceinline__ int32_t wave_excl_min(int32_t v) {
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x138, 0xf, 0xf, false);               // wave_shr:1
}

// the key of lo[0..L) against sh[0..S), S <= 64 K - 1, in the lane that holds column S
template <int K>
__device__ __forceinline__ int32_t stats_wave(const uint8_t* __restrict__ lo, int L, const uint8_t* __restrict__ sh, int S,
                                              int lane) {
    int32_t row[K];
    uint32_t sym[(K + 3) / 4];
    po_ev_load_symbols<K>(sym, sh, S, lane);
    po_acc_row_init<K>(row, lane);
    int32_t diag = po_acc_diag_init<K>(lane);
    for (int i0 = 0; i0 < L; i0 += PO_EV_WAVE) {
        const int xs = i0 + lane < L ? (int)lo[i0 + lane] : 0;
        const int m = L - i0 < PO_EV_WAVE ? L - i0 : PO_EV_WAVE;
        for (int r = 0; r < m; ++r) {
            const int x = __builtin_amdgcn_readlane(xs, r);
            const int32_t total = po_acc_row_local<K>(row, sym, diag, x, i0 + r + 1, lane);
            diag = po_acc_row_finish<K>(row, wave_excl_min(total), lane);
        }
    }
    return po_ev_row_pick<K>(row, S);
}

}  // namespace

struct PoStatsArgs {
    const uint8_t* a; const int64_t* a_off; const int32_t* a_len;
    const uint8_t* b; const int64_t* b_off; const int32_t* b_len;
    int32_t* dist; int32_t* matches; int32_t* status;
};

// WIDE as in edit_distance_kernel: false answers the pairs of K <= 8 columns per lane, true those of 16, 32 and 64 and the
// refusals; both are launched over the batch and a wave leaves a pair that is the other's.
template <bool WIDE>
__global__ __launch_bounds__(64) void edit_stats_kernel(PoStatsArgs g) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t ao = g.a_off[p], bo = g.b_off[p];
    const int64_t la64 = g.a_len ? (int64_t)g.a_len[p] : g.a_off[p + 1] - ao;
    const int64_t lb64 = g.b_len ? (int64_t)g.b_len[p] : g.b_off[p + 1] - bo;
    const int64_t S64 = la64 <= lb64 ? la64 : lb64, L64 = la64 <= lb64 ? lb64 : la64;
    if (S64 < 0 || S64 > PO_EDIT_MAX_SHORT || L64 > PO_ACC_MAX_LONG) {
        if (WIDE && lane == 0) { g.dist[p] = -1; g.matches[p] = -1; g.status[p] = S64 < 0 ? PO_E_ARG : PO_E_CAP; }
        return;
    }
    // distance and matches are symmetric: the shorter string takes the lanes
    const bool a_short = la64 <= lb64;
    const uint8_t* sh = a_short ? g.a + ao : g.b + bo;
    const uint8_t* lo = a_short ? g.b + bo : g.a + ao;
    const int S = (int)S64, L = (int)L64;
    const int K = po_ev_slot_class(po_ev_slots(S));
    if ((K > 8) != WIDE) return;
    int32_t key;
    if constexpr (WIDE) {
        switch (K) {
            case 16: key = stats_wave<16>(lo, L, sh, S, lane); break;
            case 32: key = stats_wave<32>(lo, L, sh, S, lane); break;
            default: key = stats_wave<PO_EV_MAX_SLOTS>(lo, L, sh, S, lane); break;
        }
    } else {
        switch (K) {
            case 1: key = stats_wave<1>(lo, L, sh, S, lane); break;
            case 2: key = stats_wave<2>(lo, L, sh, S, lane); break;
            case 4: key = stats_wave<4>(lo, L, sh, S, lane); break;
            default: key = stats_wave<8>(lo, L, sh, S, lane); break;
        }
    }
    if (lane == S / K) { g.dist[p] = po_acc_distance(key); g.matches[p] = po_acc_matches(key); g.status[p] = PO_OK; }
}

namespace {

// the refusals of po_logits_path and its twin that need no lengths
int path_check(const std::string& w, int n, int C, int dtype, const int* perm_h, int kind, int64_t pred_stride) {
    if (kind == PO_KIND_FLIPFLOP) return po_fail(PO_E_UNSUPPORTED, w + ": the flip-flop kind has no argmax path here");
    if (kind != PO_KIND_POREOVER && kind != PO_KIND_BONITO) return po_fail(PO_E_ARG, w + ": unknown kind");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (C != PO_ACC_CLASSES) return po_fail(PO_E_ARG, w + ": C must be 5");
    if (dtype < PO_DTYPE_F32 || dtype > PO_DTYPE_F64) return po_fail(PO_E_ARG, w + ": unknown dtype");
    if (perm_h) {
        unsigned seen = 0;
        for (int c = 0; c < C; ++c) {
            if (perm_h[c] < 0 || perm_h[c] >= C) return po_fail(PO_E_ARG, w + ": perm entry outside [0, C)");
            seen |= 1u << perm_h[c];
        }
        if (seen != (1u << C) - 1) return po_fail(PO_E_ARG, w + ": perm must name every column once");
    }
    if (pred_stride < 0) return po_fail(PO_E_ARG, w + ": negative pred_stride");
    return PO_OK;
}

}  // namespace

extern "C" {

int po_logits_path(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, const int* perm_h, int kind,
                   uint8_t* pred, int64_t pred_stride, int32_t* pred_len, void* stream) {
    po_fail(PO_OK, "");
    const std::string w("po_logits_path");
    int rc = path_check(w, n, C, dtype, perm_h, kind, pred_stride);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;
    if (!items || !row_off || !pred_len || (pred_stride > 0 && !pred)) return po_fail(PO_E_ARG, w + ": null items, row_off, pred or pred_len");
    PoPathArgs g;
    g.items = items; g.row_off = row_off; g.dtype = dtype; g.kind = kind;
    for (int c = 0; c < PO_ACC_CLASSES; ++c) g.perm[c] = perm_h ? perm_h[c] : c;
    g.pred = pred; g.pred_stride = pred_stride; g.pred_len = pred_len;
    hipLaunchKernelGGL(logits_path_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

int po_edit_stats(const uint8_t* a, const int64_t* a_off, const int32_t* a_len, const uint8_t* b, const int64_t* b_off,
                  const int32_t* b_len, int n, int32_t* dist, int32_t* matches, int32_t* status, void* stream) {
    po_fail(PO_OK, "");
    const std::string w("po_edit_stats");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (n == 0) return PO_OK;
    if (!a || !a_off || !b || !b_off || !dist || !matches || !status)
        return po_fail(PO_E_ARG, w + ": null a, a_off, b, b_off, dist, matches or status");
    const PoStatsArgs g = {a, a_off, a_len, b, b_off, b_len, dist, matches, status};
    hipLaunchKernelGGL(edit_stats_kernel<false>, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    hipLaunchKernelGGL(edit_stats_kernel<true>, dim3(n), dim3(64), 0, (hipStream_t)stream, g);
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// ------------------------------------------------------------------------------------------------------------ host buffers
int po_logits_path_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                     const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, const int* perm_h, int kind,
                     uint8_t* pred_h, int64_t pred_stride, int32_t* pred_len_h) {
    po_fail(PO_OK, "");
    const std::string w("po_logits_path_h");
    int rc = path_check(w, n, C, dtype, perm_h, kind, pred_stride);
    if (rc != PO_OK) return rc;
    if (n == 0) return PO_OK;
    if (!row_off_h || !item_off_h || !row_stride_h || !col_stride_h || !pred_len_h)
        return po_fail(PO_E_ARG, w + ": null item table, row_off or pred_len");
    if (row_off_h[0] != 0) return po_fail(PO_E_ARG, w + ": row_off[0] must be 0");
    for (int i = 0; i < n; ++i) {
        const int64_t T = row_off_h[i + 1] - row_off_h[i];
        if (T < 0 || T > 0x7fffffff) return po_fail(PO_E_ARG, w + ": offsets must not decrease (an item has fewer than 2^31 frames)");
        if (T > pred_stride)
            return po_fail(PO_E_ARG, w + ": item " + std::to_string(i) + " has " + std::to_string(T) + " frames, pred_stride is " + std::to_string(pred_stride));
        if (item_off_h[i] < 0 || row_stride_h[i] < 0 || col_stride_h[i] < 0) return po_fail(PO_E_ARG, w + ": negative offset or stride");
        if (T > 0 && (src_elems <= 0 || (T > 1 && row_stride_h[i] > (src_elems - 1) / (T - 1)) || col_stride_h[i] > (src_elems - 1) / (C - 1) ||
                      item_off_h[i] + (T - 1) * row_stride_h[i] + (C - 1) * col_stride_h[i] >= src_elems))
            return po_fail(PO_E_ARG, w + ": item " + std::to_string(i) + " reaches past src_elems");
    }
    if ((row_off_h[n] > 0 && !src_h) || (pred_stride > 0 && !pred_h)) return po_fail(PO_E_ARG, w + ": null src or pred");
    const size_t eb = (size_t)po_acc_elem_bytes(dtype), M = (size_t)n * (size_t)pred_stride;
    std::vector<po_ingest_item> items(n);
    PoDev src, it, ro, pd, pl;
    PO_HIPCHK(src.up(src_h, (size_t)std::max<int64_t>(src_elems, 0) * eb));
    for (int i = 0; i < n; ++i) items[i] = {src.as<char>() + (size_t)item_off_h[i] * eb, row_stride_h[i], col_stride_h[i]};
    PO_HIPCHK(it.up(items.data(), sizeof(po_ingest_item) * n));
    PO_HIPCHK(ro.up(row_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(pd.up(nullptr, M));
    PO_HIPCHK(hipMemset(pd.p, 0, std::max<size_t>(M, 256)));
    PO_HIPCHK(pl.up(nullptr, sizeof(int32_t) * n));
    rc = po_logits_path(it.as<po_ingest_item>(), ro, n, C, dtype, perm_h, kind, pd, pred_stride, pl, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(pd.down(pred_h, M));
    PO_HIPCHK(pl.down(pred_len_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_edit_stats_h(const uint8_t* a_h, const int64_t* a_off_h, const int32_t* a_len_h, const uint8_t* b_h, const int64_t* b_off_h,
                    const int32_t* b_len_h, int n, int32_t* dist_h, int32_t* matches_h, int32_t* status_h) {
    po_fail(PO_OK, "");
    const std::string w("po_edit_stats_h");
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (n == 0) return PO_OK;
    if (!a_off_h || !b_off_h || !dist_h || !matches_h || !status_h) return po_fail(PO_E_ARG, w + ": null a_off, b_off, dist, matches or status");
    const PoRagged ra(a_off_h, n, true), rb(b_off_h, n, true);
    if (!ra.ordered || !rb.ordered) return po_fail(PO_E_ARG, w + ": " + (ra.ordered ? "b_off" : "a_off") + " decreases somewhere");
    for (int i = 0; i < n; ++i)   // a length table names a part of the item's room
        if ((a_len_h && (a_len_h[i] < 0 || a_len_h[i] > ra.off[i + 1] - ra.off[i])) || (b_len_h && (b_len_h[i] < 0 || b_len_h[i] > rb.off[i + 1] - rb.off[i])))
            return po_fail(PO_E_ARG, w + ": pair " + std::to_string(i) + " has a length outside its offsets' room");
    if ((ra.total > 0 && !a_h) || (rb.total > 0 && !b_h)) return po_fail(PO_E_ARG, w + ": null a or b");
    PoRows a, b;
    PoDev al, bl, ds, mt, st;
    PO_HIPCHK(a.up(a_h, ra, 1));
    PO_HIPCHK(b.up(b_h, rb, 1));
    if (a_len_h) PO_HIPCHK(al.up(a_len_h, sizeof(int32_t) * n));
    if (b_len_h) PO_HIPCHK(bl.up(b_len_h, sizeof(int32_t) * n));
    PO_HIPCHK(ds.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(mt.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    int rc = po_edit_stats(a.data, a.off, a_len_h ? al.as<int32_t>() : nullptr, b.data, b.off, b_len_h ? bl.as<int32_t>() : nullptr, n,
                           ds, mt, st, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ds.down(dist_h, sizeof(int32_t) * n));
    PO_HIPCHK(mt.down(matches_h, sizeof(int32_t) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

}  // extern "C"
