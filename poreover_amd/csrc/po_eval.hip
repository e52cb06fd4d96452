// The two integer stages of `train`'s held-out validation (the rules are po_eval_rules.h's, which
// tools/eval_check.cpp holds against brute force):
//
//   eval_path_kernel      one wave per window, 64 frames a step: np.argmax of the frame's 5 probabilities, the non-blank
//                         codes compacted in frame order by a ballot and a carried count
//   edit_distance_kernel  one wave per pair: unit-cost Levenshtein, int32.  The shorter string's columns 0..S sit on the
//                         lanes, K = 1, 2, 4 .. 64 consecutive columns per lane in registers (one instantiation per K,
//                         chosen per pair, in two kernels: K <= 8 and K >= 16); the longer string is walked by rows, 64
//                         of its symbols fetched at a time.  A row is each lane's pass over its own columns, one exclusive
//                         prefix minimum across the wave (six data-parallel moves and a shift, no LDS) and a second pass;
//                         nothing else crosses lanes.
//
// No atomics, no LDS, one writer per value, nothing depends on the launch geometry or the batch position.
#include <string>

#include "po_eval_rules.h"
#include "po_hostbuf.h"

__global__ __launch_bounds__(64) void eval_path_kernel(const float* __restrict__ probs, int T, uint8_t* __restrict__ pred,
                                                       int32_t* __restrict__ pred_len) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const float* pw = probs + (int64_t)w * T * PO_EV_CLASSES;
    uint8_t* out = pred + (int64_t)w * T;
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += PO_EV_WAVE) {
        const int t = t0 + lane;
        int c = PO_EV_BLANK;
        if (t < T) {
            float p[PO_EV_CLASSES];
#pragma unroll
            for (int k = 0; k < PO_EV_CLASSES; ++k) p[k] = pw[(int64_t)t * PO_EV_CLASSES + k];
            c = po_ev_argmax(p);
        }
        const uint64_t keep = __ballot(c != PO_EV_BLANK);
        int pos;
        if (po_ev_path_slot(keep, lane, carry, &pos)) out[pos] = (uint8_t)c;   // pos < the frames seen so far <= T
        carry += po_ev_popc(keep);
    }
    if (lane == 0) pred_len[w] = carry;
}

namespace {

// po_ev_wave_excl_min, a move per step; a lane without a source keeps the identity.  Every lane of the wave is active.
__device__ __forceinline__ int32_t wave_excl_min(int32_t v) {
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = po_ev_min(v, __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_update_dpp(PO_EV_INF, v, 0x138, 0xf, 0xf, false);               // wave_shr:1
}

// D[L][S] of lo[0..L) against sh[0..S), S <= 64 K - 1, in the lane that holds column S
template <int K>
__device__ __forceinline__ int32_t edit_wave(const uint8_t* __restrict__ lo, int L, const uint8_t* __restrict__ sh, int S,
                                             int lane) {
    int32_t row[K];
    uint32_t sym[(K + 3) / 4];
    po_ev_load_symbols<K>(sym, sh, S, lane);
    po_ev_row_init<K>(row, lane);
    int32_t diag = lane * K - 1;
    for (int i0 = 0; i0 < L; i0 += PO_EV_WAVE) {
        const int xs = i0 + lane < L ? (int)lo[i0 + lane] : 0;
        const int m = L - i0 < PO_EV_WAVE ? L - i0 : PO_EV_WAVE;
        for (int r = 0; r < m; ++r) {
            const int x = __builtin_amdgcn_readlane(xs, r);
            const int32_t total = po_ev_row_local<K>(row, sym, diag, x, i0 + r + 1, lane);
            diag = po_ev_row_finish<K>(row, wave_excl_min(total), lane);
        }
    }
    return po_ev_row_pick<K>(row, S);
}

}  // namespace

struct PoEditArgs {
    const uint8_t* a; const int64_t* a_off; const int32_t* a_len;
    const uint8_t* b; const int64_t* b_off;
    int32_t* dist; int32_t* status;
};

// WIDE = false answers the pairs of K <= 8 columns per lane, WIDE = true those of 16, 32 and 64 (the registers of the widest
// instantiation set the occupancy of a kernel): both are launched over the batch and a wave leaves a pair that is the other's.
template <bool WIDE>
__global__ __launch_bounds__(64) void edit_distance_kernel(PoEditArgs g) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t ao = g.a_off[p], bo = g.b_off[p];
    const int la = g.a_len ? g.a_len[p] : (int)(g.a_off[p + 1] - ao);
    const int lb = (int)(g.b_off[p + 1] - bo);
    // the distance is symmetric: the shorter string takes the lanes
    const bool a_short = la <= lb;
    const uint8_t* sh = a_short ? g.a + ao : g.b + bo;
    const uint8_t* lo = a_short ? g.b + bo : g.a + ao;
    const int S = a_short ? la : lb, L = a_short ? lb : la;
    if (S > PO_EDIT_MAX_SHORT) {
        if (WIDE && lane == 0) { g.dist[p] = -1; g.status[p] = PO_E_CAP; }
        return;
    }
    const int K = po_ev_slot_class(po_ev_slots(S));
    if ((K > 8) != WIDE) return;
    int32_t d;
    if constexpr (WIDE) {
        switch (K) {
            case 16: d = edit_wave<16>(lo, L, sh, S, lane); break;
            case 32: d = edit_wave<32>(lo, L, sh, S, lane); break;
            default: d = edit_wave<PO_EV_MAX_SLOTS>(lo, L, sh, S, lane); break;
        }
    } else {
        switch (K) {
            case 1: d = edit_wave<1>(lo, L, sh, S, lane); break;
            case 2: d = edit_wave<2>(lo, L, sh, S, lane); break;
            case 4: d = edit_wave<4>(lo, L, sh, S, lane); break;
            default: d = edit_wave<8>(lo, L, sh, S, lane); break;
        }
    }
    if (lane == S / K) { g.dist[p] = d; g.status[p] = PO_OK; }
}

extern "C" {

int po_launch_eval_path(const float* probs, int n, int T, uint8_t* pred, int32_t* pred_len, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    hipLaunchKernelGGL(eval_path_kernel, dim3(n), dim3(64), 0, stream, probs, T, pred, pred_len);
    return PO_OK;
}

int po_launch_edit_distance(const uint8_t* a, const int64_t* a_off, const int32_t* a_len, const uint8_t* b,
                            const int64_t* b_off, int n, int32_t* dist, int32_t* status, hipStream_t stream) {
    if (n <= 0) return PO_OK;
    PoEditArgs g = {a, a_off, a_len, b, b_off, dist, status};
    hipLaunchKernelGGL(edit_distance_kernel<false>, dim3(n), dim3(64), 0, stream, g);
    hipLaunchKernelGGL(edit_distance_kernel<true>, dim3(n), dim3(64), 0, stream, g);
    return PO_OK;
}

// ------------------------------------------------------------------------------------------------------------ host buffers
int po_eval_path_h(const float* probs_h, int n, int T, uint8_t* pred_h, int32_t* pred_len_h) {
    const char* me = "po_eval_path_h";
    po_set_error("");
    if (n < 0 || T < 1) return po_fail(PO_E_ARG, std::string(me) + ": n " + std::to_string(n) + ", T " + std::to_string(T));
    if (n == 0) return PO_OK;
    if (!probs_h || !pred_h || !pred_len_h) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    const size_t M = (size_t)n * T;
    PoDev pr, pd, pl;
    PO_HIPCHK(pr.up(probs_h, M * PO_EV_CLASSES * sizeof(float)));
    PO_HIPCHK(pd.up(nullptr, M));
    PO_HIPCHK(hipMemset(pd.p, 0, std::max<size_t>(M, 256)));
    PO_HIPCHK(pl.up(nullptr, sizeof(int32_t) * n));
    po_launch_eval_path(pr, n, T, pd, pl, nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(pd.down(pred_h, M));
    PO_HIPCHK(pl.down(pred_len_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_edit_distance_batch_h(const uint8_t* a_h, const int64_t* a_off_h, const uint8_t* b_h, const int64_t* b_off_h, int n,
                             int32_t* dist_h, int32_t* status_h) {
    const char* me = "po_edit_distance_batch_h";
    po_set_error("");
    if (n < 0) return po_fail(PO_E_ARG, std::string(me) + ": n " + std::to_string(n));
    if (n == 0) return PO_OK;
    if (!a_off_h || !b_off_h || !dist_h || !status_h) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    const PoRagged ra(a_off_h, n, true), rb(b_off_h, n, true);
    if (!ra.ordered || !rb.ordered)
        return po_fail(PO_E_ARG, std::string(me) + ": " + (ra.ordered ? "b_off" : "a_off") + " decreases somewhere");
    if (ra.max + rb.max >= ((int64_t)1 << 30))
        return po_fail(PO_E_ARG, std::string(me) + ": a pair of " + std::to_string(ra.max) + " and " + std::to_string(rb.max) +
                       " symbols (the distance is an int32: the two lengths must sum to less than 2^30)");
    if ((ra.total > 0 && !a_h) || (rb.total > 0 && !b_h)) return po_fail(PO_E_ARG, std::string(me) + ": null argument");
    PoRows a, b;
    PoDev ds, st;
    PO_HIPCHK(a.up(a_h, ra, 1));
    PO_HIPCHK(b.up(b_h, rb, 1));
    PO_HIPCHK(ds.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    po_launch_edit_distance(a.data, a.off, nullptr, b.data, b.off, n, ds, st, nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ds.down(dist_h, sizeof(int32_t) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

}  // extern "C"
