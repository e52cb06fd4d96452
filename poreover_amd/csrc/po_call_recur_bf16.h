// The GRU recurrence of `call --recurrence bf16x3`: h·U as three bf16 products with f32 sums.  Included by
// po_call.hip alone; the f32 kernel of po_call_kernels.h stays the default, and the trainer is not reached.
//
// Both operands are split in two bf16 values by the rule of po_bf16_rules.h, hh = bf16(h), hl = bf16(h - hh) and the same
// for U, and the product keeps three of the four terms:
//   h·U ~ hh·Uh + hl·Uh + hh·Ul          (hl·Ul, 2^-16 of the whole, is dropped)
// on v_mfma_f32_16x16x32_bf16, all three into the one f32 accumulator of a gate, k-block after k-block in this order.  A
// product of two bf16 values is exact in f32, so what is lost is the dropped term, the second rounding of each operand
// (2^-16) and the f32 sums.  One product, bf16(h)·bf16(U), loses 2^-9 per term through the rounding of U, and that error
// feeds back through time: §10.8 has the figures.
//
// gru_recur_x3_kernel<H> keeps gru_recur_body's structure: one workgroup per 16 windows and direction, H / 16 waves of 16
// units, one persistent launch per layer, one barrier per step, the f32 state in registers, the gates of gru_gates and
// the same stores.  What differs:
//   U     each lane reads its f32 values of U once, splits them and keeps Uh and Ul as B fragments (column = unit = lane & 15,
//         k = 32 kb + 8 (lane >> 4) + j): 3 gates x KP / 32 k-blocks x 2 x 4 VGPRs, the 96 of the f32 kernel at H = 128.
//         KP = H rounded up to 32; rows k >= H are zero, which is how H = 16, 48, 80 and 112 run.  No copy of U in memory.
//   h     goes through LDS as two bf16 arrays (hi, lo), double buffered, written by the lane that owns (window, unit) with
//         the hardware's round-to-nearest-even conversion; hl from h - float(hh), exact in f32.  Columns >= H and the rows of
//         windows past n are zeroed once and never written.  The A fragment (row = window = lane & 15, the same k as B) is one
//         ds_read_b128 per array and k-block: 8 per step at H = 128, where the f32 kernel issues 32 ds_read_b32.
//   rows  of KP + 16 bf16: 32 bytes of pad.  ds_read_b128 takes a wave as four groups of 16 lanes, and each group holds the
//         lanes of TWO k-quarters (lanes 0-3, 12-15 of one and 4-11 of the next).  With a row stride of 32 bytes modulo 64
//         the eight rows of a quarter land on the even 16-byte slots of the 256-byte bank row and the next quarter, 16
//         bytes on, on the odd ones: no conflict at any of the four KP.  (16 bytes of pad, the usual choice, leaves one
//         slot of each group 2-way.)
//
// Determinism: as for f32, every element is a function of its own window alone (fixed k order, rows never mix, zero rows
// and zero k add exact zeros), so a window's bits do not depend on batch, tile or pass.
#pragma once
#include "po_bf16_rules.h"
#include "po_call_bf16.h"
#include "po_call_kernels.h"

namespace {

typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

constexpr int X3_PAD = 16;   // bf16 of padding per LDS row (see above)
__host__ __device__ constexpr int x3_kp(int H) { return (H + 31) / 32 * 32; }

template <int H, bool REC>
__global__ __launch_bounds__(H * 4) void gru_recur_x3_kernel(RecurArgs a, float* rec) {
    constexpr int G = 3 * H, KP = x3_kp(H), KB = KP / 32, LS = KP + X3_PAD;
    __shared__ __attribute__((aligned(16))) __bf16 hs[2][2][RT][LS];   // [buffer][hi, lo][window][k]
    const RecurDir D = a.dir[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int unit = wave * 16 + i;
    const int w0 = blockIdx.x * RT;
    const int T = a.T;
    // this lane's B fragments for every k-block and gate, hi and lo: U[32 kb + 8 kq + j][g * H + unit], zero past H
    bf16x8 uh[3][KB], ul[3][KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            float uf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * kb + 8 * kq + j;
                uf[j] = k < H ? D.U[k * G + g * H + unit] : 0.f;
            }
            u16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint16_t bh, bl;
                po_bf16_split(uf[j], &bh, &bl);
                hi[j] = bh;
                lo[j] = bl;
            }
            uh[g][kb] = __builtin_bit_cast(bf16x8, hi);
            ul[g][kb] = __builtin_bit_cast(bf16x8, lo);
        }
    float br[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) br[g] = D.brec[g * H + unit];
    for (int e = threadIdx.x; e < 2 * 2 * RT * LS / 2; e += blockDim.x) reinterpret_cast<uint32_t*>(&hs[0][0][0][0])[e] = 0u;
    float h[4] = {0.f, 0.f, 0.f, 0.f};     // (window w0 + kq * 4 + r, unit): the lane's own slice of the state
    bool live[4];
    const float* prow[4];
    float* orow[4];
    float* rrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int w = w0 + kq * 4 + r;
        live[r] = w < a.n;
        prow[r] = D.P + (int64_t)(live[r] ? w : 0) * T * G + unit;
        orow[r] = a.out + (int64_t)(live[r] ? w : 0) * T * a.out_stride + D.col + unit;
        rrow[r] = REC ? rec + ((int64_t)blockIdx.y * a.n + (live[r] ? w : 0)) * T * G + unit : nullptr;
    }
    __syncthreads();
    for (int s = 0; s < T; ++s) {
        const int t = D.backward ? T - 1 - s : s;
        const int to = D.rev_out ? s : t;
        const int cur = s & 1;
        float px[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int g = 0; g < 3; ++g) px[r][g] = live[r] ? prow[r][(int64_t)t * G + g * H] : 0.f;
        f32x4 acc[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&hs[cur][0][i][32 * kb + 8 * kq]);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(&hs[cur][1][i][32 * kb + 8 * kq]);
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, uh[g][kb], acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, uh[g][kb], acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, ul[g][kb], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float z, rg, hc, hn;
            gru_gates(px[r], acc[0][r], acc[1][r], acc[2][r], br, h[r], z, rg, hc, hn);
            if (live[r]) {
                if (REC) {
#pragma unroll
                    for (int g = 0; g < 3; ++g) rrow[r][(int64_t)t * G + g * H] = acc[g][r] + br[g];
                }
                h[r] = hn;
                const __bf16 hh = (__bf16)hn;          // v_cvt_pk_bf16_f32: round to nearest even
                hs[cur ^ 1][0][kq * 4 + r][unit] = hh;
                hs[cur ^ 1][1][kq * 4 + r][unit] = (__bf16)(hn - (float)hh);   // (exact in f32)
                orow[r][(int64_t)to * a.out_stride] = hn;
            }
        }
        __syncthreads();
    }
}

// the recurrence of one GRU layer on `stream`, by the kernel of `precision` (PO_RECUR_*, checked by the caller); rec: where
// the recurrent pre-activations go ([nd][n * T][3 H]; the stage entry alone), or null
inline void launch_gru_recur(hipStream_t stream, int H, int nd, const RecurArgs& ra, int precision, float* rec) {
    const dim3 grid((unsigned)((ra.n + RT - 1) / RT), (unsigned)nd);
    if (precision == PO_RECUR_BF16X3) {
        if (rec) {
            PO_FOR_UNITS(H, hipLaunchKernelGGL((gru_recur_x3_kernel<HH, true>), grid, dim3(HH * 4), 0, stream, ra, rec));
        } else {
            PO_FOR_UNITS(H, hipLaunchKernelGGL((gru_recur_x3_kernel<HH, false>), grid, dim3(HH * 4), 0, stream, ra, (float*)nullptr));
        }
    } else if (rec) {
        PO_FOR_UNITS(H, hipLaunchKernelGGL(gru_recur_rec_kernel<HH>, grid, dim3(HH * 4), 0, stream, ra, rec));
    } else {
        PO_FOR_UNITS(H, hipLaunchKernelGGL(gru_recur_kernel<HH>, grid, dim3(HH * 4), 0, stream, ra));
    }
}

}  // namespace
