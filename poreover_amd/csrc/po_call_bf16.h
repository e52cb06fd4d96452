// The GRU input projection of `call --precision bf16`: bf16 operands, f32 products and sums.  Included
// by po_call.hip and, through po_train_bf16.h, by po_train.hip: a trainer set to PO_CALL_BF16 (po_train_set_precision,
// DESIGN.md §11.2) runs this same projection in its forward pass, so its logits are `call`'s bits.  The f32 kernels of
// po_call_kernels.h stay both files' default.
//
//   w_to_bf16_kernel      a GRU layer's W[d][k][c] (f32, rows of 384) rounded by the rule of po_bf16_rules.h into
//                         Wb[d][c][Kp] (bf16, TRANSPOSED: k runs fastest; Kp = cin rounded up to 32, zeros past cin), so that
//                         an MFMA B fragment (8 consecutive k of one column) is 16 contiguous bytes
//   gru_proj_bf16_kernel  P[d][m][c] = sum_k bf16(x[m][k]) * Wb[d][c][k] + b_in[d][c] on v_mfma_f32_16x16x32_bf16
//
// The MFMA shape.  16x16x32 and not 32x32x16: (a) its C layout (column on lane & 15, rows 4 (lane >> 4) + r) is the one the
// f32 kernel and gru_recur_kernel already use, so the store pattern of P is unchanged; (b) a wave's 16 rows x 192 columns
// are 12 accumulators of 4 registers (48 VGPRs) where the 32 x 32 shape needs 96 for 32 x 192, which with the x prefetch
// would leave no room for two waves per SIMD; (c) a lane's A fragment is 8 consecutive k of one row: 32 contiguous bytes
// of the f32 x row, two 16-byte loads.
//
// The shape of the launch.  A workgroup (8 waves) owns one direction and one HALF of its 384 columns (192) for the whole
// launch and keeps that half of Wb in LDS, read from global memory once per workgroup and K panel; it then walks row tiles
// of 128 rows (16 per wave) with the stride of the grid.  Per row tile a wave reads its 16 x rows once from global memory
// (f32, rounded to bf16 in registers by the hardware's packed conversion, the next 32 k prefetched under the MFMAs of the
// current) and its B fragments from LDS (ds_read_b128; rows of Kp + 8 bf16 = 16 bytes of pad, so that the 16 columns of a
// fragment start 4 banks apart).  The 2 x ndir workgroups that share a row tile are neighbours in the grid, so its x rows
// reach HBM once and the other readers find them in the caches.  One direction's 256 x 384 bf16 is 196 KB and does not
// fit the 160 KB of LDS: hence the halves.
//
// cin above PK = 256 is walked in K panels: panel after panel is staged in LDS and every row tile is passed once per
// panel, the partial sums carried through P itself (read back as the MFMA's C input: the same f32 chain as in registers,
// so the bits do not depend on the panel size).  The bias is added after the last panel.
//
// Determinism: an output row's value is a function of its own x row alone — the k order is fixed (32 at a time in
// ascending order, the MFMA's own order inside), rows never mix (each is one row of an A fragment), and a zero row or a
// zero k past cin adds exact zeros.  So a window's bits do not depend on batch, tile or pass, as for f32.
#pragma once
#include "po_bf16_rules.h"
#include "po_call_kernels.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int G = G_MAX;            // these kernels are built for 128 units alone (po_call_batch refuses the others)
constexpr int BF_CH = G / 2;        // columns a workgroup owns (one half of a direction)
constexpr int BF_CT = BF_CH / 16;   // 12 column tiles per wave
constexpr int BF_PK = 256;          // k per LDS panel
constexpr int BF_LS = BF_PK + 8;    // LDS row stride in bf16 (16 bytes of pad)
constexpr int BF_WAVES = 8;
constexpr int BF_BM = BF_WAVES * 16;   // rows per tile

__host__ __device__ inline int bf_kp(int cin) { return (cin + 31) / 32 * 32; }
// bf16 elements of a GRU layer's converted kernels
inline size_t bf_w_elems(int cin, int ndir) { return (size_t)ndir * G * bf_kp(cin); }

// Wb[d][c][k] = bf16(W[d][k][c]) for k < cin, 0 for cin <= k < Kp.  wstride: f32 elements between the directions' W.
__global__ __launch_bounds__(256) void w_to_bf16_kernel(const float* __restrict__ W, int64_t wstride, int cin, int ndir,
                                                        uint16_t* __restrict__ Wb) {
    const int Kp = bf_kp(cin);
    const int64_t total = (int64_t)ndir * G * Kp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        // e walks the INPUT order (d, k, c): coalesced reads; the writes are 2 bytes apart by Kp (the matrix is small)
        const int c = (int)(e % G);
        const int k = (int)((e / G) % Kp);
        const int d = (int)(e / ((int64_t)G * Kp));
        const uint16_t v = k < cin ? po_bf16_from_f32(W[d * wstride + (int64_t)k * G + c]) : (uint16_t)0;
        Wb[((int64_t)d * G + c) * Kp + k] = v;
    }
}

// the lane's A fragment: xk[0 .. 8) = x[row][k .. k + 8), zero past cin and for a row past M
template <bool VEC>
__device__ __forceinline__ void bf_load_a(const float* __restrict__ xk, bool row_ok, int k, int cin, float (&a)[8]) {
    if (VEC) {   // cin % 4 == 0: every 4 consecutive k from a multiple of 4 are 16-byte aligned and wholly inside or outside
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row_ok && k + 4 * h < cin) v = *reinterpret_cast<const f32x4*>(xk + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[4 * h + j] = v[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (row_ok && k + j < cin) ? xk[j] : 0.f;
    }
}

__device__ __forceinline__ bf16x8 bf_pack(const float (&a)[8]) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)a[j];   // v_cvt_pk_bf16_f32: round to nearest even
    return r;
}

template <bool VEC>
__device__ __forceinline__ void gru_proj_bf16_body(const float* __restrict__ x, int cin, const uint16_t* __restrict__ Wb,
                                                   const float* __restrict__ bin, int64_t bstride, float* __restrict__ P,
                                                   int64_t M, int ndir, uint16_t* wl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int nq = 2 * ndir;                       // (direction, half) pairs: neighbours in the grid share their row tiles
    const int dh = blockIdx.x % nq;
    const int d = dh >> 1, c0 = (dh & 1) * BF_CH;
    const int64_t tile0 = blockIdx.x / nq, tstride = gridDim.x / nq;   // (the host makes gridDim.x a multiple of nq)
    const int64_t ntiles = (M + BF_BM - 1) / BF_BM;
    const int Kp = bf_kp(cin);
    const uint16_t* Wd = Wb + ((int64_t)d * G + c0) * Kp;
    float* Pd = P + (int64_t)d * M * G;
    float bias[BF_CT];
#pragma unroll
    for (int ct = 0; ct < BF_CT; ++ct) bias[ct] = bin[d * bstride + c0 + ct * 16 + i];

    for (int kb = 0; kb < Kp; kb += BF_PK) {
        const int kn = min(BF_PK, Kp - kb);        // k of this panel (a multiple of 32)
        const bool first = kb == 0, last = kb + BF_PK >= Kp;
        if (!first) __syncthreads();               // every wave is done reading the previous panel
        // stage Wb[d][c0 .. c0 + 192)[kb .. kb + kn) into wl[c][BF_LS], 16 bytes (8 k) per thread and step
        const int vpr = kn / 8;                    // vectors per row
        for (int v = threadIdx.x; v < BF_CH * vpr; v += blockDim.x) {
            const int c = v / vpr, kv = v % vpr;
            *reinterpret_cast<uint4*>(wl + c * BF_LS + kv * 8) =
                *reinterpret_cast<const uint4*>(Wd + (int64_t)c * Kp + kb + kv * 8);
        }
        __syncthreads();
        const uint16_t* bl = wl + i * BF_LS + q * 8;   // the lane's B fragments: column ct * 16 + i, k = k0 + 8 q ..
        for (int64_t tile = tile0; tile < ntiles; tile += tstride) {
            const int64_t m0 = tile * BF_BM + wave * 16;
            if (m0 >= M) continue;                 // (wave-uniform; no barrier inside the tile loop)
            const int64_t arow = m0 + i;
            const bool row_ok = arow < M;
            const float* xr = x + (row_ok ? arow : 0) * cin;
            const int ka = kb + q * 8;             // the lane's first k of the panel
            f32x4 acc[BF_CT];
#pragma unroll
            for (int ct = 0; ct < BF_CT; ++ct) {
                if (first) {
                    acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t row = m0 + q * 4 + r;
                        acc[ct][r] = row < M ? Pd[row * G + c0 + ct * 16 + i] : 0.f;
                    }
                }
            }
            float a[8], an[8] = {};                // (an: the prefetched next step; unused after the panel's last)
            bf_load_a<VEC>(xr + ka, row_ok, ka, cin, a);
            for (int k0 = 0; k0 < kn; k0 += 32) {
                if (k0 + 32 < kn) bf_load_a<VEC>(xr + ka + k0 + 32, row_ok, ka + k0 + 32, cin, an);
                const bf16x8 af = bf_pack(a);
#pragma unroll
                for (int ct = 0; ct < BF_CT; ++ct) {
                    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(bl + ct * 16 * BF_LS + k0);
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[ct], 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = an[j];
            }
#pragma unroll
            for (int ct = 0; ct < BF_CT; ++ct) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = m0 + q * 4 + r;
                    if (row < M) Pd[row * G + c0 + ct * 16 + i] = last ? acc[ct][r] + bias[ct] : acc[ct][r];
                }
            }
        }
    }
}

__global__ __launch_bounds__(BF_WAVES * 64) void gru_proj_bf16_kernel(const float* __restrict__ x, int cin,
                                                                      const uint16_t* __restrict__ Wb,
                                                                      const float* __restrict__ bin, int64_t bstride,
                                                                      float* __restrict__ P, int64_t M, int ndir) {
    __shared__ __attribute__((aligned(16))) uint16_t wl[BF_CH * BF_LS];
    if ((cin & 3) == 0)
        gru_proj_bf16_body<true>(x, cin, Wb, bin, bstride, P, M, ndir, wl);
    else
        gru_proj_bf16_body<false>(x, cin, Wb, bin, bstride, P, M, ndir, wl);
}

// the two launches of one GRU layer's projection.  Wb: room for bf_w_elems(cin, ndir) bf16.
inline void launch_gru_proj_bf16(hipStream_t stream, const float* x, int cin, int ndir, const float* W, int64_t wstride,
                                 const float* bin, int64_t bstride, uint16_t* Wb, float* P, int64_t M, int blocks_cap) {
    const int64_t welems = (int64_t)bf_w_elems(cin, ndir);
    hipLaunchKernelGGL(w_to_bf16_kernel, dim3((unsigned)std::min<int64_t>((welems + 255) / 256, 1024)), dim3(256), 0, stream,
                       W, wstride, cin, ndir, Wb);
    const int nq = 2 * ndir;
    const int64_t ntiles = (M + BF_BM - 1) / BF_BM;
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(ntiles, blocks_cap / nq));
    hipLaunchKernelGGL(gru_proj_bf16_kernel, dim3((unsigned)(per * nq)), dim3(BF_WAVES * 64), 0, stream, x, cin, Wb, bin,
                       bstride, P, M, ndir);
}

// workgroups of gru_proj_bf16_kernel: one per compute unit (each holds ~100 KB of LDS); any count gives the same bits
inline int bf_blocks_cap() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1)
        cus = 256;
    return cus;
}

// the bf16 projection kernels own G / 2 = 192 columns per workgroup: 128 units alone
inline int check_bf16_units(int units, const char* me) {
    if (units && units != H_MAX)
        return po_fail(PO_E_UNSUPPORTED, std::string(me) + ": bf16 precision (PO_CALL_BF16) is built for GRU layers of " +
                       std::to_string(H_MAX) + " units, the model has " + std::to_string(units) + " (use PO_CALL_F32)");
    return PO_OK;
}

}  // namespace
