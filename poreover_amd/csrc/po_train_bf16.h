// The weight and input GEMMs of a GRU layer under `train --gemm_precision bf16` (po_train_set_precision(PO_CALL_BF16),
// DESIGN.md §11.2): both operands rounded to bf16 by the rule of po_bf16_rules.h (round to nearest even; the hardware's
// packed conversion, as gru_proj_bf16_kernel does for x), products and sums in f32 on v_mfma_f32_16x16x32_bf16.  Included by
// po_train.hip alone, after po_call_bf16.h (whose forward projection the trainer runs in this mode).  Built for 128 units
// (384 gate columns).
//
//   wgrad_bf16_kernel     part[z][k][c] = sum over the rows m of split z of bf16(A[m][k]) · bf16(D[m][c]), k < K, c < 384:
//                         dW = Xᵀ·dA (K = cin) and dU = H_prevᵀ·dR (K = 128); combine_kernel adds the splits in order.
//                         Also bpart[z][c] = sum over the same rows of D[m][c], UNROUNDED and in f32: the bias gradients
//                         (column sums of dA and dR), from the values the kernel holds anyway instead of a colsum_kernel
//                         pass over dA and dR (measured: 39 of the stage's 73 ms at batch 512 with that pass)
//   w_rows_to_bf16_kernel a GRU layer's W[d][c][k] (f32, its native rows of 384) rounded to bf16 in the same layout
//   dx_bf16_kernel        dX[m][c] = sum_d sum_k bf16(dA_d[m][k]) · Wb_d[c][k], k < 384, c < cin
//
// wgrad_bf16_kernel.  The reduction index is the row m, so a lane's MFMA fragment is 8 consecutive m of ONE column of A or
// D: a whole row apart in memory.  Hence LDS: a workgroup (4 waves) owns a 64 (k) x 192 (c) tile of the result and one
// split; it walks the split 32 rows at a time.  A block is 32 x 64 of A and 32 x 192 of D: every thread reads an 8-row x
// 4-column piece (8 loads of 16 bytes, each a whole 256-byte-or-longer run across neighbouring lanes; scalar loads for A
// where cin is no multiple of 4), rounds it and writes four 16-byte pieces of the TRANSPOSED image [column][32 m] (rows of
// 32 + 8 bf16: 80 bytes, so the 8 lanes of a ds_write_b128 group fall on distinct banks).  Each element leaves global memory
// once per tile and is rounded once.  A wave then owns 32 x 96 of the tile: 2 A fragments and 6 D fragments (ds_read_b128),
// 12 MFMAs per block, 48 accumulator registers.  The image is double buffered: the loads of block b + 1 are issued before
// the MFMAs of block b and written to the other buffer after them, one barrier per block.  Rows past the split's end or M,
// and columns past K, are zeros in the image (every lane runs every MFMA: no lane masking).
//
// The bias sums: a D thread adds its 8 rows of every block to four f32 registers in row order (rows past the end add an
// exact 0), and after the last block the four row groups of a column are added in order through LDS; the workgroups of the
// first k tile write them.
//
// Determinism: split z's rows are [z·rows, (z + 1)·rows) with rows a multiple of 32 (po_train_rules.h), each walked in
// ascending blocks of 32; a partial sum depends on nothing but its own rows, and the splits are added in order by
// combine_kernel.  No atomics, no hand-off between workgroups.
//
// dx_bf16_kernel.  Both fragments are 8 contiguous k: of a dA row (f32, two 16-byte loads, rounded in registers) and of a W
// row (bf16, one 16-byte load: W's native [cin][384] layout has k fastest, so no transpose).  One wave per 16 rows x 64
// columns, four waves per workgroup along the rows, the column tiles of one row block neighbours in the grid (dA reaches
// HBM once); the directions are accumulated in order in the same f32 registers.
#pragma once
#include "po_call_bf16.h"

namespace {

constexpr int WB_TK = 64;            // k (result rows) per workgroup
constexpr int WB_TC = 192;           // c (result columns) per workgroup: half of the 384
constexpr int WB_MB = 32;            // rows of A / D per block: one MFMA's k
constexpr int WB_LS = WB_MB + 8;     // LDS row stride in bf16 (80 bytes)
constexpr int WB_COLS = WB_TK + WB_TC;   // LDS rows: A's 64 columns, then D's 192

// this thread's 8 x 4 piece of block [m0, m0 + 32): rows m0 + 8 j + r, columns 4 g .. 4 g + 3 of D's tile (threads 0 .. 191)
// or of A's (192 .. 255); zeros past mend and past K
template <bool VEC>
__device__ __forceinline__ void wb_fetch(const float* __restrict__ A, int64_t lda, int K, const float* __restrict__ D, int k0,
                                         int c0, int64_t m0, int64_t mend, f32x4 (&v)[8]) {
    const int tid = threadIdx.x;
    const bool isA = tid >= WB_TC;   // (wave-uniform: the fourth wave)
    const int e = isA ? tid - WB_TC : tid;
    const int g = e >> 2, j = e & 3;
    const int64_t mr = m0 + 8 * j;
    if (!isA) {
        const float* p = D + mr * G + c0 + 4 * g;
#pragma unroll
        for (int r = 0; r < 8; ++r)
            v[r] = mr + r < mend ? *reinterpret_cast<const f32x4*>(p + (int64_t)r * G) : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
        const int k = k0 + 4 * g;
        const float* p = A + mr * lda + k;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool ok = mr + r < mend;
            if (VEC) {   // K and lda multiples of 4: the piece is wholly inside or outside, and 16-byte aligned
                v[r] = ok && k < K ? *reinterpret_cast<const f32x4*>(p + (int64_t)r * lda) : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) v[r][cc] = ok && k + cc < K ? p[(int64_t)r * lda + cc] : 0.f;
            }
        }
    }
}

// the piece rounded and written to the image `buf`: [column][8 j .. 8 j + 8); cs: the running sums of this thread's four
// columns of D over its rows, unrounded and in row order (the bias gradient; A's threads carry zeros)
__device__ __forceinline__ void wb_stage(const f32x4 (&v)[8], uint16_t* buf, f32x4& cs) {
    const int tid = threadIdx.x;
    const bool isA = tid >= WB_TC;
    const int e = isA ? tid - WB_TC : tid;
    const int g = e >> 2, j = e & 3;
    if (!isA) {
#pragma unroll
        for (int r = 0; r < 8; ++r) cs += v[r];
    }
    uint16_t* p = buf + ((isA ? 0 : WB_TK) + 4 * g) * WB_LS + 8 * j;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        bf16x8 o;
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = (__bf16)v[r][cc];   // v_cvt_pk_bf16_f32: round to nearest even
        *reinterpret_cast<bf16x8*>(p + cc * WB_LS) = o;
    }
}

template <bool VEC>
__device__ __forceinline__ void wgrad_bf16_body(const float* __restrict__ A, int64_t lda, int K, const float* __restrict__ D,
                                                int64_t M, int64_t rows, float* __restrict__ part, int64_t pstride,
                                                float* __restrict__ bpart, uint16_t (&img)[2][WB_COLS * WB_LS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int k0 = blockIdx.x * WB_TK, c0 = blockIdx.y * WB_TC;
    const int wk = (wave & 1) * 32, wc = (wave >> 1) * 96;   // the wave's 32 x 96 of the tile
    const int64_t mbeg = (int64_t)blockIdx.z * rows, mend = mbeg + rows < M ? mbeg + rows : M;
    const int nb = (int)((mend - mbeg + WB_MB - 1) / WB_MB);
    f32x4 acc[2][6];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v[8], cs = f32x4{0.f, 0.f, 0.f, 0.f};
    wb_fetch<VEC>(A, lda, K, D, k0, c0, mbeg, mend, v);
    wb_stage(v, img[0], cs);
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        const bool more = b + 1 < nb;   // (uniform over the workgroup)
        if (more) wb_fetch<VEC>(A, lda, K, D, k0, c0, mbeg + (int64_t)(b + 1) * WB_MB, mend, v);   // in flight under the MFMAs
        const uint16_t* cur = img[b & 1];
        bf16x8 fa[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[a] = *reinterpret_cast<const bf16x8*>(cur + (wk + 16 * a + i) * WB_LS + 8 * q);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const bf16x8 fb = *reinterpret_cast<const bf16x8*>(cur + (WB_TK + wc + 16 * t + i) * WB_LS + 8 * q);
#pragma unroll
            for (int a = 0; a < 2; ++a) acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb, acc[a][t], 0, 0, 0);
        }
        if (more) wb_stage(v, img[(b + 1) & 1], cs);   // (every wave left that buffer before the barrier that ended block b - 1)
        __syncthreads();
    }
    if (bpart && blockIdx.x == 0) {   // (uniform over the workgroup) the column sums of D over the split: the four row groups in order
        float* red = reinterpret_cast<float*>(&img[0][0]);   // (free: the loop ended on a barrier)
        if (threadIdx.x < WB_TC) {
            const int g = threadIdx.x >> 2, j = threadIdx.x & 3;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) red[j * WB_TC + 4 * g + cc] = cs[cc];
        }
        __syncthreads();
        if (threadIdx.x < WB_TC) {
            const int c = threadIdx.x;
            bpart[(int64_t)blockIdx.z * G + c0 + c] = ((red[c] + red[WB_TC + c]) + red[2 * WB_TC + c]) + red[3 * WB_TC + c];
        }
    }
    float* pz = part + (int64_t)blockIdx.z * pstride;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int c = c0 + wc + 16 * t + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k0 + wk + 16 * a + 4 * q + r;
                if (k < K) pz[(int64_t)k * G + c] = acc[a][t][r];
            }
        }
}

// grid (ceil(K / 64), 2, splits); rows: rows per split, a multiple of 32; part: [splits][pstride >= K·384]; bpart (or
// null): [splits][384], the f32 column sums of the unrounded D over each split (written by the workgroups of the first k tile)
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const float* __restrict__ A, int64_t lda, int K,
                                                         const float* __restrict__ D, int64_t M, int64_t rows,
                                                         float* __restrict__ part, int64_t pstride, float* __restrict__ bpart) {
    __shared__ __attribute__((aligned(16))) uint16_t img[2][WB_COLS * WB_LS];
    if (((K | lda) & 3) == 0)
        wgrad_bf16_body<true>(A, lda, K, D, M, rows, part, pstride, bpart, img);
    else
        wgrad_bf16_body<false>(A, lda, K, D, M, rows, part, pstride, bpart, img);
}

inline void launch_wgrad_bf16(hipStream_t stream, const float* A, int64_t lda, int K, const float* D, int64_t M, int64_t rows,
                              int nz, float* part, int64_t pstride, float* bpart) {
    hipLaunchKernelGGL(wgrad_bf16_kernel, dim3((unsigned)((K + WB_TK - 1) / WB_TK), (unsigned)(G / WB_TC), (unsigned)nz),
                       dim3(256), 0, stream, A, lda, K, D, M, rows, part, pstride, bpart);
}

// Wb[d][e] = bf16(W[d · wstride + e]), e < cin · 384
__global__ __launch_bounds__(256) void w_rows_to_bf16_kernel(const float* __restrict__ W, int64_t wstride, int cin, int ndir,
                                                             uint16_t* __restrict__ Wb) {
    const int64_t per = (int64_t)cin * G, total = ndir * per;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
        Wb[e] = po_bf16_from_f32(W[(e / per) * wstride + e % per]);
}

// grid (row blocks of 64 x nct column tiles of 64, the column tile fastest); Wb: [nd][cin][384] bf16
__global__ __launch_bounds__(256) void dx_bf16_kernel(const float* __restrict__ dA, int64_t dastride,
                                                      const uint16_t* __restrict__ Wb, int nd, int cin, float* __restrict__ dX,
                                                      int64_t M, int nct) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)(blockIdx.x / nct) * 4 + wave) * 16;
    if (m0 >= M) return;   // (wave-uniform; the kernel has no barrier)
    const int c0 = (blockIdx.x % nct) * 64;
    const int i = lane & 15, q = lane >> 4;
    const int64_t arow = m0 + i;
    const bool row_ok = arow < M;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < nd; ++d) {
        const float* ar = dA + d * dastride + (row_ok ? arow : 0) * G + 8 * q;
        const uint16_t* wr[4];
        bool cok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = c0 + 16 * t + i;
            cok[t] = c < cin;
            wr[t] = Wb + ((int64_t)d * cin + (cok[t] ? c : 0)) * G + 8 * q;
        }
        float a[8], an[8] = {};
        bf_load_a<true>(ar, row_ok, 0, G, a);
        for (int k0 = 0; k0 < G; k0 += 32) {
            if (k0 + 32 < G) bf_load_a<true>(ar + k0 + 32, row_ok, 0, G, an);
            const bf16x8 af = bf_pack(a);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bf16x8 bf;
#pragma unroll
                for (int e = 0; e < 8; ++e) bf[e] = (__bf16)0.f;
                if (cok[t]) bf = *reinterpret_cast<const bf16x8*>(wr[t] + k0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = an[e];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = c0 + 16 * t + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + 4 * q + r;
            if (row < M && c < cin) dX[row * cin + c] = acc[t][r];
        }
    }
}

// the two launches of one GRU layer's input gradient.  Wb: room for nd · cin · 384 bf16
inline void launch_dx_bf16(hipStream_t stream, const float* dA, int64_t dastride, const float* W, int64_t wstride, int nd,
                           int cin, uint16_t* Wb, float* dX, int64_t M) {
    const int64_t welems = (int64_t)nd * cin * G;
    hipLaunchKernelGGL(w_rows_to_bf16_kernel, dim3((unsigned)std::min<int64_t>((welems + 255) / 256, 1024)), dim3(256), 0, stream,
                       W, wstride, cin, nd, Wb);
    const int nct = (cin + 63) / 64;
    hipLaunchKernelGGL(dx_bf16_kernel, dim3((unsigned)(((M + 63) / 64) * nct)), dim3(256), 0, stream, dA, dastride, Wb, nd, cin,
                       dX, M, nct);
}

}  // namespace
