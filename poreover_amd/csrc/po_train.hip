// CTC training of the basecalling network (`poreover train`) on the device, in f32 like `call` (the CTC lattice in f64).
//
// Replaces, from network/network.py of the reference: train_ctc_model's step (network.py:78-131): the Keras model's
// forward pass, tf.compat.v1.nn.ctc_loss averaged over the batch, its gradient through GradientTape and Keras Adam.
// The forward pass is `call`'s (po_call_kernels.h), with the recurrence also saving what backpropagation needs.  One
// step, for a batch of n windows of T samples:
//
//   forward            conv_relu_kernel, gru_proj_kernel, gru_recur_body<SAVE = true>, dense_softmax_kernel; every
//                      layer's output is kept
//   ctc_lsm_kernel     log-softmax of the logits, f64, one lane per frame
//   ctc_alpha_beta_kernel  one workgroup per window: the α and β recursions over the 2L+1 states, f64 in log space;
//                      merge_repeated = 0 is the decoder's `ctc` lattice (label states do not self-loop, a blank may always
//                      be skipped), 1 is standard CTC; writes -log Z
//   ctc_grad_kernel    one lane per frame: dlogits = (softmax - posterior occupancy) / n, summed over states in order
//   dense backward     dW = Xᵀ·dlogits (wgrad), db = column sums, dX = dlogits·Wᵀ (dense_dx_kernel)
//   gru_back_recur_kernel  BPTT, one persistent launch per GRU layer covering both directions, the mirror of the forward
//                      recurrence: 16 windows x one direction per workgroup, H / 16 waves x 16 units (a template on H like
//                      the forward one); each lane keeps its unit's row of U (3H f32 = 3H/4 VGPRs, 96 at H = 128) as the B
//                      operand of dh_prev = dh⊙z + dR·Uᵀ (3H/4 MFMA per step); dR passes through LDS, double buffered (one
//                      barrier per step)
//   wgrad_kernel + combine_kernel  every weight gradient as Aᵀ·B over the M = n·T rows on v_mfma_f32_16x16x4_f32: dW = Xᵀ·dA,
//                      dU = H_prevᵀ·dR, Conv1D dW per tap from row-shifted inputs; split over M in a fixed partition, the
//                      partial sums combined in a fixed order by a second launch (colsum_kernel: the bias gradients so)
//   dx_kernel          dX = Σ_d dA_d·W_dᵀ of a GRU layer (directions in a fixed order); conv_dx_kernel for a deeper Conv1D
//   adam_kernel        Keras Adam on the flat parameter vector
// No float atomics and no hand-off between workgroups within a launch: a step's gradient is the same bits every run.
//
// po_train_set_precision(PO_CALL_BF16) (opt-in, per trainer) gives four products of every GRU layer bf16
// operands with f32 sums: the forward projection by po_call_bf16.h's kernels (the logits are `call --precision bf16`'s), dW
// and dU by wgrad_bf16_kernel (+ combine_kernel; the bias sums come out of the same pass) and dX by dx_bf16_kernel
// (po_train_bf16.h).  Everything else, and every kernel of the default mode, is as described here.
//
// po_train_eval (held-out validation) is the forward pass above, ctc_lsm_kernel + ctc_alpha_beta_kernel (α
// only) + ctc_loss_kernel where the losses are asked for, then po_eval.hip's eval_path_kernel and edit_distance_kernel on the
// trainer's probabilities and labels: no gradient, no Adam.
//
// The recipe around a step (opt-in; DESIGN.md §11.3, the rules are po_train_recipe_rules.h): po_train_accumulate is the step
// up to and including the backward pass, then grad_axpy_kernel adds weight·g to an accumulator of the gradient's size;
// po_train_apply runs grad_sqsum_kernel + grad_norm_final_kernel (the accumulator's global L2 norm in f64 over a fixed
// partition, and a 16-byte record of norm, clip scale and whether the norm is finite) and adamw_apply_kernel (Adam on the
// clipped gradient plus decoupled weight decay; a record that is not finite leaves p, m and v alone), and reads the record
// back with its results.  The same rules as a step: no float atomics, no hand-off between workgroups, no host
// synchronisation between the launches.
//
// BPTT of one direction, walk step s (input time t, output position to), dh = dout[to] + the carried dh:
//   dz = dh·(h_prev − h~);  dah = dh·(1 − z)·(1 − h~²);  dr = dah·u_h;  daz = dz·z(1 − z);  dar = dr·r(1 − r)
//   dA = (daz, dar, dah) → input projection and b_in;  dR = (daz, dar, dah·r) → U and b_rec;  dh_prev = dh·z + dR·Uᵀ
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "po_call_kernels.h"
#include "po_train_bf16.h"
#include "po_train_recipe_rules.h"
#include "po_train_rules.h"

#include "po_internal.h"

namespace {

constexpr int WG_ROWS = PO_TRAIN_WG_ROWS;    // rows per split of the M-reductions (at most MAX_SPLIT splits)
constexpr int MAX_SPLIT = PO_TRAIN_MAX_SPLIT;
constexpr int NSTAGE = 5;        // forward, CTC, backward recurrence, weight and input GEMMs, Adam

__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1p(exp(-fabs(a - b)));
}

// lsm[m][c] = log softmax(logits[m])[c] in f64
__global__ __launch_bounds__(256) void ctc_lsm_kernel(const float* __restrict__ logits, double* __restrict__ lsm, int64_t M) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    double x[NOUT], mx = -INFINITY, sum = 0.0;
    for (int c = 0; c < NOUT; ++c) { x[c] = logits[m * NOUT + c]; mx = fmax(mx, x[c]); }
    for (int c = 0; c < NOUT; ++c) sum += exp(x[c] - mx);
    const double lz = mx + log(sum);
    for (int c = 0; c < NOUT; ++c) lsm[m * NOUT + c] = x[c] - lz;
}

// state s of a window with labels lab[0..L): blank (4) for even s, lab[(s - 1) / 2] for odd s
__device__ __forceinline__ int state_label(const int32_t* lab, int s) { return (s & 1) ? lab[s >> 1] : NOUT - 1; }
// may the path reach label state s (odd) from label state s - 2, skipping the blank between?
__device__ __forceinline__ bool skip_ok(const int32_t* lab, int s, int merge) {
    return s >= 3 && (!merge || lab[s >> 1] != lab[(s >> 1) - 1]);
}

// One workgroup per window.  A[t][s] = log P(frames 0..t, state s at t), B[t][s] = log P(frames t+1..T-1 | state s at
// t) (exclusive of frame t), rows of S = 2L+1 states at stride Smax; logz[w] = log P(label | window), which is α's alone:
// with_beta = 0 (po_train_eval, which runs no gradient) leaves B as it is
__global__ __launch_bounds__(256) void ctc_alpha_beta_kernel(const double* __restrict__ lsm, const int32_t* __restrict__ labels,
                                                             const int64_t* __restrict__ loff, int T, int Smax, int merge,
                                                             int with_beta, double* __restrict__ A, double* __restrict__ B,
                                                             double* __restrict__ logz) {
    const int w = blockIdx.x;
    const int32_t* lab = labels + loff[w];
    const int L = (int)(loff[w + 1] - loff[w]);
    const int S = 2 * L + 1;
    const double* lp = lsm + (int64_t)w * T * NOUT;
    double* Aw = A + (int64_t)w * T * Smax;
    double* Bw = B + (int64_t)w * T * Smax;
    for (int s = threadIdx.x; s < S; s += blockDim.x)
        Aw[s] = s == 0 ? lp[NOUT - 1] : (s == 1 ? lp[lab[0]] : -INFINITY);
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        const double* prev = Aw + (int64_t)(t - 1) * Smax;
        double* row = Aw + (int64_t)t * Smax;
        for (int s = threadIdx.x; s < S; s += blockDim.x) {
            const bool lbl = s & 1;
            double v = (!lbl || merge) ? prev[s] : -INFINITY;
            if (s >= 1) v = lse2(v, prev[s - 1]);
            if (lbl && skip_ok(lab, s, merge)) v = lse2(v, prev[s - 2]);
            row[s] = v + lp[(int64_t)t * NOUT + state_label(lab, s)];
        }
        __syncthreads();
    }
    for (int s = threadIdx.x; with_beta && s < S; s += blockDim.x)
        Bw[(int64_t)(T - 1) * Smax + s] = (s == S - 1 || s == S - 2) ? 0.0 : -INFINITY;
    __syncthreads();
    for (int t = T - 2; with_beta && t >= 0; --t) {
        const double* nx = Bw + (int64_t)(t + 1) * Smax;
        const double* lpn = lp + (int64_t)(t + 1) * NOUT;
        double* row = Bw + (int64_t)t * Smax;
        for (int s = threadIdx.x; s < S; s += blockDim.x) {
            const bool lbl = s & 1;
            double v = (!lbl || merge) ? nx[s] + lpn[state_label(lab, s)] : -INFINITY;
            if (s + 1 < S) v = lse2(v, nx[s + 1] + lpn[state_label(lab, s + 1)]);
            if (lbl && s + 2 < S && skip_ok(lab, s + 2, merge)) v = lse2(v, nx[s + 2] + lpn[state_label(lab, s + 2)]);
            row[s] = v;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double* last = Aw + (int64_t)(T - 1) * Smax;
        logz[w] = S >= 2 ? lse2(last[S - 1], last[S - 2]) : last[0];
    }
}

// dlogits[m][c] = (softmax[m][c] - sum_{s: label(s) = c} exp(A + B - log Z)) * inv_n; loss[w] = -log Z
__global__ __launch_bounds__(256) void ctc_grad_kernel(const double* __restrict__ lsm, const int32_t* __restrict__ labels,
                                                       const int64_t* __restrict__ loff, int n, int T, int Smax,
                                                       const double* __restrict__ A, const double* __restrict__ B,
                                                       const double* __restrict__ logz, float inv_n,
                                                       float* __restrict__ dlogits, float* __restrict__ loss) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (int64_t)n * T) return;
    const int w = (int)(m / T), t = (int)(m % T);
    const int32_t* lab = labels + loff[w];
    const int S = 2 * (int)(loff[w + 1] - loff[w]) + 1;
    const double lz = logz[w];
    const double* a = A + ((int64_t)w * T + t) * Smax;
    const double* b = B + ((int64_t)w * T + t) * Smax;
    double occ[NOUT] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) occ[state_label(lab, s)] += exp(a[s] + b[s] - lz);
    for (int c = 0; c < NOUT; ++c) dlogits[m * NOUT + c] = (float)(exp(lsm[m * NOUT + c]) - occ[c]) * inv_n;
    if (t == 0) loss[w] = (float)(-lz);
}

// loss[w] = -log Z, as ctc_grad_kernel writes it (po_train_eval runs no gradient)
__global__ __launch_bounds__(256) void ctc_loss_kernel(const double* __restrict__ logz, int n, float* __restrict__ loss) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n) loss[w] = (float)(-logz[w]);
}

// dX[m][c] = sum_k dY[m][k] * Wd[c][k]  (Dense: k < 5)
__global__ __launch_bounds__(256) void dense_dx_kernel(const float* __restrict__ dY, const float* __restrict__ Wd, int cin,
                                                       float* __restrict__ dX, int64_t M) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M * cin) return;
    const int64_t m = e / cin;
    const int c = (int)(e % cin);
    float acc = 0.f;
    for (int k = 0; k < NOUT; ++k) acc = fmaf(dY[m * NOUT + k], Wd[c * NOUT + k], acc);
    dX[e] = acc;
}

// dY[e] = 0 where the ReLU output is 0 (the Conv1D's pre-activation gradient, in place)
__global__ __launch_bounds__(256) void relu_mask_kernel(float* __restrict__ dY, const float* __restrict__ out, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && !(out[e] > 0.f)) dY[e] = 0.f;
}

// part[z][p0 + k][c] = sum over rows m of split z of A[m + shift][k] * Bm[m][c], k < K, c < N; the A row counts as zero
// where its time index m % T + shift falls outside [0, T) (Conv1D taps).  One wave per 16 (k) x 64 (c) tile, four waves
// per workgroup along k; the split's rows are walked 4 at a time (v_mfma_f32_16x16x4_f32, zero-filled past its end).
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                    int64_t ldb, int K, int N, int64_t M, int T, int shift, int64_t rows,
                                                    float* __restrict__ part, int ldp, int p0, int64_t pstride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k0 = (blockIdx.x * 4 + wave) * 16;
    if (k0 >= K) return;
    const int c0 = blockIdx.y * 64;
    const int i = lane & 15, kq = lane >> 4;
    const int64_t mbeg = (int64_t)blockIdx.z * rows, mend = mbeg + rows < M ? mbeg + rows : M;
    const bool kok = k0 + i < K;
    f32x4 acc[4];
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t m0 = mbeg; m0 < mend; m0 += 4) {
        const int64_t m = m0 + kq;
        const bool mok = m < mend;
        bool aok = mok && kok;
        if (shift != 0 && aok) {
            const int ts = (int)(m % T) + shift;
            aok = ts >= 0 && ts < T;
        }
        const float a = aok ? A[(m + shift) * lda + k0 + i] : 0.f;
        const float* br = Bm + (mok ? m : 0) * ldb + c0 + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool cok = mok && c0 + q * 16 + i < N;
            acc[q] = mfma4(a, cok ? br[q * 16] : 0.f, acc[q]);
        }
    }
    float* pz = part + (int64_t)blockIdx.z * pstride;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + q * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + kq * 4 + r;
            if (k < K && c < N) pz[(int64_t)(p0 + k) * ldp + c] = acc[q][r];
        }
    }
}

// part[z][c] = sum over rows m of split z of X[m][c], in row order
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int64_t ldx, int N, int64_t M,
                                                     int64_t rows, float* __restrict__ part, int64_t pstride) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const int64_t mbeg = (int64_t)blockIdx.y * rows, mend = mbeg + rows < M ? mbeg + rows : M;
    float acc = 0.f;
    for (int64_t m = mbeg; m < mend; ++m) acc += X[m * ldx + c];
    part[(int64_t)blockIdx.y * pstride + c] = acc;
}

// out[e] = sum_{z < nz} part[z][e], in z order
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ part, int nz, int64_t pstride, int64_t n,
                                                      float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float acc = part[e];
    for (int z = 1; z < nz; ++z) acc += part[(int64_t)z * pstride + e];
    out[e] = acc;
}

// dX[m][c] = sum_{d < nd} sum_k dA_d[m][k] * W_d[c][k], k < G: the GRU layer's input gradient.  One wave per 16 rows x
// 64 columns, four waves per workgroup along the rows (gru_proj_kernel's tiling).
__global__ __launch_bounds__(256) void dx_kernel(const float* __restrict__ dA, int64_t dastride, const float* __restrict__ W,
                                                 int64_t wstride, int nd, int cin, float* __restrict__ dX, int64_t M, int G) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (m0 >= M) return;
    const int c0 = blockIdx.y * 64;
    const int i = lane & 15, kq = lane >> 4;
    const int64_t arow = m0 + i;
    const bool arow_ok = arow < M;
    f32x4 acc[4];
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < nd; ++d) {
        const float* Ad = dA + d * dastride + (arow_ok ? arow : 0) * G;
        const float* Wd = W + d * wstride;
        for (int kb = 0; kb < G; kb += 12) {   // (G = 3 H is a multiple of 48: three k-steps per trip, in k order)
#pragma unroll
            for (int k0 = kb; k0 < kb + 12; k0 += 4) {
                const int k = k0 + kq;
                const float a = arow_ok ? Ad[k] : 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = c0 + q * 16 + i;
                    acc[q] = mfma4(a, c < cin ? Wd[(int64_t)c * G + k] : 0.f, acc[q]);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + q * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + kq * 4 + r;
            if (row < M && c < cin) dX[row * cin + c] = acc[q][r];
        }
    }
}

// dX[m][c] = sum_j sum_f dpre[w][t - j + padl][f] * Wt[j][c][f] (rows outside [0, T) read 0): a deeper Conv1D's input
// gradient, one lane per element
__global__ __launch_bounds__(256) void conv_dx_kernel(const float* __restrict__ dpre, const float* __restrict__ Wt, int K,
                                                      int cin, int F, float* __restrict__ dX, int64_t M, int T) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M * cin) return;
    const int64_t m = e / cin;
    const int c = (int)(e % cin);
    const int t = (int)(m % T);
    const int64_t w0 = m - t;
    const int padl = (K - 1) / 2;
    float acc = 0.f;
    for (int j = 0; j < K; ++j) {
        const int ts = t - j + padl;
        if (ts < 0 || ts >= T) continue;
        const float* dr = dpre + (w0 + ts) * F;
        const float* wr = Wt + ((int64_t)j * cin + c) * F;
        for (int f = 0; f < F; ++f) acc = fmaf(dr[f], wr[f], acc);
    }
    dX[e] = acc;
}

struct BackDir {
    const float* save;  // [n * T][5 H] the forward recurrence's saved values, walk order
    const float* U;     // [H][G] recurrent kernel
    float* dA;          // [n * T][G] input-projection gradient (daz, dar, dah) at input time t
    float* dR;          // [n * T][G] recurrent gradient (daz, dar, dah·r), walk order
    int backward, rev_out, col;
};
struct BackArgs {
    BackDir dir[2];
    const float* dout;  // [n * T][dout_stride] gradient of the layer's output
    int dout_stride, n, T;
};

// LDS-only barrier: the stores of dA / dR to global memory need not complete before the next step
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int H>
__global__ __launch_bounds__(H * 4) void gru_back_recur_kernel(BackArgs a) {
    constexpr int G = 3 * H, SV = SV_N * H;
    constexpr int GS = G + 1;   // LDS row stride of dR (one pad word: the 16 rows of an MFMA operand hit distinct banks)
    __shared__ float ds[2][RT][GS];
    const BackDir D = a.dir[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int unit = wave * 16 + i;
    const int w0 = blockIdx.x * RT;
    const int T = a.T;
    // this lane's B operands: Uᵀ[4 kk + kq][unit] = U[unit][4 kk + kq]
    float u[G / 4];
#pragma unroll
    for (int kk = 0; kk < G / 4; ++kk) u[kk] = D.U[(int64_t)unit * G + 4 * kk + kq];
    for (int e = threadIdx.x; e < 2 * RT * GS; e += blockDim.x) (&ds[0][0][0])[e] = 0.f;   // rows of absent windows stay 0
    bool live[4];
    int64_t wrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int w = w0 + kq * 4 + r;
        live[r] = w < a.n;
        wrow[r] = (int64_t)(live[r] ? w : 0) * T;
    }
    float carry[4] = {0.f, 0.f, 0.f, 0.f};
    float sv[4][5], go[4];
    auto fetch = [&](int s) {
        const int to = D.rev_out ? s : (D.backward ? T - 1 - s : s);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* p = D.save + (wrow[r] + s) * SV + unit;
#pragma unroll
            for (int g = 0; g < 5; ++g) sv[r][g] = live[r] ? p[g * H] : 0.f;
            go[r] = live[r] ? a.dout[(wrow[r] + to) * a.dout_stride + D.col + unit] : 0.f;
        }
    };
    __syncthreads();
    fetch(T - 1);
    for (int s = T - 1; s >= 0; --s) {
        const int t = D.backward ? T - 1 - s : s;
        const int cur = s & 1;
        float dhz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float z = sv[r][0], rg = sv[r][1], hh = sv[r][2], uh = sv[r][3], hp = sv[r][4];
            const float dh = go[r] + carry[r];
            const float dz = dh * (hp - hh);
            const float dah = dh * (1.f - z) * (1.f - hh * hh);
            const float dr = dah * uh;
            const float daz = dz * z * (1.f - z);
            const float dar = dr * rg * (1.f - rg);
            const float drh = dah * rg;
            dhz[r] = dh * z;
            if (live[r]) {
                float* pa = D.dA + (wrow[r] + t) * G + unit;
                float* pr = D.dR + (wrow[r] + s) * G + unit;
                pa[0] = daz; pa[H] = dar; pa[2 * H] = dah;
                pr[0] = daz; pr[H] = dar; pr[2 * H] = drh;
                float* l = &ds[cur][kq * 4 + r][unit];
                l[0] = daz; l[H] = dar; l[2 * H] = drh;
            }
        }
        lds_barrier();
        if (s > 0) fetch(s - 1);   // in flight during the MFMAs
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* drow = &ds[cur][i][0];
#pragma unroll
        for (int kk = 0; kk < G / 4; ++kk) acc = mfma4(drow[4 * kk + kq], u[kk], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[r] = dhz[r] + acc[r];
    }
}

// Keras Adam (ResourceApplyAdam): m += (g - m)(1 - b1); v += (g² - v)(1 - b2); p -= lr_t · m / (sqrt(v) + eps)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float lr_t, float b1, float b2, float eps) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float ge = g[e];
    const float me = m[e] + (ge - m[e]) * (1.f - b1);
    const float ve = v[e] + (ge * ge - v[e]) * (1.f - b2);
    m[e] = me;
    v[e] = ve;
    p[e] = p[e] - lr_t * me / (sqrtf(ve) + eps);
}

// ---- the recipe (the rules are po_train_recipe_rules.h): accumulation, global norm, clipping, AdamW

// ga[e] = w·g[e] (FIRST: the first contribution after a reset; w = 1 gives g's bits) or fmaf(w, g[e], ga[e]).  One lane per
// 16 bytes (both vectors are whole allocations), the last n % 4 elements one by one
template <bool FIRST>
__global__ __launch_bounds__(256) void grad_axpy_kernel(float* __restrict__ ga, const float* __restrict__ g, int64_t n, float w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e0 = 4 * i;
    if (e0 + 3 < n) {
        const float4 x = reinterpret_cast<const float4*>(g)[i];
        float4 a;
        if (FIRST) {
            a.x = w * x.x; a.y = w * x.y; a.z = w * x.z; a.w = w * x.w;
        } else {
            a = reinterpret_cast<const float4*>(ga)[i];
            a.x = fmaf(w, x.x, a.x); a.y = fmaf(w, x.y, a.y); a.z = fmaf(w, x.z, a.z); a.w = fmaf(w, x.w, a.w);
        }
        reinterpret_cast<float4*>(ga)[i] = a;
    } else {
        for (int64_t e = e0; e < n; ++e) ga[e] = FIRST ? w * g[e] : fmaf(w, g[e], ga[e]);
    }
}

// part[b] = the sum of g[e]² over chunk b in f64, by po_train_recipe_rules.h's partition: 16-byte loads where g is 16-byte
// aligned and the group lies within n, else element by element in the same order (the same bits either way)
__global__ __launch_bounds__(PO_RECIPE_NORM_WG) void grad_sqsum_kernel(const float* __restrict__ g, int64_t n,
                                                                        double* __restrict__ part) {
    __shared__ double ws[PO_RECIPE_NORM_WG / 64];
    const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PO_RECIPE_NORM_VECS; ++j) {
        const int64_t e0 = po_recipe_norm_elem(blockIdx.x, j, threadIdx.x);
        if (vec && e0 + 3 < n) {
            const float4 x = *reinterpret_cast<const float4*>(g + e0);
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (e0 + k < n) {
                    const double x = g[e0 + k];
                    acc += x * x;
                }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = ws[0];
        for (int w = 1; w < PO_RECIPE_NORM_WG / 64; ++w) s += ws[w];
        part[blockIdx.x] = s;
    }
}

// one workgroup: the chunks' sums in chunk order, then the record
__global__ __launch_bounds__(64) void grad_norm_final_kernel(const double* __restrict__ part, int64_t nparts, float clip_norm,
                                                             po_recipe_record* __restrict__ rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int64_t b = 0; b < nparts; ++b) s += part[b];
    *rec = po_recipe_make_record(s, clip_norm);
}

// AdamW on the flat parameter vector from the accumulated gradient and the norm stage's record; a record that is not finite
// leaves p, m and v as they are.  One lane per 16 bytes, the last n % 4 elements one by one
__global__ __launch_bounds__(256) void adamw_apply_kernel(float* __restrict__ p, const float* __restrict__ ga,
                                                          float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                          const po_recipe_record* __restrict__ rec, float lr_t, float b1,
                                                          float b2, float eps, float decay) {
    if (!rec->finite) return;
    const float scale = rec->scale;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e0 = 4 * i;
    if (e0 + 3 < n) {
        const float4 g4 = reinterpret_cast<const float4*>(ga)[i];
        float4 p4 = reinterpret_cast<float4*>(p)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
        po_recipe_adamw(p4.x, m4.x, v4.x, g4.x, scale, lr_t, b1, b2, eps, decay);
        po_recipe_adamw(p4.y, m4.y, v4.y, g4.y, scale, lr_t, b1, b2, eps, decay);
        po_recipe_adamw(p4.z, m4.z, v4.z, g4.z, scale, lr_t, b1, b2, eps, decay);
        po_recipe_adamw(p4.w, m4.w, v4.w, g4.w, scale, lr_t, b1, b2, eps, decay);
        reinterpret_cast<float4*>(p)[i] = p4;
        reinterpret_cast<float4*>(m)[i] = m4;
        reinterpret_cast<float4*>(v)[i] = v4;
    } else {
        for (int64_t e = e0; e < n; ++e) po_recipe_adamw(p[e], m[e], v[e], ga[e], scale, lr_t, b1, b2, eps, decay);
    }
}

template <int H>
__global__ __launch_bounds__(H * 4) void gru_recur_save_kernel(RecurArgs a, float* save0, float* save1) {
    __shared__ float hs[2][RT][H + 1];
    gru_recur_body<H, true>(a, blockIdx.y ? save1 : save0, hs);
}

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

}  // namespace

struct po_trainer {
    std::vector<po_call_layer> layers;
    std::vector<int64_t> woff;          // each layer's first weight
    int max_batch = 0, T = 0;
    int64_t nw = 0, wmax = 0;
    int H = 0, G = 0;                   // the GRU layers' units per direction and 3 H
    int64_t step = 0;                   // Adam's t
    float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
    float* sig = nullptr;
    std::vector<float*> act;            // each layer's output [max_batch * T][cout]
    std::vector<float*> save;           // per GRU direction [max_batch * T][5 H], 2 per layer (the second unused for 1-dir)
    float *P = nullptr, *probs = nullptr, *dlog = nullptr, *loss = nullptr;
    float *dact[2] = {nullptr, nullptr}, *dA = nullptr, *dR = nullptr, *part = nullptr;
    double *lsm = nullptr, *logz = nullptr, *alpha = nullptr, *beta = nullptr;
    size_t ab_cap = 0, lab_cap = 0;
    int32_t* lab = nullptr;
    int64_t* loff = nullptr;
    int64_t part_cap = 0;
    // po_train_eval: the windows' paths (T codes of room each, at poff), their lengths, distances and statuses, the labels as bytes
    uint8_t *pred = nullptr, *lab8 = nullptr;
    int64_t* poff = nullptr;
    int32_t *pred_len = nullptr, *edit = nullptr, *estatus = nullptr;
    size_t lab8_cap = 0;
    // po_train_set_precision: the mode, and under PO_CALL_BF16 the bf16 copies of a GRU layer's input kernels, made anew in
    // every step: wb for the forward projection (transposed, po_call_bf16.h), wb2 for dX (native rows, po_train_bf16.h)
    int precision = PO_CALL_F32, bf_cap = 0;
    uint16_t *wb = nullptr, *wb2 = nullptr;
    float* bpart = nullptr;             // [MAX_SPLIT][384]: wgrad_bf16_kernel's bias sums per split
    // the recipe (po_train_accumulate / po_train_apply), allocated at first use: the accumulated gradient,
    // the norm's per-chunk sums and its record; accum_n = the contributions since the last reset (0: empty)
    float* ga = nullptr;
    double* npart = nullptr;
    po_recipe_record* rec = nullptr;
    int64_t accum_n = 0;
    hipStream_t stream = nullptr;
};

namespace {

void trainer_free(po_trainer* tr) {
    auto f = [](void* q) { if (q) (void)hipFree(q); };
    for (void* q : {(void*)tr->p, (void*)tr->g, (void*)tr->m, (void*)tr->v, (void*)tr->sig, (void*)tr->P, (void*)tr->probs,
                    (void*)tr->dlog, (void*)tr->loss, (void*)tr->dact[0], (void*)tr->dact[1], (void*)tr->dA, (void*)tr->dR,
                    (void*)tr->part, (void*)tr->lsm, (void*)tr->logz, (void*)tr->alpha, (void*)tr->beta, (void*)tr->lab,
                    (void*)tr->loff, (void*)tr->pred, (void*)tr->lab8, (void*)tr->poff, (void*)tr->pred_len, (void*)tr->edit,
                    (void*)tr->estatus, (void*)tr->wb, (void*)tr->wb2, (void*)tr->bpart, (void*)tr->ga, (void*)tr->npart,
                    (void*)tr->rec})
        f(q);
    for (float* q : tr->act) f(q);
    for (float* q : tr->save) f(q);
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int64_t split_rows(int64_t M) { return po_train_split_rows(M, 4); }

// grad[0 .. K·N) = sum over the M rows of A[m + shift]ᵀ·B[m] (one call per Conv1D tap: rows p0 .. p0 + K of a K_tot x N
// result); the partial sums of the splits, then their fixed-order combine
int wgrad(po_trainer* tr, const float* A, int64_t lda, const float* B, int64_t ldb, int K, int N, int64_t M, int shift,
          int p0, int Ktot, float* out, bool combine) {
    const int64_t rows = split_rows(M);
    const int nz = (int)((M + rows - 1) / rows);
    const int64_t pstride = (int64_t)Ktot * N;
    if ((int64_t)nz * pstride > tr->part_cap) return po_fail(PO_E_CAP, "po_train_step: split-K buffer too small");
    hipLaunchKernelGGL(wgrad_kernel, dim3(blocks(K, 64), blocks(N, 64), nz), dim3(256), 0, tr->stream, A, lda, B, ldb, K, N,
                       M, tr->T, shift, rows, tr->part, N, p0, pstride);
    if (combine)
        hipLaunchKernelGGL(combine_kernel, dim3(blocks(pstride, 256)), dim3(256), 0, tr->stream, tr->part, nz, pstride,
                           pstride, out);
    return PO_OK;
}

// grad[0 .. K·384) = sum over the M rows of bf16(A[m])ᵀ·bf16(D[m]) (PO_CALL_BF16: a GRU layer's dW and dU), and bias[0 .. 384)
// = the f32 column sums of the unrounded D (b_in's gradient from dA, b_rec's from dR)
int wgrad_bf16(po_trainer* tr, const float* A, int64_t lda, int K, const float* D, int64_t M, float* out, float* bias) {
    const int64_t rows = po_train_split_rows(M, PO_TRAIN_BF16_ALIGN);
    const int nz = po_train_split_count(M, rows);
    const int64_t pstride = (int64_t)K * G_MAX;
    if (po_train_part_floats(M, rows, K, G_MAX) > tr->part_cap) return po_fail(PO_E_CAP, "po_train_step: split-K buffer too small");
    launch_wgrad_bf16(tr->stream, A, lda, K, D, M, rows, nz, tr->part, pstride, tr->bpart);
    hipLaunchKernelGGL(combine_kernel, dim3(blocks(pstride, 256)), dim3(256), 0, tr->stream, tr->part, nz, pstride, pstride,
                       out);
    hipLaunchKernelGGL(combine_kernel, dim3(blocks(G_MAX, 256)), dim3(256), 0, tr->stream, tr->bpart, nz, (int64_t)G_MAX,
                       (int64_t)G_MAX, bias);
    return PO_OK;
}

int colsum(po_trainer* tr, const float* X, int64_t ldx, int N, int64_t M, float* out) {
    const int64_t rows = split_rows(M);
    const int nz = (int)((M + rows - 1) / rows);
    if ((int64_t)nz * N > tr->part_cap) return po_fail(PO_E_CAP, "po_train_step: split-K buffer too small");
    hipLaunchKernelGGL(colsum_kernel, dim3(blocks(N, 256), nz), dim3(256), 0, tr->stream, X, ldx, N, M, rows, tr->part,
                       (int64_t)N);
    hipLaunchKernelGGL(combine_kernel, dim3(blocks(N, 256)), dim3(256), 0, tr->stream, tr->part, nz, (int64_t)N, (int64_t)N,
                       out);
    return PO_OK;
}

struct Timer {
    po_trainer* tr;
    float* ms;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev;
    int open = -1;
    int begin(int kind) {
        if (!ms) return PO_OK;
        if (open >= 0) { int rc = end(); if (rc) return rc; }
        hipEvent_t a, b;
        PO_HIPCHK(hipEventCreate(&a));
        PO_HIPCHK(hipEventCreate(&b));
        ev.push_back({kind, {a, b}});
        PO_HIPCHK(hipEventRecord(a, tr->stream));
        open = kind;
        return PO_OK;
    }
    int end() {
        if (!ms || open < 0) return PO_OK;
        PO_HIPCHK(hipEventRecord(ev.back().second.second, tr->stream));
        open = -1;
        return PO_OK;
    }
    void finish(bool ok) {
        for (auto& e : ev) {
            float t = 0.f;
            if (ok && hipEventElapsedTime(&t, e.second.first, e.second.second) == hipSuccess) ms[e.first] += t;
            (void)hipEventDestroy(e.second.first);
            (void)hipEventDestroy(e.second.second);
        }
    }
};

int64_t per_dir_weights(const po_call_layer& l) {
    const int64_t H = gru_units(l), G = 3 * H;
    return l.cin * G + H * G + 2 * G;
}

// the forward pass of n windows (tr->sig) into every layer's output and the logits; the GRU recurrences save for BPTT
int train_forward(po_trainer* tr, int n, Timer& tm) {
    const int T = tr->T, H = tr->H, G = tr->G;
    const int64_t M = (int64_t)n * T;
    const float* x = tr->sig;
    int rc;
    if ((rc = tm.begin(0)) != PO_OK) return rc;
    for (size_t k = 0; k < tr->layers.size(); ++k) {
        const po_call_layer& l = tr->layers[k];
        const float* w = tr->p + tr->woff[k];
        float* out = tr->act[k];
        if (l.kind == PO_CALL_CONV) {
            hipLaunchKernelGGL(conv_relu_kernel, dim3((unsigned)M), dim3(256), 0, tr->stream, x, l.cin, w,
                               w + (int64_t)l.kernel * l.cin * l.cout, l.kernel, l.cout, out, M, T);
        } else if (l.kind == PO_CALL_DENSE) {
            hipLaunchKernelGGL(dense_softmax_kernel, dim3(blocks(M, 256)), dim3(256), 0, tr->stream, x, l.cin, w,
                               w + (int64_t)l.cin * NOUT, tr->probs, out, M);
        } else {
            const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
            const int64_t per_dir = per_dir_weights(l);
            if (tr->precision == PO_CALL_BF16)   // po_call_batch's launch: the same bits
                launch_gru_proj_bf16(tr->stream, x, l.cin, nd, w, per_dir, w + (int64_t)l.cin * G + (int64_t)H * G, per_dir, tr->wb,
                                     tr->P, M, tr->bf_cap);
            else
                launch_gru_proj(tr->stream, x, l.cin, w, w + (int64_t)l.cin * G + (int64_t)H * G, per_dir, per_dir, tr->P, M, G, nd);
            RecurArgs ra;
            std::memset(&ra, 0, sizeof(ra));
            for (int d = 0; d < nd; ++d) {
                const float* wd = w + d * per_dir;
                ra.dir[d].P = tr->P + (int64_t)d * M * G;
                ra.dir[d].U = wd + (int64_t)l.cin * G;
                ra.dir[d].brec = wd + (int64_t)l.cin * G + (int64_t)H * G + G;
                ra.dir[d].backward = (d == 1 || l.kind == PO_CALL_GRU_BACK) ? 1 : 0;
                ra.dir[d].rev_out = l.kind == PO_CALL_GRU_BACK ? 1 : 0;
                ra.dir[d].col = d * H;
            }
            ra.out = out;
            ra.out_stride = l.cout;
            ra.n = n;
            ra.T = T;
            PO_FOR_UNITS(H, hipLaunchKernelGGL(gru_recur_save_kernel<HH>, dim3(blocks(n, RT), (unsigned)nd), dim3(HH * 4), 0,
                                               tr->stream, ra, tr->save[2 * k], tr->save[2 * k + 1]));
        }
        x = out;
    }
    return tm.end();
}

int train_backward(po_trainer* tr, int n, Timer& tm) {
    const int T = tr->T, H = tr->H, G = tr->G, SV = SV_N * H;
    const int64_t M = (int64_t)n * T;
    const int nl = (int)tr->layers.size();
    int rc, cur = 0;
    float* dY = tr->dlog;        // gradient of the current layer's output
    for (int k = nl - 1; k >= 0; --k) {
        const po_call_layer& l = tr->layers[k];
        const float* w = tr->p + tr->woff[k];
        float* gw = tr->g + tr->woff[k];
        const float* X = k > 0 ? tr->act[k - 1] : tr->sig;
        float* dX = tr->dact[cur];
        if (l.kind == PO_CALL_DENSE) {
            if ((rc = tm.begin(3)) != PO_OK) return rc;
            if ((rc = wgrad(tr, X, l.cin, dY, NOUT, l.cin, NOUT, M, 0, 0, l.cin, gw, true)) != PO_OK) return rc;
            if ((rc = colsum(tr, dY, NOUT, NOUT, M, gw + (int64_t)l.cin * NOUT)) != PO_OK) return rc;
            if (k > 0)
                hipLaunchKernelGGL(dense_dx_kernel, dim3(blocks(M * l.cin, 256)), dim3(256), 0, tr->stream, dY, w, l.cin,
                                   dX, M);
        } else if (l.kind == PO_CALL_CONV) {
            if ((rc = tm.begin(3)) != PO_OK) return rc;
            const int K = l.kernel, F = l.cout, padl = (K - 1) / 2;
            hipLaunchKernelGGL(relu_mask_kernel, dim3(blocks(M * F, 256)), dim3(256), 0, tr->stream, dY, tr->act[k], M * F);
            for (int j = 0; j < K; ++j)
                if ((rc = wgrad(tr, X, l.cin, dY, F, l.cin, F, M, j - padl, j * l.cin, K * l.cin, gw, j == K - 1)) != PO_OK)
                    return rc;
            if ((rc = colsum(tr, dY, F, F, M, gw + (int64_t)K * l.cin * F)) != PO_OK) return rc;
            if (k > 0)
                hipLaunchKernelGGL(conv_dx_kernel, dim3(blocks(M * l.cin, 256)), dim3(256), 0, tr->stream, dY, w, K, l.cin,
                                   F, dX, M, T);
        } else {
            const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
            const int64_t per_dir = per_dir_weights(l);
            BackArgs ba;
            std::memset(&ba, 0, sizeof(ba));
            for (int d = 0; d < nd; ++d) {
                ba.dir[d].save = tr->save[2 * k + d];
                ba.dir[d].U = w + d * per_dir + (int64_t)l.cin * G;
                ba.dir[d].dA = tr->dA + (int64_t)d * M * G;
                ba.dir[d].dR = tr->dR + (int64_t)d * M * G;
                ba.dir[d].backward = (d == 1 || l.kind == PO_CALL_GRU_BACK) ? 1 : 0;
                ba.dir[d].rev_out = l.kind == PO_CALL_GRU_BACK ? 1 : 0;
                ba.dir[d].col = d * H;
            }
            ba.dout = dY;
            ba.dout_stride = l.cout;
            ba.n = n;
            ba.T = T;
            if ((rc = tm.begin(2)) != PO_OK) return rc;
            PO_FOR_UNITS(H, hipLaunchKernelGGL(gru_back_recur_kernel<HH>, dim3(blocks(n, RT), (unsigned)nd), dim3(HH * 4), 0,
                                               tr->stream, ba));
            if ((rc = tm.begin(3)) != PO_OK) return rc;
            const bool bf16 = tr->precision == PO_CALL_BF16;
            for (int d = 0; d < nd; ++d) {
                float* gd = gw + d * per_dir;
                const float* dAd = tr->dA + (int64_t)d * M * G;
                const float* dRd = tr->dR + (int64_t)d * M * G;
                const float* hp = tr->save[2 * k + d] + SV_HP * H;
                float* gb = gd + (int64_t)l.cin * G + (int64_t)H * G;
                if (bf16) {   // (the bias sums come out of the same passes over dA and dR)
                    if ((rc = wgrad_bf16(tr, X, l.cin, l.cin, dAd, M, gd, gb)) != PO_OK) return rc;
                    if ((rc = wgrad_bf16(tr, hp, SV, H, dRd, M, gd + (int64_t)l.cin * G, gb + G)) != PO_OK) return rc;
                } else {
                    if ((rc = wgrad(tr, X, l.cin, dAd, G, l.cin, G, M, 0, 0, l.cin, gd, true)) != PO_OK) return rc;
                    if ((rc = wgrad(tr, hp, SV, dRd, G, H, G, M, 0, 0, H, gd + (int64_t)l.cin * G, true)) != PO_OK) return rc;
                    if ((rc = colsum(tr, dAd, G, G, M, gb)) != PO_OK) return rc;
                    if ((rc = colsum(tr, dRd, G, G, M, gb + G)) != PO_OK) return rc;
                }
            }
            if (k > 0 && bf16)
                launch_dx_bf16(tr->stream, tr->dA, M * G, w, per_dir, nd, l.cin, tr->wb2, dX, M);
            else if (k > 0)
                hipLaunchKernelGGL(dx_kernel, dim3(blocks(M, 64), blocks(l.cin, 64)), dim3(256), 0, tr->stream, tr->dA, M * G,
                                   w, per_dir, nd, l.cin, dX, M, G);
        }
        dY = dX;
        cur ^= 1;
    }
    return tm.end();
}

// the argument and label checks of a step, for `me` (po_train_step / po_train_eval): loff[0..n] = the windows' label
// offsets, *maxL = the longest label
int check_batch(const po_trainer* tr, const std::string& me, int n, const int32_t* labels_h, const int32_t* label_len_h,
                int merge_repeated, std::vector<int64_t>& loff, int64_t* maxL) {
    if (n < 1 || n > tr->max_batch)
        return po_fail(PO_E_ARG, me + ": " + std::to_string(n) + " windows, the trainer holds 1 to " +
                       std::to_string(tr->max_batch));
    const int T = tr->T;
    loff.assign(n + 1, 0);
    *maxL = 0;
    for (int w = 0; w < n; ++w) {
        const int L = label_len_h[w];
        if (L < 0) return po_fail(PO_E_ARG, me + ": window " + std::to_string(w) + " has a negative label length");
        if (L > 0 && !labels_h) return po_fail(PO_E_ARG, me + ": null labels");
        int rep = 0;
        for (int j = 0; j < L; ++j) {
            const int32_t c = labels_h[loff[w] + j];
            if (c < 0 || c > 3)
                return po_fail(PO_E_ARG, me + ": window " + std::to_string(w) + " has label " + std::to_string(c) +
                               " at position " + std::to_string(j) + " (labels are 0..3 = A C G T)");
            if (j > 0 && c == labels_h[loff[w] + j - 1]) ++rep;
        }
        const int need = L + (merge_repeated ? rep : 0);
        if (need > T)
            return po_fail(PO_E_ARG, me + ": window " + std::to_string(w) + "'s " + std::to_string(L) +
                           " labels need " + std::to_string(need) + " frames, the window has " +
                                            std::to_string(T));
        loff[w + 1] = loff[w] + L;
        *maxL = std::max<int64_t>(*maxL, L);
    }
    return PO_OK;
}

// α / β (with_ab) and the labels: sized by this batch's longest label and label count, grown when a batch needs more
int grow_batch_buffers(po_trainer* tr, int64_t M, int Smax, int64_t n_labels, bool with_ab) {
    const size_t ab = (size_t)M * Smax * 8;
    if (with_ab && ab > tr->ab_cap) {
        if (tr->alpha) (void)hipFree(tr->alpha);
        if (tr->beta) (void)hipFree(tr->beta);
        tr->alpha = tr->beta = nullptr;
        tr->ab_cap = 0;
        PO_HIPCHK(hipMalloc(&tr->alpha, ab));
        PO_HIPCHK(hipMalloc(&tr->beta, ab));
        tr->ab_cap = ab;
    }
    const size_t lb = (size_t)std::max<int64_t>(1, n_labels) * 4;
    if (lb > tr->lab_cap) {
        if (tr->lab) (void)hipFree(tr->lab);
        tr->lab = nullptr;
        tr->lab_cap = 0;
        PO_HIPCHK(hipMalloc(&tr->lab, lb));
        tr->lab_cap = lb;
    }
    return PO_OK;
}

// A step up to and including the backward pass, for `me` (po_train_step / po_train_accumulate): the argument checks, buffer
// growth, uploads, the forward pass, CTC and the backward pass on the trainer's stream; the gradient of the batch-mean
// loss is then in tr->g and the losses in tr->loss (nothing is waited for)
int train_grad(po_trainer* tr, const std::string& me, const float* signal_h, int n, const int32_t* labels_h,
               const int32_t* label_len_h, int merge_repeated, float* loss_h, float* stage_ms_h, Timer& tm) {
    if (!tr || !signal_h || !label_len_h || !loss_h) return po_fail(PO_E_ARG, me + ": null argument");
    std::vector<int64_t> loff;
    int64_t maxL = 0;
    int rc = check_batch(tr, me, n, labels_h, label_len_h, merge_repeated, loff, &maxL);
    if (rc != PO_OK) return rc;
    const int T = tr->T;
    const int64_t M = (int64_t)n * T;
    const int Smax = (int)(2 * maxL + 1);
    if ((rc = grow_batch_buffers(tr, M, Smax, loff[n], true)) != PO_OK) return rc;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + NSTAGE, 0.f);
    PO_HIPCHK(hipMemcpyAsync(tr->sig, signal_h, (size_t)M * 4, hipMemcpyHostToDevice, tr->stream));
    if (loff[n] > 0) PO_HIPCHK(hipMemcpyAsync(tr->lab, labels_h, (size_t)loff[n] * 4, hipMemcpyHostToDevice, tr->stream));
    PO_HIPCHK(hipMemcpyAsync(tr->loff, loff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, tr->stream));
    rc = train_forward(tr, n, tm);
    if (rc == PO_OK) rc = tm.begin(1);
    if (rc == PO_OK) {
        const float* logits = tr->act.back();
        hipLaunchKernelGGL(ctc_lsm_kernel, dim3(blocks(M, 256)), dim3(256), 0, tr->stream, logits, tr->lsm, M);
        hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3((unsigned)n), dim3(256), 0, tr->stream, tr->lsm, tr->lab, tr->loff, T,
                           Smax, merge_repeated ? 1 : 0, 1, tr->alpha, tr->beta, tr->logz);
        hipLaunchKernelGGL(ctc_grad_kernel, dim3(blocks(M, 256)), dim3(256), 0, tr->stream, tr->lsm, tr->lab, tr->loff, n, T,
                           Smax, tr->alpha, tr->beta, tr->logz, 1.f / (float)n, tr->dlog, tr->loss);
        rc = tm.end();
    }
    if (rc == PO_OK) rc = train_backward(tr, n, tm);
    return rc;
}

// the recipe's device buffers, at first use (po_train_create's footprint does not change)
int ensure_recipe(po_trainer* tr, const char* me) {
    if (tr->ga) return PO_OK;
    float* a = nullptr;
    double* b = nullptr;
    po_recipe_record* c = nullptr;
    hipError_t e = hipMalloc(&a, std::max<size_t>((size_t)tr->nw * 4, 4));
    if (e == hipSuccess) e = hipMalloc(&b, std::max<size_t>((size_t)po_recipe_norm_chunks(tr->nw) * 8, 8));
    if (e == hipSuccess) e = hipMalloc(&c, sizeof(po_recipe_record));
    if (e != hipSuccess) {
        if (a) (void)hipFree(a);
        if (b) (void)hipFree(b);
        return po_fail_hip(e, (std::string(me) + ": device allocation").c_str());
    }
    tr->ga = a;
    tr->npart = b;
    tr->rec = c;
    tr->accum_n = 0;
    return PO_OK;
}

// the norm stage of g[0..n) on `stream`: part holds po_recipe_norm_chunks(n) doubles
void launch_grad_norm(hipStream_t stream, const float* g, int64_t n, float clip_norm, double* part, po_recipe_record* rec) {
    const int64_t nparts = po_recipe_norm_chunks(n);
    if (nparts > 0)
        hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)nparts), dim3(PO_RECIPE_NORM_WG), 0, stream, g, n, part);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(64), 0, stream, part, nparts, clip_norm, rec);
}

}  // namespace

extern "C" {

po_trainer* po_train_create(const po_call_layer* layers_h, int n_layers, int max_batch, int T) {
    po_set_error("");
    int64_t nw;
    int units = 0;
    const int64_t wmax = check_model(layers_h, n_layers, &nw, &units);
    if (wmax < 0) return nullptr;
    if (max_batch < 1 || T < 1) {
        po_fail(PO_E_ARG, "po_train_create: max_batch and T must be positive");
        return nullptr;
    }
    po_trainer* tr = new po_trainer;
    tr->layers.assign(layers_h, layers_h + n_layers);
    tr->max_batch = max_batch;
    tr->T = T;
    tr->nw = nw;
    tr->wmax = wmax;
    tr->H = units;
    tr->G = 3 * units;
    const int H = tr->H, G = tr->G, SV = SV_N * H;
    const int64_t M = (int64_t)max_batch * T;
    int64_t off = 0, maxkn = NOUT;
    bool ok = true;
    hipError_t e = hipSuccess;
    auto alloc = [&](void** q, size_t bytes) {
        if (ok && (e = hipMalloc(q, std::max<size_t>(bytes, 4))) != hipSuccess) ok = false;
    };
    for (int k = 0; k < n_layers; ++k) {
        const po_call_layer& l = layers_h[k];
        tr->woff.push_back(off);
        float *a = nullptr, *s0 = nullptr, *s1 = nullptr;
        alloc((void**)&a, (size_t)M * l.cout * 4);
        tr->act.push_back(a);
        if (l.kind == PO_CALL_CONV) {
            off += (int64_t)l.kernel * l.cin * l.cout + l.cout;
            maxkn = std::max<int64_t>(maxkn, (int64_t)l.kernel * l.cin * l.cout);
        } else if (l.kind == PO_CALL_DENSE) {
            off += (int64_t)l.cin * NOUT + NOUT;
            maxkn = std::max<int64_t>(maxkn, (int64_t)l.cin * NOUT);
        } else {
            const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
            off += nd * per_dir_weights(l);
            maxkn = std::max<int64_t>(maxkn, (int64_t)std::max(l.cin, H) * G);
            alloc((void**)&s0, (size_t)M * SV * 4);
            if (nd == 2) alloc((void**)&s1, (size_t)M * SV * 4);
        }
        tr->save.push_back(s0);
        tr->save.push_back(s1);
    }
    tr->part_cap = MAX_SPLIT * maxkn;
    alloc((void**)&tr->p, nw * 4);
    alloc((void**)&tr->g, nw * 4);
    alloc((void**)&tr->m, nw * 4);
    alloc((void**)&tr->v, nw * 4);
    alloc((void**)&tr->sig, (size_t)M * 4);
    alloc((void**)&tr->P, (size_t)2 * M * G * 4);
    alloc((void**)&tr->probs, (size_t)M * NOUT * 4);
    alloc((void**)&tr->dlog, (size_t)M * NOUT * 4);
    alloc((void**)&tr->loss, (size_t)max_batch * 4);
    alloc((void**)&tr->dact[0], (size_t)M * wmax * 4);
    alloc((void**)&tr->dact[1], (size_t)M * wmax * 4);
    alloc((void**)&tr->dA, (size_t)2 * M * G * 4);
    alloc((void**)&tr->dR, (size_t)2 * M * G * 4);
    alloc((void**)&tr->part, (size_t)tr->part_cap * 4);
    alloc((void**)&tr->lsm, (size_t)M * NOUT * 8);
    alloc((void**)&tr->logz, (size_t)max_batch * 8);
    alloc((void**)&tr->loff, (size_t)(max_batch + 1) * 8);
    alloc((void**)&tr->pred, (size_t)M);
    alloc((void**)&tr->poff, (size_t)(max_batch + 1) * 8);
    alloc((void**)&tr->pred_len, (size_t)max_batch * 4);
    alloc((void**)&tr->edit, (size_t)max_batch * 4);
    alloc((void**)&tr->estatus, (size_t)max_batch * 4);
    if (ok && (e = hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking)) != hipSuccess) ok = false;
    if (ok && (e = hipMemset(tr->p, 0, nw * 4)) != hipSuccess) ok = false;
    if (ok && (e = hipMemset(tr->m, 0, nw * 4)) != hipSuccess) ok = false;
    if (ok && (e = hipMemset(tr->v, 0, nw * 4)) != hipSuccess) ok = false;
    if (!ok) {
        po_fail_hip(e, "po_train_create: device allocation");
        trainer_free(tr);
        return nullptr;
    }
    return tr;
}

void po_train_destroy(po_trainer* tr) {
    if (tr) trainer_free(tr);
}

int po_train_set_params(po_trainer* tr, const float* w_h, int64_t n) {
    po_set_error("");
    if (!tr || !w_h) return po_fail(PO_E_ARG, "po_train_set_params: null argument");
    if (n != tr->nw) return po_fail(PO_E_ARG, "po_train_set_params: the model has " + std::to_string(tr->nw) +
                                    " weights, " + std::to_string(n) + " given");
    PO_HIPCHK(hipMemcpy(tr->p, w_h, n * 4, hipMemcpyHostToDevice));
    PO_HIPCHK(hipMemset(tr->m, 0, n * 4));
    PO_HIPCHK(hipMemset(tr->v, 0, n * 4));
    tr->step = 0;
    tr->accum_n = 0;
    return PO_OK;
}

int po_train_get_params(po_trainer* tr, float* w_h, int64_t n) {
    po_set_error("");
    if (!tr || !w_h) return po_fail(PO_E_ARG, "po_train_get_params: null argument");
    if (n != tr->nw) return po_fail(PO_E_ARG, "po_train_get_params: the model has " + std::to_string(tr->nw) +
                                    " weights, " + std::to_string(n) + " asked for");
    PO_HIPCHK(hipStreamSynchronize(tr->stream));
    PO_HIPCHK(hipMemcpy(w_h, tr->p, n * 4, hipMemcpyDeviceToHost));
    return PO_OK;
}

int po_train_last(po_trainer* tr, int n, float* logits_h, float* dlogits_h) {
    po_set_error("");
    if (!tr || n < 1 || n > tr->max_batch) return po_fail(PO_E_ARG, "po_train_last: null trainer or bad window count");
    const size_t b = (size_t)n * tr->T * NOUT * 4;
    PO_HIPCHK(hipStreamSynchronize(tr->stream));
    if (logits_h) PO_HIPCHK(hipMemcpy(logits_h, tr->act.back(), b, hipMemcpyDeviceToHost));
    if (dlogits_h) PO_HIPCHK(hipMemcpy(dlogits_h, tr->dlog, b, hipMemcpyDeviceToHost));
    return PO_OK;
}

int po_train_step(po_trainer* tr, const float* signal_h, int n, const int32_t* labels_h, const int32_t* label_len_h,
                  int merge_repeated, float lr, float beta1, float beta2, float eps, int update, float* loss_h,
                  float* grad_h, float* stage_ms_h) {
    po_set_error("");
    Timer tm{tr, stage_ms_h};
    int rc = train_grad(tr, "po_train_step", signal_h, n, labels_h, label_len_h, merge_repeated, loss_h, stage_ms_h, tm);
    if (rc == PO_OK && update) {
        rc = tm.begin(4);
        tr->step += 1;
        const double t = (double)tr->step;
        const float lr_t = (float)(lr * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
        hipLaunchKernelGGL(adam_kernel, dim3(blocks(tr->nw, 256)), dim3(256), 0, tr->stream, tr->p, tr->g, tr->m, tr->v,
                           tr->nw, lr_t, beta1, beta2, eps);
        if (rc == PO_OK) rc = tm.end();
    }
    if (rc == PO_OK) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = po_fail_hip(e, "po_train_step: launch");
    }
    if (rc == PO_OK) {
        hipError_t e = hipMemcpyAsync(loss_h, tr->loss, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess && grad_h) e = hipMemcpyAsync(grad_h, tr->g, (size_t)tr->nw * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tr->stream);
        if (e != hipSuccess) rc = po_fail_hip(e, "po_train_step: results");
    }
    tm.finish(rc == PO_OK);
    return rc;
}

int po_train_accumulate(po_trainer* tr, const float* signal_h, int n, const int32_t* labels_h, const int32_t* label_len_h,
                        int merge_repeated, float weight, float* loss_h, float* stage_ms_h) {
    po_set_error("");
    if (tr && !std::isfinite(weight)) return po_fail(PO_E_ARG, "po_train_accumulate: weight " + std::to_string(weight) + " (finite)");
    int rc;
    if (tr && (rc = ensure_recipe(tr, "po_train_accumulate")) != PO_OK) return rc;
    Timer tm{tr, stage_ms_h};
    rc = train_grad(tr, "po_train_accumulate", signal_h, n, labels_h, label_len_h, merge_repeated, loss_h, stage_ms_h, tm);
    if (rc == PO_OK) rc = tm.begin(4);
    if (rc == PO_OK) {
        const unsigned nb = blocks((tr->nw + 3) / 4, 256);
        if (tr->accum_n == 0)
            hipLaunchKernelGGL(grad_axpy_kernel<true>, dim3(nb), dim3(256), 0, tr->stream, tr->ga, tr->g, tr->nw, weight);
        else
            hipLaunchKernelGGL(grad_axpy_kernel<false>, dim3(nb), dim3(256), 0, tr->stream, tr->ga, tr->g, tr->nw, weight);
        rc = tm.end();
    }
    if (rc == PO_OK) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = po_fail_hip(e, "po_train_accumulate: launch");
    }
    if (rc == PO_OK) {
        hipError_t e = hipMemcpyAsync(loss_h, tr->loss, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tr->stream);
        if (e != hipSuccess) rc = po_fail_hip(e, "po_train_accumulate: results");
    }
    if (rc == PO_OK) tr->accum_n += 1;
    tm.finish(rc == PO_OK);
    return rc;
}

int po_train_accum_reset(po_trainer* tr) {
    po_set_error("");
    if (!tr) return po_fail(PO_E_ARG, "po_train_accum_reset: null trainer");
    tr->accum_n = 0;
    return PO_OK;
}

int po_train_get_accum(po_trainer* tr, float* g_h, int64_t n) {
    po_set_error("");
    if (!tr || !g_h) return po_fail(PO_E_ARG, std::string("po_train_get_accum: null argument ") + (!tr ? "tr" : "g_h"));
    if (n != tr->nw) return po_fail(PO_E_ARG, "po_train_get_accum: n " + std::to_string(n) + " (the model has " +
                                    std::to_string(tr->nw) + " weights)");
    if (tr->accum_n == 0) return po_fail(PO_E_ARG, "po_train_get_accum: nothing is accumulated");
    PO_HIPCHK(hipStreamSynchronize(tr->stream));
    PO_HIPCHK(hipMemcpy(g_h, tr->ga, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PO_OK;
}

int po_train_set_accum(po_trainer* tr, const float* g_h, int64_t n) {
    po_set_error("");
    if (!tr || !g_h) return po_fail(PO_E_ARG, std::string("po_train_set_accum: null argument ") + (!tr ? "tr" : "g_h"));
    if (n != tr->nw) return po_fail(PO_E_ARG, "po_train_set_accum: n " + std::to_string(n) + " (the model has " +
                                    std::to_string(tr->nw) + " weights)");
    int rc;
    if ((rc = ensure_recipe(tr, "po_train_set_accum")) != PO_OK) return rc;
    PO_HIPCHK(hipStreamSynchronize(tr->stream));
    PO_HIPCHK(hipMemcpy(tr->ga, g_h, (size_t)n * 4, hipMemcpyHostToDevice));
    tr->accum_n = 1;
    return PO_OK;
}

int po_train_apply(po_trainer* tr, float lr, float beta1, float beta2, float eps, float weight_decay, float clip_norm,
                   double* grad_norm_h, int* applied_h) {
    po_set_error("");
    // ---- every refusal, before any launch
    if (!tr) return po_fail(PO_E_ARG, "po_train_apply: null trainer");
    if (!(clip_norm >= 0.f) || !std::isfinite(clip_norm))
        return po_fail(PO_E_ARG, "po_train_apply: clip_norm " + std::to_string(clip_norm) + " (0: no clipping, or positive and finite)");
    if (!(weight_decay >= 0.f) || !std::isfinite(weight_decay))
        return po_fail(PO_E_ARG, "po_train_apply: weight_decay " + std::to_string(weight_decay) + " (0 or positive and finite)");
    if (tr->accum_n == 0) return po_fail(PO_E_ARG, "po_train_apply: nothing is accumulated");
    // Adam's t advances only when the update is applied, which the record says; the kernels are launched with t + 1 and the
    // record comes back with the call's results
    const float lr_t = po_recipe_lr_t(lr, beta1, beta2, tr->step + 1);
    launch_grad_norm(tr->stream, tr->ga, tr->nw, clip_norm, tr->npart, tr->rec);
    hipLaunchKernelGGL(adamw_apply_kernel, dim3(blocks((tr->nw + 3) / 4, 256)), dim3(256), 0, tr->stream, tr->p, tr->ga, tr->m,
                       tr->v, tr->nw, tr->rec, lr_t, beta1, beta2, eps, po_recipe_decay(lr, weight_decay));
    tr->accum_n = 0;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return po_fail_hip(e, "po_train_apply: launch");
    po_recipe_record r;
    e = hipMemcpyAsync(&r, tr->rec, sizeof(r), hipMemcpyDeviceToHost, tr->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(tr->stream);
    if (e != hipSuccess) return po_fail_hip(e, "po_train_apply: results");
    if (r.finite) tr->step += 1;
    if (grad_norm_h) *grad_norm_h = r.norm;
    if (applied_h) *applied_h = r.finite ? 1 : 0;
    return PO_OK;
}

// ---- for po_train_group.hip (po_internal.h): a trainer's accumulator and a batch's checks, nothing launched
int po_trainer_accum_view(po_trainer* tr, po_trainer_accum* out) {
    if (!tr || !out) return po_fail(PO_E_ARG, "po_trainer_accum_view: null argument");
    int rc;
    if ((rc = ensure_recipe(tr, "po_train_group")) != PO_OK) return rc;
    out->ga = tr->ga;
    out->n = tr->nw;
    out->count = &tr->accum_n;
    out->stream = tr->stream;
    return PO_OK;
}

int po_trainer_check_batch(const po_trainer* tr, const char* me, int n, const int32_t* labels_h, const int32_t* label_len_h,
                           int merge_repeated) {
    if (!tr || !me || !label_len_h) return po_fail(PO_E_ARG, std::string(me ? me : "po_trainer_check_batch") + ": null argument");
    std::vector<int64_t> loff;
    int64_t maxL = 0;
    return check_batch(tr, me, n, labels_h, label_len_h, merge_repeated, loff, &maxL);
}

int po_train_get_state(po_trainer* tr, float* m_h, float* v_h, int64_t n, int64_t* step_h) {
    po_set_error("");
    if (!tr || !m_h || !v_h || !step_h)
        return po_fail(PO_E_ARG, std::string("po_train_get_state: null argument ") +
                       (!tr ? "tr" : !m_h ? "m_h" : !v_h ? "v_h" : "step_h"));
    if (n != tr->nw) return po_fail(PO_E_ARG, "po_train_get_state: n " + std::to_string(n) + " (the model has " +
                                    std::to_string(tr->nw) + " weights)");
    PO_HIPCHK(hipStreamSynchronize(tr->stream));
    PO_HIPCHK(hipMemcpy(m_h, tr->m, (size_t)n * 4, hipMemcpyDeviceToHost));
    PO_HIPCHK(hipMemcpy(v_h, tr->v, (size_t)n * 4, hipMemcpyDeviceToHost));
    *step_h = tr->step;
    return PO_OK;
}

int po_train_set_state(po_trainer* tr, const float* m_h, const float* v_h, int64_t n, int64_t step) {
    po_set_error("");
    if (!tr || !m_h || !v_h)
        return po_fail(PO_E_ARG, std::string("po_train_set_state: null argument ") + (!tr ? "tr" : !m_h ? "m_h" : "v_h"));
    if (n != tr->nw) return po_fail(PO_E_ARG, "po_train_set_state: n " + std::to_string(n) + " (the model has " +
                                    std::to_string(tr->nw) + " weights)");
    if (step < 0) return po_fail(PO_E_ARG, "po_train_set_state: step " + std::to_string(step) + " (0 or more)");
    PO_HIPCHK(hipStreamSynchronize(tr->stream));
    PO_HIPCHK(hipMemcpy(tr->m, m_h, (size_t)n * 4, hipMemcpyHostToDevice));
    PO_HIPCHK(hipMemcpy(tr->v, v_h, (size_t)n * 4, hipMemcpyHostToDevice));
    tr->step = step;
    return PO_OK;
}

int po_grad_norm_h(const float* g_h, int64_t n, double* norm_h) {
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (!norm_h || (!g_h && n > 0))
        return po_fail(PO_E_ARG, std::string("po_grad_norm_h: null argument ") + (!norm_h ? "norm_h" : "g_h"));
    if (n < 0) return po_fail(PO_E_ARG, "po_grad_norm_h: n " + std::to_string(n));
    PoDev dg, dpart, drec;
    PO_HIPCHK(dg.up(g_h, (size_t)n * 4));
    PO_HIPCHK(dpart.up(nullptr, (size_t)po_recipe_norm_chunks(n) * 8));
    PO_HIPCHK(drec.up(nullptr, sizeof(po_recipe_record)));
    launch_grad_norm(nullptr, dg, n, 0.f, dpart, drec.as<po_recipe_record>());
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    po_recipe_record r;
    PO_HIPCHK(drec.down(&r, sizeof(r)));
    *norm_h = r.norm;
    return PO_OK;
}

int po_train_eval(po_trainer* tr, const float* signal_h, int n, const int32_t* labels_h, const int32_t* label_len_h,
                  int merge_repeated, float* loss_h, int32_t* edit_h, int32_t* pred_len_h, int32_t* status_h,
                  uint8_t* pred_h, float* stage_ms_h) {
    po_set_error("");
    if (!tr || !signal_h || !label_len_h || !edit_h || !pred_len_h || !status_h)
        return po_fail(PO_E_ARG, "po_train_eval: null argument");
    std::vector<int64_t> loff;
    int64_t maxL = 0;
    int rc = check_batch(tr, "po_train_eval", n, labels_h, label_len_h, merge_repeated, loff, &maxL);
    if (rc != PO_OK) return rc;
    const int T = tr->T;
    const int64_t M = (int64_t)n * T;
    const int Smax = (int)(2 * maxL + 1);
    if ((rc = grow_batch_buffers(tr, M, Smax, loff[n], loss_h != nullptr)) != PO_OK) return rc;
    const size_t nl = (size_t)loff[n];
    if (std::max<size_t>(nl, 1) > tr->lab8_cap) {
        if (tr->lab8) (void)hipFree(tr->lab8);
        tr->lab8 = nullptr;
        tr->lab8_cap = 0;
        PO_HIPCHK(hipMalloc(&tr->lab8, std::max<size_t>(nl, 1)));
        tr->lab8_cap = std::max<size_t>(nl, 1);
    }
    // (pageable host memory: each copy below has left these vectors when its call returns)
    std::vector<uint8_t> lab8(nl);
    for (size_t j = 0; j < nl; ++j) lab8[j] = (uint8_t)labels_h[j];
    std::vector<int64_t> poff(n + 1);
    for (int w = 0; w <= n; ++w) poff[w] = (int64_t)w * T;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + 3, 0.f);
    PO_HIPCHK(hipMemcpyAsync(tr->sig, signal_h, (size_t)M * 4, hipMemcpyHostToDevice, tr->stream));
    if (nl > 0) {
        PO_HIPCHK(hipMemcpyAsync(tr->lab8, lab8.data(), nl, hipMemcpyHostToDevice, tr->stream));
        if (loss_h) PO_HIPCHK(hipMemcpyAsync(tr->lab, labels_h, nl * 4, hipMemcpyHostToDevice, tr->stream));
    }
    PO_HIPCHK(hipMemcpyAsync(tr->loff, loff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, tr->stream));
    PO_HIPCHK(hipMemcpyAsync(tr->poff, poff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, tr->stream));
    Timer tm{tr, stage_ms_h};
    rc = train_forward(tr, n, tm);
    if (rc == PO_OK && loss_h) {
        rc = tm.begin(1);
        if (rc == PO_OK) {
            hipLaunchKernelGGL(ctc_lsm_kernel, dim3(blocks(M, 256)), dim3(256), 0, tr->stream, tr->act.back(), tr->lsm, M);
            hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3((unsigned)n), dim3(256), 0, tr->stream, tr->lsm, tr->lab, tr->loff,
                               T, Smax, merge_repeated ? 1 : 0, 0, tr->alpha, tr->beta, tr->logz);
            hipLaunchKernelGGL(ctc_loss_kernel, dim3(blocks(n, 256)), dim3(256), 0, tr->stream, tr->logz, n, tr->loss);
            rc = tm.end();
        }
    }
    if (rc == PO_OK) rc = tm.begin(2);
    if (rc == PO_OK) {
        po_launch_eval_path(tr->probs, n, T, tr->pred, tr->pred_len, tr->stream);
        po_launch_edit_distance(tr->pred, tr->poff, tr->pred_len, tr->lab8, tr->loff, n, tr->edit, tr->estatus, tr->stream);
        rc = tm.end();
    }
    if (rc == PO_OK) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = po_fail_hip(e, "po_train_eval: launch");
    }
    if (rc == PO_OK) {
        hipError_t e = hipMemcpyAsync(edit_h, tr->edit, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(pred_len_h, tr->pred_len, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(status_h, tr->estatus, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess && loss_h) e = hipMemcpyAsync(loss_h, tr->loss, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess && pred_h) e = hipMemcpyAsync(pred_h, tr->pred, (size_t)M, hipMemcpyDeviceToHost, tr->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tr->stream);
        if (e != hipSuccess) rc = po_fail_hip(e, "po_train_eval: results");
    }
    tm.finish(rc == PO_OK);
    return rc;
}

int po_train_set_precision(po_trainer* tr, int precision) {
    po_set_error("");
    // ---- every refusal, before the first allocation; the trainer stays in the mode it was in
    if (!tr) return po_fail(PO_E_ARG, "po_train_set_precision: null trainer");
    if (precision != PO_CALL_F32 && precision != PO_CALL_BF16)
        return po_fail(PO_E_ARG, "po_train_set_precision: precision " + std::to_string(precision) + " (PO_CALL_F32 or PO_CALL_BF16)");
    int rc;
    if (precision == PO_CALL_BF16 && (rc = check_bf16_units(tr->H, "po_train_set_precision")) != PO_OK) return rc;
    if (precision == PO_CALL_BF16 && !tr->wb) {
        size_t fwd = 1, bwd = 1;   // bf16 elements: the largest layer's copies (a layer's are made in its own stage)
        for (const po_call_layer& l : tr->layers)
            if (l.kind == PO_CALL_BIGRU || l.kind == PO_CALL_GRU || l.kind == PO_CALL_GRU_BACK) {
                const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
                fwd = std::max(fwd, bf_w_elems(l.cin, nd));
                bwd = std::max(bwd, (size_t)nd * l.cin * G_MAX);
            }
        uint16_t *a = nullptr, *b = nullptr;
        float* c = nullptr;
        hipError_t e = hipMalloc(&a, fwd * 2);
        if (e == hipSuccess) e = hipMalloc(&b, bwd * 2);
        if (e == hipSuccess) e = hipMalloc(&c, (size_t)MAX_SPLIT * G_MAX * 4);
        if (e != hipSuccess) {
            if (a) (void)hipFree(a);
            if (b) (void)hipFree(b);
            return po_fail_hip(e, "po_train_set_precision: device allocation");
        }
        tr->wb = a;
        tr->wb2 = b;
        tr->bpart = c;
        tr->bf_cap = bf_blocks_cap();
    }
    tr->precision = precision;
    return PO_OK;
}

int po_train_get_precision(const po_trainer* tr) {
    po_set_error("");
    if (!tr) return po_fail(PO_E_ARG, "po_train_get_precision: null trainer");
    return tr->precision;
}

int po_gru_wgrad_h(const float* a_h, int64_t lda, int64_t M, int K, const float* d_h, int precision, float* out_h) {
    const std::string me = "po_gru_wgrad_h: ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (!a_h || !d_h || !out_h) return po_fail(PO_E_ARG, me + "null argument " + (!a_h ? "a_h" : !d_h ? "d_h" : "out_h"));
    if (M < 0) return po_fail(PO_E_ARG, me + "M " + std::to_string(M));
    if (K < 1) return po_fail(PO_E_ARG, me + "K " + std::to_string(K) + " (at least 1)");
    if (lda < K) return po_fail(PO_E_ARG, me + "lda " + std::to_string(lda) + " (at least K = " + std::to_string(K) + ")");
    if (precision != PO_CALL_F32 && precision != PO_CALL_BF16)
        return po_fail(PO_E_ARG, me + "precision " + std::to_string(precision) + " (PO_CALL_F32 or PO_CALL_BF16)");
    if (M == 0) return PO_OK;
    const bool bf16 = precision == PO_CALL_BF16;
    const int64_t rows = po_train_split_rows(M, bf16 ? PO_TRAIN_BF16_ALIGN : 4);
    const int nz = po_train_split_count(M, rows);
    const int64_t pstride = (int64_t)K * G_MAX;
    PoDev da, dd, dpart, dout;
    PO_HIPCHK(da.up(a_h, (size_t)((M - 1) * lda + K) * 4));   // (the last row ends at its K-th value)
    PO_HIPCHK(dd.up(d_h, (size_t)M * G_MAX * 4));
    PO_HIPCHK(dpart.up(nullptr, (size_t)nz * pstride * 4));
    PO_HIPCHK(dout.up(nullptr, (size_t)pstride * 4));
    if (bf16)
        launch_wgrad_bf16(nullptr, da, lda, K, dd, M, rows, nz, dpart, pstride, nullptr);
    else
        hipLaunchKernelGGL(wgrad_kernel, dim3(blocks(K, 64), blocks(G_MAX, 64), nz), dim3(256), 0, nullptr, da.as<float>(), lda,
                           dd.as<float>(), (int64_t)G_MAX, K, G_MAX, M, 1, 0, rows, dpart.as<float>(), G_MAX, 0, pstride);
    hipLaunchKernelGGL(combine_kernel, dim3(blocks(pstride, 256)), dim3(256), 0, nullptr, dpart.as<float>(), nz, pstride, pstride,
                       dout.as<float>());
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(dout.down(out_h, (size_t)pstride * 4));
    return PO_OK;
}

int po_gru_dx_h(const float* dA_h, int64_t M, int ndir, const float* w_h, int cin, int precision, float* dX_h) {
    const std::string me = "po_gru_dx_h: ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (!dA_h || !w_h || !dX_h) return po_fail(PO_E_ARG, me + "null argument " + (!dA_h ? "dA_h" : !w_h ? "w_h" : "dX_h"));
    if (M < 0) return po_fail(PO_E_ARG, me + "M " + std::to_string(M));
    if (ndir < 1 || ndir > 2) return po_fail(PO_E_ARG, me + "ndir " + std::to_string(ndir) + " (1 or 2)");
    if (cin < 1) return po_fail(PO_E_ARG, me + "cin " + std::to_string(cin) + " (at least 1)");
    if (precision != PO_CALL_F32 && precision != PO_CALL_BF16)
        return po_fail(PO_E_ARG, me + "precision " + std::to_string(precision) + " (PO_CALL_F32 or PO_CALL_BF16)");
    if (M == 0) return PO_OK;
    const int64_t wstride = (int64_t)cin * G_MAX;
    PoDev dda, dw, dwb, ddx;
    PO_HIPCHK(dda.up(dA_h, (size_t)ndir * M * G_MAX * 4));
    PO_HIPCHK(dw.up(w_h, (size_t)ndir * wstride * 4));
    PO_HIPCHK(ddx.up(nullptr, (size_t)M * cin * 4));
    if (precision == PO_CALL_BF16) {
        PO_HIPCHK(dwb.up(nullptr, (size_t)ndir * wstride * 2));
        launch_dx_bf16(nullptr, dda, M * G_MAX, dw, wstride, ndir, cin, dwb, ddx, M);
    } else {
        hipLaunchKernelGGL(dx_kernel, dim3(blocks(M, 64), blocks(cin, 64)), dim3(256), 0, nullptr, dda.as<float>(), M * G_MAX,
                           dw.as<float>(), wstride, ndir, cin, ddx.as<float>(), M, G_MAX);
    }
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ddx.down(dX_h, (size_t)M * cin * 4));
    return PO_OK;
}

}  // extern "C"
