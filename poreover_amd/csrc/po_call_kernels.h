// The basecalling network's forward kernels, shared by `call` (po_call.hip) and `train` (po_train.hip); each translation
// unit that includes this gets its own copy.  What they compute, and how, is described in po_call.hip.
#pragma once
#include "po_device.h"
#include "po_hostbuf.h"

namespace {


// GRU units per direction, H: a multiple of 16 from 16 to H_MAX, one width for the whole model (check_model).  The
// recurrence kernels are templates on H (H / 16 waves of 16 units, G = 3 H gate columns per direction); everything else
// takes a layer's H and G as arguments.
constexpr int H_MAX = 128;
constexpr int G_MAX = 3 * H_MAX;
constexpr int NOUT = 5;         // Dense outputs (A, C, G, T, blank)
constexpr int RT = 16;          // windows per recurrence workgroup (the MFMA's M)

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// out[m][f] = relu(bias[f] + sum_{j, c} x[w][t + j - padl][c] * W[j][c][f]), m = w * T + t, rows outside [0, T) read 0
__global__ __launch_bounds__(256) void conv_relu_kernel(const float* __restrict__ x, int cin, const float* __restrict__ Wt,
                                                        const float* __restrict__ bias, int K, int F, float* __restrict__ out,
                                                        int64_t M, int T) {
    const int64_t m = blockIdx.x;
    const int t = (int)(m % T);
    const int64_t w0 = m - t;
    const int padl = (K - 1) / 2;
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        float acc = 0.f;
        for (int j = 0; j < K; ++j) {
            const int ts = t + j - padl;
            if (ts < 0 || ts >= T) continue;
            const float* xr = x + (w0 + ts) * cin;
            const float* wr = Wt + (int64_t)j * cin * F + f;
            for (int c = 0; c < cin; ++c) acc = fmaf(xr[c], wr[(int64_t)c * F], acc);
        }
        out[m * F + f] = fmaxf(acc + bias[f], 0.f);
    }
}

// P[d][m][c] = sum_k x[m][k] * W[d][k][c] + b_in[d][c] for m < M, c < G, d < ndir.  One wave per 16 rows x 64 columns
// (four 16 x 16 accumulators), four waves per workgroup along the rows; K is walked 4 at a time, zero-filled past cin.
// G is a multiple of 16: the last of a direction's (G + 63) / 64 column tiles may hold fewer than four live 16-column
// sub-tiles, and a dead one neither loads nor stores (the gates' boundaries mean nothing here).  WHOLE: G is a multiple of
// 64 (H = 64 and 128) and every sub-tile is live, known at compile time.
template <bool WHOLE>
__global__ __launch_bounds__(256) void gru_proj_kernel(const float* __restrict__ x, int cin, const float* __restrict__ W,
                                                       const float* __restrict__ bin, int64_t wstride, int64_t bstride,
                                                       float* __restrict__ P, int64_t M, int G) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (m0 >= M) return;
    const int ntile = (G + 63) / 64;
    const int d = blockIdx.y / ntile;
    const int c0 = (blockIdx.y % ntile) * 64;
    const int nq = WHOLE ? 4 : min(4, (G - c0) / 16);   // live sub-tiles (wave-uniform)
    const float* Wd = W + d * wstride;
    const int i = lane & 15, kq = lane >> 4;
    const int64_t arow = m0 + i;
    const bool arow_ok = arow < M;
    f32x4 acc[4];
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < cin; k0 += 4) {
        const int k = k0 + kq;
        const bool kok = k < cin;
        const float a = (arow_ok && kok) ? x[arow * cin + k] : 0.f;
        const float* wr = Wd + (int64_t)k * G + c0 + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mfma4(a, (kok && q < nq) ? wr[q * 16] : 0.f, acc[q]);
    }
    float* Pd = P + (int64_t)d * M * G;
    const float* bd = bin + d * bstride;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q >= nq) break;
        const int col = c0 + q * 16 + i;
        const float b = bd[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + kq * 4 + r;
            if (row < M) Pd[row * G + col] = acc[q][r] + b;
        }
    }
}

// gru_proj_kernel for nd directions on `stream`
inline void launch_gru_proj(hipStream_t stream, const float* x, int cin, const float* W, const float* bin, int64_t wstride,
                            int64_t bstride, float* P, int64_t M, int G, int nd) {
    const dim3 grid((unsigned)((M + 63) / 64), (unsigned)(nd * ((G + 63) / 64)));
    if (G % 64 == 0)
        hipLaunchKernelGGL(gru_proj_kernel<true>, grid, dim3(256), 0, stream, x, cin, W, bin, wstride, bstride, P, M, G);
    else
        hipLaunchKernelGGL(gru_proj_kernel<false>, grid, dim3(256), 0, stream, x, cin, W, bin, wstride, bstride, P, M, G);
}

struct RecurDir {
    const float* P;     // [n * T][G] input projections of this direction
    const float* U;     // [H][G] recurrent kernel
    const float* brec;  // [G] recurrent bias
    int backward;       // walk t = T-1 .. 0
    int rev_out;        // write step s at position s (go_backwards without Bidirectional) instead of at t
    int col;            // first output channel
};
struct RecurArgs {
    RecurDir dir[2];
    float* out;         // [n * T][out_stride]
    int out_stride, n, T;
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// SAVE (training): also write, per walk step s of window w, what backpropagation through time needs to `save` (this
// workgroup's direction) at row
// w * T + s: z, r, h~, u_h = h_prev·U_h + b_rec,h and h_prev, H values each, in this order (rows of SV = 5 H)
enum { SV_Z = 0, SV_R = 1, SV_HH = 2, SV_UH = 3, SV_HP = 4, SV_N = 5 };

// The gates of one (window, unit) element of a step, for both recurrence kernels (this file's f32 one and
// po_call_recur_bf16.h's): px its input projections x_z, x_r, x_h; az, ar, ah its element of h_prev·U per gate; br the
// recurrent bias; h its previous state.  z, rg, hh (h~) and the new state hn come back.
__device__ __forceinline__ void gru_gates(const float (&px)[3], float az, float ar, float ah, const float (&br)[3], float h,
                                          float& z, float& rg, float& hh, float& hn) {
    z = sigmoidf_(px[0] + (az + br[0]));
    rg = sigmoidf_(px[1] + (ar + br[1]));
    hh = tanhf(px[2] + rg * (ah + br[2]));
    hn = z * h + (1.f - z) * hh;
}

// A workgroup of H / 16 waves, 16 units each; hs: h_t in LDS at a row stride of H + 1 (one pad word: the 16 rows of an
// MFMA operand hit distinct banks).  REC (the stage entry po_gru_recur_h alone): also write the recurrent pre-activations
// h_prev·U + b_rec to rec[((d * n + w) * T + t) * 3 H + g * H + unit], d this workgroup's direction, t the frame the step consumed.
template <int H, bool SAVE, bool REC = false>
__device__ __forceinline__ void gru_recur_body(RecurArgs a, float* save, float (&hs)[2][RT][H + 1], float* rec = nullptr) {
    constexpr int G = 3 * H, HS = H + 1, SV = SV_N * H;
    const RecurDir D = a.dir[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int unit = wave * 16 + i;
    const int w0 = blockIdx.x * RT;
    const int T = a.T;
    // this lane's B operands for every k-step and gate: U[4 kk + kq][g * H + unit]
    float u[3][H / 4];
#pragma unroll
    for (int kk = 0; kk < H / 4; ++kk)
#pragma unroll
        for (int g = 0; g < 3; ++g) u[g][kk] = D.U[(4 * kk + kq) * G + g * H + unit];
    float br[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) br[g] = D.brec[g * H + unit];
    for (int e = threadIdx.x; e < 2 * RT * HS; e += blockDim.x) (&hs[0][0][0])[e] = 0.f;
    float h[4] = {0.f, 0.f, 0.f, 0.f};     // (window w0 + kq * 4 + r, unit): the lane's own slice of the state
    bool live[4];
    const float* prow[4];
    float* orow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int w = w0 + kq * 4 + r;
        live[r] = w < a.n;
        prow[r] = D.P + (int64_t)(live[r] ? w : 0) * T * G + unit;
        orow[r] = a.out + (int64_t)(live[r] ? w : 0) * T * a.out_stride + D.col + unit;
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
        const float* hrow = &hs[cur][i][0];
#pragma unroll
        for (int kk = 0; kk < H / 4; ++kk) {
            const float hv = hrow[4 * kk + kq];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = mfma4(hv, u[g][kk], acc[g]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float z, rg, hh, hn;
            gru_gates(px[r], acc[0][r], acc[1][r], acc[2][r], br, h[r], z, rg, hh, hn);
            if (SAVE && live[r]) {
                float* sv = save + ((int64_t)(w0 + kq * 4 + r) * T + s) * SV + unit;
                sv[SV_Z * H] = z;
                sv[SV_R * H] = rg;
                sv[SV_HH * H] = hh;
                sv[SV_UH * H] = acc[2][r] + br[2];
                sv[SV_HP * H] = h[r];
            }
            if (REC && live[r]) {
                float* rv = rec + (((int64_t)blockIdx.y * a.n + w0 + kq * 4 + r) * T + t) * G + unit;
#pragma unroll
                for (int g = 0; g < 3; ++g) rv[g * H] = acc[g][r] + br[g];
            }
            if (live[r]) {
                h[r] = hn;
                hs[cur ^ 1][kq * 4 + r][unit] = hn;
                orow[r][(int64_t)to * a.out_stride] = hn;
            }
        }
        __syncthreads();
    }
}

template <int H>
__global__ __launch_bounds__(H * 4) void gru_recur_kernel(RecurArgs a) {
    __shared__ float hs[2][RT][H + 1];
    gru_recur_body<H, false>(a, nullptr, hs);
}

// gru_recur_kernel that also stores the recurrent pre-activations (REC) to rec[nd][n * T][3 H]
template <int H>
__global__ __launch_bounds__(H * 4) void gru_recur_rec_kernel(RecurArgs a, float* rec) {
    __shared__ float hs[2][RT][H + 1];
    gru_recur_body<H, false, true>(a, nullptr, hs, rec);
}

// STMT with `HH` the compile-time constant equal to H_, one of the supported widths (check_model has refused the others)
#define PO_FOR_UNITS(H_, STMT)                                                             \
    switch (H_) {                                                                          \
        case 16: { constexpr int HH = 16; STMT; } break;                                   \
        case 32: { constexpr int HH = 32; STMT; } break;                                   \
        case 48: { constexpr int HH = 48; STMT; } break;                                   \
        case 64: { constexpr int HH = 64; STMT; } break;                                   \
        case 80: { constexpr int HH = 80; STMT; } break;                                   \
        case 96: { constexpr int HH = 96; STMT; } break;                                   \
        case 112: { constexpr int HH = 112; STMT; } break;                                 \
        case 128: { constexpr int HH = 128; STMT; } break;                                 \
        default: break;                                                                    \
    }

// probs[m][c] = softmax(x[m]·Wd + bd)[c]; logits too when asked
__global__ __launch_bounds__(256) void dense_softmax_kernel(const float* __restrict__ x, int cin, const float* __restrict__ Wd,
                                                            const float* __restrict__ bd, float* __restrict__ probs,
                                                            float* __restrict__ logits, int64_t M) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float acc[NOUT];
    for (int c = 0; c < NOUT; ++c) acc[c] = 0.f;
    const float* xr = x + m * cin;
    for (int k = 0; k < cin; ++k) {
        const float v = xr[k];
#pragma unroll
        for (int c = 0; c < NOUT; ++c) acc[c] = fmaf(v, Wd[k * NOUT + c], acc[c]);
    }
    float mx = -__builtin_inff();
    for (int c = 0; c < NOUT; ++c) { acc[c] += bd[c]; mx = fmaxf(mx, acc[c]); }
    float e[NOUT], sum = 0.f;
    for (int c = 0; c < NOUT; ++c) { e[c] = expf(acc[c] - mx); sum += e[c]; }
    for (int c = 0; c < NOUT; ++c) {
        probs[m * NOUT + c] = e[c] / sum;
        if (logits) logits[m * NOUT + c] = acc[c];
    }
}

// units per direction of a GRU layer, or 0 where cout is not a whole number of directions
inline int gru_units(const po_call_layer& l) {
    const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
    return l.cout > 0 && l.cout % nd == 0 ? l.cout / nd : 0;
}

// the model checked against the weights' length; returns the widest activation (channels) or po_fail(PO_E_*, message)'s code.
// *units: the GRU layers' units per direction (0 for a model without one)
int64_t check_model(const po_call_layer* L, int nl, int64_t* nweights, int* units = nullptr) {
    if (!L || nl < 1) return po_fail(PO_E_ARG, "po_call: empty model");
    int64_t wmax = 1, nw = 0;
    int cin = 1, H = 0;
    for (int k = 0; k < nl; ++k) {
        const po_call_layer& l = L[k];
        if (l.cin != cin) return po_fail(PO_E_ARG, "po_call: layer " + std::to_string(k) + " takes " + std::to_string(l.cin) +
                                         " channels, its input has " + std::to_string(cin));
        if (l.kind == PO_CALL_CONV) {
            if (l.kernel < 1 || l.kernel > 64)
                return po_fail(PO_E_ARG, "po_call: layer " + std::to_string(k) + " is a Conv1D of kernel size " +
                               std::to_string(l.kernel) + " (supported: 1 to 64)");
            if (l.cout < 1)
                return po_fail(PO_E_ARG, "po_call: layer " + std::to_string(k) + " is a Conv1D of " + std::to_string(l.cout) +
                               " filters (at least 1)");
            nw += (int64_t)l.kernel * l.cin * l.cout + l.cout;
        } else if (l.kind == PO_CALL_BIGRU || l.kind == PO_CALL_GRU || l.kind == PO_CALL_GRU_BACK) {
            const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
            const int h = gru_units(l);
            const std::string accepted = " (accepted: 16, 32, 48, 64, 80, 96, 112 or 128 units per direction, one width for "
                                         "every GRU layer)";
            if (h < 16 || h > H_MAX || h % 16 != 0)
                return po_fail(PO_E_UNSUPPORTED, "po_call: layer " + std::to_string(k) + " is a GRU of " + std::to_string(l.cout) +
                               " outputs in " + std::to_string(nd) + " direction" + (nd == 2 ? "s" : "") + ", " +
                               (h ? std::to_string(h) : std::string("not a whole number of")) + " units each" + accepted);
            if (H && h != H)
                return po_fail(PO_E_UNSUPPORTED, "po_call: layer " + std::to_string(k) + " is a GRU of " + std::to_string(h) +
                               " units, an earlier one has " + std::to_string(H) + accepted);
            H = h;
            const int64_t G = 3 * (int64_t)H;
            nw += nd * ((int64_t)l.cin * G + (int64_t)H * G + 2 * G);
        } else if (l.kind == PO_CALL_DENSE) {
            if (k != nl - 1 || l.cout != NOUT) return po_fail(PO_E_UNSUPPORTED, "po_call: the model must end in Dense(5)");
            nw += (int64_t)l.cin * NOUT + NOUT;
        } else {
            return po_fail(PO_E_ARG, "po_call: layer kind " + std::to_string(l.kind));
        }
        cin = l.cout;
        wmax = std::max<int64_t>(wmax, l.cout);
    }
    if (L[nl - 1].kind != PO_CALL_DENSE) return po_fail(PO_E_UNSUPPORTED, "po_call: the model must end in Dense(5)");
    *nweights = nw;
    if (units) *units = H;
    return wmax;
}

}  // namespace
