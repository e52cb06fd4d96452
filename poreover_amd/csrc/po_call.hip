// The basecalling network's forward pass (`poreover call`) on the device, in f32 throughout.
//
// Replaces, from network/network.py of the reference: the Keras models of build_model (network.py:15-55: bigru3,
// conv1_bigru3, conv2_bigru3, conv1_gru5) run by call_helper (network.py:253-282) on windows of the scaled signal, and
// tf.nn.softmax.  A model is a list of layers (po_call_layer in include/poreover_hip.h); each runs as one to two launches
// over every window of the batch:
//
//   conv_relu_kernel   Conv1D(padding "same", stride 1) + bias + ReLU, direct: one workgroup per frame, one lane per filter
//   gru_proj_kernel    a GRU layer's input projection x·W + b_in for all timesteps of all windows and both directions:
//                      a time-parallel GEMM on v_mfma_f32_16x16x4_f32 (a k-ordered fma chain per element)
//   gru_recur_kernel   the recurrence, ONE persistent launch per layer covering both directions: a workgroup owns 16
//                      windows in one direction and walks their T steps; its 8 waves own 16 hidden units each and keep
//                      their 48 columns of U (128 x 48 f32 = 96 VGPRs per lane) in registers for the whole walk; h_t
//                      goes through LDS (double buffered: one barrier per step)
//   dense_softmax_kernel  Dense(5) + softmax, one lane per frame
//
// Keras' GRU (reset_after = True), gates in the order z, r, h:
//   x_z, x_r, x_h = x·W + b_in;   u_z, u_r, u_h = h·U + b_rec
//   z = sigmoid(x_z + u_z);  r = sigmoid(x_r + u_r);  h~ = tanh(x_h + r * u_h);  h' = z * h + (1 - z) * h~
// Windows are independent (h_0 = 0 each) and every element's arithmetic depends only on its own window, so a window's
// output is the same bits whichever batch, tile or chunk it runs in.
#include <algorithm>
#include <cstring>
#include <vector>

#include "po_device.h"

extern "C" void po_set_error(const char* msg);

namespace {

constexpr int H = 128;          // GRU units
constexpr int G = 3 * H;        // gate columns per direction
constexpr int NOUT = 5;         // Dense outputs (A, C, G, T, blank)
constexpr int RT = 16;          // windows per recurrence workgroup (the MFMA's M)
constexpr int RWAVES = H / 16;  // 8 waves, 16 units each
constexpr int HS = H + 1;       // LDS row stride of h (one pad word: the 16 rows of an MFMA operand hit distinct banks)

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

// P[d][m][c] = sum_k x[m][k] * W[d][k][c] + b_in[d][c] for m < M, c < 384, d < ndir.  One wave per 16 rows x 64 columns
// (four 16 x 16 accumulators), four waves per workgroup along the rows; K is walked 4 at a time, zero-filled past cin.
__global__ __launch_bounds__(256) void gru_proj_kernel(const float* __restrict__ x, int cin, const float* __restrict__ W,
                                                       const float* __restrict__ bin, int64_t wstride, int64_t bstride,
                                                       float* __restrict__ P, int64_t M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (m0 >= M) return;
    const int d = blockIdx.y / (G / 64);
    const int c0 = (blockIdx.y % (G / 64)) * 64;
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
        for (int q = 0; q < 4; ++q) acc[q] = mfma4(a, kok ? wr[q * 16] : 0.f, acc[q]);
    }
    float* Pd = P + (int64_t)d * M * G;
    const float* bd = bin + d * bstride;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col = c0 + q * 16 + i;
        const float b = bd[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + kq * 4 + r;
            if (row < M) Pd[row * G + col] = acc[q][r] + b;
        }
    }
}

struct RecurDir {
    const float* P;     // [n * T][384] input projections of this direction
    const float* U;     // [128][384] recurrent kernel
    const float* brec;  // [384] recurrent bias
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

__global__ __launch_bounds__(RWAVES * 64) void gru_recur_kernel(RecurArgs a) {
    __shared__ float hs[2][RT][HS];
    const RecurDir D = a.dir[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int unit = wave * 16 + i;
    const int w0 = blockIdx.x * RT;
    const int T = a.T;
    // this lane's B operands for every k-step and gate: U[4 kk + kq][g * 128 + unit]
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
            const float z = sigmoidf_(px[r][0] + (acc[0][r] + br[0]));
            const float rg = sigmoidf_(px[r][1] + (acc[1][r] + br[1]));
            const float hh = tanhf(px[r][2] + rg * (acc[2][r] + br[2]));
            const float hn = z * h[r] + (1.f - z) * hh;
            if (live[r]) {
                h[r] = hn;
                hs[cur ^ 1][kq * 4 + r][unit] = hn;
                orow[r][(int64_t)to * a.out_stride] = hn;
            }
        }
        __syncthreads();
    }
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

thread_local std::string g_call_err;
int call_fail(int code, const std::string& msg) {
    g_call_err = msg;
    po_set_error(msg.c_str());
    return code;
}
int call_hip(hipError_t e, const char* what) {
    return call_fail(PO_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define CALLCHK(x)                                      \
    do {                                                \
        hipError_t e_ = (x);                            \
        if (e_ != hipSuccess) return call_hip(e_, #x);  \
    } while (0)

// the model checked against the weights' length; returns the widest activation (channels) or a PO_E_* code
int64_t check_model(const po_call_layer* L, int nl, int64_t* nweights) {
    if (!L || nl < 1) return call_fail(PO_E_ARG, "po_call: empty model");
    int64_t wmax = 1, nw = 0;
    int cin = 1;
    for (int k = 0; k < nl; ++k) {
        const po_call_layer& l = L[k];
        if (l.cin != cin) return call_fail(PO_E_ARG, "po_call: layer " + std::to_string(k) + " takes " + std::to_string(l.cin) +
                                                         " channels, its input has " + std::to_string(cin));
        if (l.kind == PO_CALL_CONV) {
            if (l.cout < 1 || l.kernel < 1 || l.kernel > 64) return call_fail(PO_E_ARG, "po_call: conv filters / kernel size");
            nw += (int64_t)l.kernel * l.cin * l.cout + l.cout;
        } else if (l.kind == PO_CALL_BIGRU || l.kind == PO_CALL_GRU || l.kind == PO_CALL_GRU_BACK) {
            const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
            if (l.cout != nd * H) return call_fail(PO_E_UNSUPPORTED, "po_call: GRU layers have 128 units per direction");
            nw += nd * ((int64_t)l.cin * G + (int64_t)H * G + 2 * G);
        } else if (l.kind == PO_CALL_DENSE) {
            if (k != nl - 1 || l.cout != NOUT) return call_fail(PO_E_UNSUPPORTED, "po_call: the model must end in Dense(5)");
            nw += (int64_t)l.cin * NOUT + NOUT;
        } else {
            return call_fail(PO_E_ARG, "po_call: layer kind " + std::to_string(l.kind));
        }
        cin = l.cout;
        wmax = std::max<int64_t>(wmax, l.cout);
    }
    if (L[nl - 1].kind != PO_CALL_DENSE) return call_fail(PO_E_UNSUPPORTED, "po_call: the model must end in Dense(5)");
    *nweights = nw;
    return wmax;
}

inline size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

size_t ws_bytes_for(int64_t M, int64_t wmax) {
    return 2 * al256((size_t)M * wmax * 4) + al256((size_t)2 * M * G * 4);
}

struct Stage {
    hipEvent_t a = nullptr, b = nullptr;
    int kind;
};

}  // namespace

extern "C" {

size_t po_call_workspace_bytes(int n, int T, const po_call_layer* layers_h, int n_layers) {
    int64_t nw;
    const int64_t wmax = check_model(layers_h, n_layers, &nw);
    if (wmax < 0 || n < 0 || T < 1) return 0;
    return ws_bytes_for((int64_t)n * T, wmax);
}

int po_call_batch(const float* signal, int n, int T, const po_call_layer* layers_h, int n_layers, const float* weights,
                  int64_t n_weights, float* probs, float* logits, void* ws, size_t ws_bytes, void* stream_,
                  float* stage_ms_h) {
    g_call_err.clear();
    po_set_error("");
    if (n < 0 || T < 1 || !signal || !weights || !probs) return call_fail(PO_E_ARG, "po_call_batch: null argument or T < 1");
    int64_t nw;
    const int64_t wmax = check_model(layers_h, n_layers, &nw);
    if (wmax < 0) return (int)wmax;
    if (nw != n_weights) return call_fail(PO_E_ARG, "po_call_batch: the model has " + std::to_string(nw) + " weights, " +
                                                        std::to_string(n_weights) + " given");
    if (n == 0) return PO_OK;
    const int64_t M = (int64_t)n * T;
    if (!ws || ws_bytes < ws_bytes_for(M, wmax)) return call_fail(PO_E_CAP, "po_call_batch: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    char* p = (char*)ws;
    float* act[2] = {(float*)p, (float*)(p + al256((size_t)M * wmax * 4))};
    float* P = (float*)(p + 2 * al256((size_t)M * wmax * 4));
    std::vector<Stage> st;
    auto begin = [&](int kind) -> int {
        if (!stage_ms_h) return PO_OK;
        Stage s;
        s.kind = kind;
        CALLCHK(hipEventCreate(&s.a));
        CALLCHK(hipEventCreate(&s.b));
        st.push_back(s);
        CALLCHK(hipEventRecord(s.a, stream));
        return PO_OK;
    };
    auto end = [&]() -> int {
        if (!stage_ms_h) return PO_OK;
        CALLCHK(hipEventRecord(st.back().b, stream));
        return PO_OK;
    };
    const float* x = signal;
    const float* w = weights;
    int rc = PO_OK, cur = 0;
    for (int k = 0; k < n_layers && rc == PO_OK; ++k) {
        const po_call_layer& l = layers_h[k];
        float* out = act[cur];
        if (l.kind == PO_CALL_CONV) {
            if ((rc = begin(0)) != PO_OK) break;
            hipLaunchKernelGGL(conv_relu_kernel, dim3((unsigned)M), dim3(256), 0, stream, x, l.cin, w,
                               w + (int64_t)l.kernel * l.cin * l.cout, l.kernel, l.cout, out, M, T);
            rc = end();
            w += (int64_t)l.kernel * l.cin * l.cout + l.cout;
        } else if (l.kind == PO_CALL_DENSE) {
            if ((rc = begin(3)) != PO_OK) break;
            hipLaunchKernelGGL(dense_softmax_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, x, l.cin, w,
                               w + (int64_t)l.cin * NOUT, probs, logits, M);
            rc = end();
            w += (int64_t)l.cin * NOUT + NOUT;
            break;
        } else {
            const int nd = l.kind == PO_CALL_BIGRU ? 2 : 1;
            const int64_t per_dir = (int64_t)l.cin * G + (int64_t)H * G + 2 * G;   // W, U, bias (2, 384)
            if ((rc = begin(1)) != PO_OK) break;
            hipLaunchKernelGGL(gru_proj_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)(nd * (G / 64))), dim3(256), 0,
                               stream, x, l.cin, w, w + (int64_t)l.cin * G + (int64_t)H * G, per_dir, per_dir, P, M);
            if ((rc = end()) != PO_OK) break;
            RecurArgs ra;
            std::memset(&ra, 0, sizeof(ra));
            for (int d = 0; d < nd; ++d) {
                const float* wd = w + d * per_dir;
                ra.dir[d].P = P + (int64_t)d * M * G;
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
            if ((rc = begin(2)) != PO_OK) break;
            hipLaunchKernelGGL(gru_recur_kernel, dim3((unsigned)((n + RT - 1) / RT), (unsigned)nd), dim3(RWAVES * 64), 0,
                               stream, ra);
            rc = end();
            w += nd * per_dir;
        }
        x = out;
        cur ^= 1;
    }
    if (rc == PO_OK) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = call_hip(e, "po_call_batch: launch");
    }
    if (stage_ms_h) {
        if (rc == PO_OK) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) rc = call_hip(e, "po_call_batch: hipStreamSynchronize");
        }
        for (auto& s : st) {
            float ms = 0.f;
            if (rc == PO_OK && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) stage_ms_h[s.kind] += ms;
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
    }
    return rc;
}

int po_call_batch_h(const float* signal_h, int n, int T, const po_call_layer* layers_h, int n_layers,
                    const float* weights_h, int64_t n_weights, float* probs_h, float* logits_h, float* stage_ms_h) {
    g_call_err.clear();
    po_set_error("");
    if (n < 0 || T < 1 || !signal_h || !weights_h || !probs_h) return call_fail(PO_E_ARG, "po_call_batch_h: null argument or T < 1");
    int64_t nw;
    const int64_t wmax = check_model(layers_h, n_layers, &nw);
    if (wmax < 0) return (int)wmax;
    if (nw != n_weights) return call_fail(PO_E_ARG, "po_call_batch_h: the model has " + std::to_string(nw) + " weights, " +
                                                        std::to_string(n_weights) + " given");
    if (n == 0) return PO_OK;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + 4, 0.f);
    // windows per pass: as many as ~4 GiB of workspace holds, a whole number of recurrence tiles (a window's bits do
    // not depend on the pass it runs in)
    const size_t per_window = ws_bytes_for(T, wmax) + (size_t)T * NOUT * 4 * (logits_h ? 2 : 1) + (size_t)T * 4;
    int chunk = (int)std::max<size_t>(1, ((size_t)4 << 30) / per_window);
    if (chunk >= RT) chunk = chunk / RT * RT;
    chunk = std::min(chunk, n);
    const int64_t Mc = (int64_t)chunk * T;
    float *dw = nullptr, *dsig = nullptr, *dprob = nullptr, *dlog = nullptr;
    void* dws = nullptr;
    const size_t wsb = ws_bytes_for(Mc, wmax);
    int rc = PO_OK;
    hipError_t e;
    if ((e = hipMalloc(&dw, (size_t)n_weights * 4)) != hipSuccess ||
        (e = hipMalloc(&dsig, (size_t)Mc * 4)) != hipSuccess ||
        (e = hipMalloc(&dprob, (size_t)Mc * NOUT * 4)) != hipSuccess ||
        (logits_h && (e = hipMalloc(&dlog, (size_t)Mc * NOUT * 4)) != hipSuccess) ||
        (e = hipMalloc(&dws, wsb)) != hipSuccess) {
        rc = call_hip(e, "po_call_batch_h: hipMalloc");
    }
    if (rc == PO_OK && (e = hipMemcpy(dw, weights_h, (size_t)n_weights * 4, hipMemcpyHostToDevice)) != hipSuccess)
        rc = call_hip(e, "po_call_batch_h: hipMemcpy (weights)");
    for (int w0 = 0; rc == PO_OK && w0 < n; w0 += chunk) {
        const int nc = std::min(chunk, n - w0);
        const int64_t M = (int64_t)nc * T;
        if ((e = hipMemcpy(dsig, signal_h + (int64_t)w0 * T, (size_t)M * 4, hipMemcpyHostToDevice)) != hipSuccess) {
            rc = call_hip(e, "po_call_batch_h: hipMemcpy (signal)");
            break;
        }
        rc = po_call_batch(dsig, nc, T, layers_h, n_layers, dw, n_weights, dprob, dlog, dws, wsb, nullptr, stage_ms_h);
        if (rc != PO_OK) break;
        if ((e = hipMemcpy(probs_h + (int64_t)w0 * T * NOUT, dprob, (size_t)M * NOUT * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
            (logits_h && (e = hipMemcpy(logits_h + (int64_t)w0 * T * NOUT, dlog, (size_t)M * NOUT * 4, hipMemcpyDeviceToHost)) != hipSuccess))
            rc = call_hip(e, "po_call_batch_h: hipMemcpy (outputs)");
    }
    std::string keep = rc == PO_OK ? std::string() : g_call_err;
    (void)hipFree(dw);
    (void)hipFree(dsig);
    (void)hipFree(dprob);
    if (dlog) (void)hipFree(dlog);
    (void)hipFree(dws);
    if (rc != PO_OK) po_set_error(keep.c_str());
    return rc;
}

}  // extern "C"
