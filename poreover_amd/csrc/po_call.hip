// The basecalling network's forward pass (`poreover call`) on the device, in f32 throughout by default; under
// po_set_call_precision(PO_CALL_BF16) the GRU input projections alone take bf16 operands (f32 products and sums): the two
// kernels of po_call_bf16.h in place of gru_proj_kernel; under po_set_recur_precision(PO_RECUR_BF16X3) the recurrence's h·U
// alone is three bf16 products of split operands with f32 sums: gru_recur_x3_kernel of po_call_recur_bf16.h in place of
// gru_recur_kernel.  The two selectors are independent.  No fp16, no bf16 anywhere else.
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
//                      windows in one direction and walks their T steps; its H / 16 waves (H units per direction: 16 to
//                      128 in steps of 16, one instantiation each) own 16 hidden units each and keep their 48 columns
//                      of U (H x 48 f32 = 3H/4 VGPRs per lane, 96 at H = 128) in registers for the whole walk; h_t goes
//                      through LDS (double buffered: one barrier per step)
//   gru_recur_x3_kernel  the same launch under PO_RECUR_BF16X3: U split in two bf16 B fragments per lane, h_t through LDS as
//                      two bf16 arrays, 36 v_mfma_f32_16x16x32_bf16 per step for 96 of the f32 form (po_call_recur_bf16.h)
//   dense_softmax_kernel  Dense(5) + softmax, one lane per frame
//
// Keras' GRU (reset_after = True), gates in the order z, r, h:
//   x_z, x_r, x_h = x·W + b_in;   u_z, u_r, u_h = h·U + b_rec
//   z = sigmoid(x_z + u_z);  r = sigmoid(x_r + u_r);  h~ = tanh(x_h + r * u_h);  h' = z * h + (1 - z) * h~
// Windows are independent (h_0 = 0 each) and every element's arithmetic depends only on its own window, so a window's
// output is the same bits whichever batch, tile or chunk it runs in.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "po_call_kernels.h"
#include "po_call_bf16.h"
#include "po_call_recur_bf16.h"

#include "po_host.h"
#include "po_internal.h"

namespace {

std::atomic<int> g_precision{PO_CALL_F32};   // po_set_call_precision: process-wide, read once per po_call_batch call
std::atomic<int> g_recur{PO_RECUR_F32};      // po_set_recur_precision: the same

// room for the bf16 copy of a GRU layer's input kernels: the largest layer's (a layer's copy is made in its own stage)
size_t wb_bytes_for(const po_call_layer* L, int nl) {
    size_t b = 0;
    for (int k = 0; k < nl; ++k)
        if (L[k].kind == PO_CALL_BIGRU || L[k].kind == PO_CALL_GRU || L[k].kind == PO_CALL_GRU_BACK)
            b = std::max(b, al256(bf_w_elems(L[k].cin, L[k].kind == PO_CALL_BIGRU ? 2 : 1) * 2));
    return b;
}

// (P is sized for the widest GRU, whatever the model's)
size_t ws_bytes_for(int64_t M, int64_t wmax) {
    return 2 * al256((size_t)M * wmax * 4) + al256((size_t)2 * M * G_MAX * 4);
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
    return ws_bytes_for((int64_t)n * T, wmax) + (g_precision.load() == PO_CALL_BF16 ? wb_bytes_for(layers_h, n_layers) : 0);
}

int po_set_call_precision(int precision) {
    if (precision != PO_CALL_F32 && precision != PO_CALL_BF16)
        return po_fail(PO_E_ARG, "po_set_call_precision: precision " + std::to_string(precision) + " (PO_CALL_F32 or PO_CALL_BF16)");
    g_precision.store(precision);
    return PO_OK;
}

int po_get_call_precision(void) { return g_precision.load(); }

int po_set_recur_precision(int precision) {
    if (precision != PO_RECUR_F32 && precision != PO_RECUR_BF16X3)
        return po_fail(PO_E_ARG, "po_set_recur_precision: precision " + std::to_string(precision) +
                       " (PO_RECUR_F32 or PO_RECUR_BF16X3)");
    g_recur.store(precision);
    return PO_OK;
}

int po_get_recur_precision(void) { return g_recur.load(); }

int po_call_batch(const float* signal, int n, int T, const po_call_layer* layers_h, int n_layers, const float* weights,
                  int64_t n_weights, float* probs, float* logits, void* ws, size_t ws_bytes, void* stream_,
                  float* stage_ms_h) {
    po_set_error("");
    if (n < 0 || T < 1 || !signal || !weights || !probs) return po_fail(PO_E_ARG, "po_call_batch: null argument or T < 1");
    int64_t nw;
    int units = 0, rc0;
    const int64_t wmax = check_model(layers_h, n_layers, &nw, &units);
    if (wmax < 0) return (int)wmax;
    if (nw != n_weights) return po_fail(PO_E_ARG, "po_call_batch: the model has " + std::to_string(nw) + " weights, " +
                                        std::to_string(n_weights) + " given");
    const bool bf16 = g_precision.load() == PO_CALL_BF16;   // (a mode set after the size query finds the workspace too small)
    const int recur = g_recur.load();
    if (bf16 && (rc0 = check_bf16_units(units, "po_call_batch")) != PO_OK) return rc0;
    if (n == 0) return PO_OK;
    const int64_t M = (int64_t)n * T;
    if (!ws || ws_bytes < ws_bytes_for(M, wmax) + (bf16 ? wb_bytes_for(layers_h, n_layers) : 0))
        return po_fail(PO_E_CAP, "po_call_batch: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    char* p = (char*)ws;
    float* act[2] = {(float*)p, (float*)(p + al256((size_t)M * wmax * 4))};
    float* P = (float*)(p + 2 * al256((size_t)M * wmax * 4));
    uint16_t* Wb = (uint16_t*)(p + ws_bytes_for(M, wmax));
    const int bf_cap = bf16 ? bf_blocks_cap() : 0;
    std::vector<Stage> st;
    auto begin = [&](int kind) -> int {
        if (!stage_ms_h) return PO_OK;
        Stage s;
        s.kind = kind;
        PO_HIPCHK(hipEventCreate(&s.a));
        PO_HIPCHK(hipEventCreate(&s.b));
        st.push_back(s);
        PO_HIPCHK(hipEventRecord(s.a, stream));
        return PO_OK;
    };
    auto end = [&]() -> int {
        if (!stage_ms_h) return PO_OK;
        PO_HIPCHK(hipEventRecord(st.back().b, stream));
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
            const int H = gru_units(l), G = 3 * H;
            const int64_t per_dir = (int64_t)l.cin * G + (int64_t)H * G + 2 * G;   // W, U, bias (2, G)
            if ((rc = begin(1)) != PO_OK) break;
            if (bf16)
                launch_gru_proj_bf16(stream, x, l.cin, nd, w, per_dir, w + (int64_t)l.cin * G + (int64_t)H * G, per_dir, Wb, P, M,
                                     bf_cap);
            else
                launch_gru_proj(stream, x, l.cin, w, w + (int64_t)l.cin * G + (int64_t)H * G, per_dir, per_dir, P, M, G, nd);
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
            launch_gru_recur(stream, H, nd, ra, recur, nullptr);
            rc = end();
            w += nd * per_dir;
        }
        x = out;
        cur ^= 1;
    }
    if (rc == PO_OK) {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = po_fail_hip(e, "po_call_batch: launch");
    }
    if (stage_ms_h) {
        if (rc == PO_OK) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) rc = po_fail_hip(e, "po_call_batch: hipStreamSynchronize");
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
    po_set_error("");
    if (n < 0 || T < 1 || !signal_h || !weights_h || !probs_h) return po_fail(PO_E_ARG, "po_call_batch_h: null argument or T < 1");
    int64_t nw;
    int units = 0, rc0;
    const int64_t wmax = check_model(layers_h, n_layers, &nw, &units);
    if (wmax < 0) return (int)wmax;
    if (nw != n_weights) return po_fail(PO_E_ARG, "po_call_batch_h: the model has " + std::to_string(nw) + " weights, " +
                                        std::to_string(n_weights) + " given");
    if (g_precision.load() == PO_CALL_BF16 && (rc0 = check_bf16_units(units, "po_call_batch_h")) != PO_OK) return rc0;
    if (n == 0) return PO_OK;
    if (stage_ms_h) std::fill(stage_ms_h, stage_ms_h + 4, 0.f);
    // windows per pass: as many as ~4 GiB of workspace holds, a whole number of recurrence tiles (a window's bits do
    // not depend on the pass it runs in)
    const size_t per_window = ws_bytes_for(T, wmax) + (size_t)T * NOUT * 4 * (logits_h ? 2 : 1) + (size_t)T * 4;
    int chunk = (int)std::max<size_t>(1, ((size_t)4 << 30) / per_window);
    if (chunk >= RT) chunk = chunk / RT * RT;
    chunk = std::min(chunk, n);
    const int64_t Mc = (int64_t)chunk * T;
    // (the bf16 copies are a few hundred KB and do not grow with the pass; a mode set by another thread in between is
    // answered by po_call_batch's own check)
    const size_t wsb = ws_bytes_for(Mc, wmax) + (g_precision.load() == PO_CALL_BF16 ? wb_bytes_for(layers_h, n_layers) : 0);
    PoDev dw, dsig, dprob, dlog, dws;   // (dlog stays NULL without a logits output)
    PO_HIPCHK(dw.up(weights_h, (size_t)n_weights * 4));
    PO_HIPCHK(dsig.up(nullptr, (size_t)Mc * 4));
    PO_HIPCHK(dprob.up(nullptr, (size_t)Mc * NOUT * 4));
    if (logits_h) PO_HIPCHK(dlog.up(nullptr, (size_t)Mc * NOUT * 4));
    PO_HIPCHK(dws.up(nullptr, wsb));
    for (int w0 = 0; w0 < n; w0 += chunk) {
        const int nc = std::min(chunk, n - w0);
        const size_t M = (size_t)nc * T;
        PO_HIPCHK(hipMemcpy(dsig, signal_h + (int64_t)w0 * T, M * 4, hipMemcpyHostToDevice));
        const int rc = po_call_batch(dsig, nc, T, layers_h, n_layers, dw, n_weights, dprob, dlog, dws, wsb, nullptr, stage_ms_h);
        if (rc != PO_OK) return rc;
        PO_HIPCHK(dprob.down(probs_h + (int64_t)w0 * T * NOUT, M * NOUT * 4));
        if (logits_h) PO_HIPCHK(dlog.down(logits_h + (int64_t)w0 * T * NOUT, M * NOUT * 4));
    }
    return PO_OK;
}

int po_gru_proj_h(const float* x_h, int64_t M, int cin, int ndir, const float* w_h, const float* bin_h, int precision,
                  float* P_h) {
    const std::string me = "po_gru_proj_h: ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (!x_h || !w_h || !bin_h || !P_h)
        return po_fail(PO_E_ARG, me + "null argument " + (!x_h ? "x_h" : !w_h ? "w_h" : !bin_h ? "bin_h" : "P_h"));
    if (M < 0) return po_fail(PO_E_ARG, me + "M " + std::to_string(M));
    if (cin < 1) return po_fail(PO_E_ARG, me + "cin " + std::to_string(cin) + " (at least 1)");
    if (ndir < 1 || ndir > 2) return po_fail(PO_E_ARG, me + "ndir " + std::to_string(ndir) + " (1 or 2)");
    if (precision != PO_CALL_F32 && precision != PO_CALL_BF16)
        return po_fail(PO_E_ARG, me + "precision " + std::to_string(precision) + " (PO_CALL_F32 or PO_CALL_BF16)");
    if (M == 0) return PO_OK;
    constexpr int G = G_MAX;   // (this entry is the 128-unit projection alone)
    PoDev dx, dw, db, dP, dwb;
    PO_HIPCHK(dx.up(x_h, (size_t)M * cin * 4));
    PO_HIPCHK(dw.up(w_h, (size_t)ndir * cin * G * 4));
    PO_HIPCHK(db.up(bin_h, (size_t)ndir * G * 4));
    PO_HIPCHK(dP.up(nullptr, (size_t)ndir * M * G * 4));
    if (precision == PO_CALL_BF16) {
        PO_HIPCHK(dwb.up(nullptr, bf_w_elems(cin, ndir) * 2));
        launch_gru_proj_bf16(nullptr, dx, cin, ndir, dw, (int64_t)cin * G, db, G, dwb, dP, M, bf_blocks_cap());
    } else {
        launch_gru_proj(nullptr, dx.as<float>(), cin, dw.as<float>(), db.as<float>(), (int64_t)cin * G, (int64_t)G, dP.as<float>(),
                        M, G, ndir);
    }
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(dP.down(P_h, (size_t)ndir * M * G * 4));
    return PO_OK;
}

int po_gru_recur_h(const float* P_h, const float* U_h, const float* brec_h, int n, int T, int H, int kind, int precision,
                   float* out_h, float* rec_h) {
    const std::string me = "po_gru_recur_h: ";
    po_set_error("");
    // ---- every argument error, before the first allocation
    if (!P_h || !U_h || !brec_h || !out_h)
        return po_fail(PO_E_ARG, me + "null argument " + (!P_h ? "P_h" : !U_h ? "U_h" : !brec_h ? "brec_h" : "out_h"));
    if (n < 0) return po_fail(PO_E_ARG, me + "n " + std::to_string(n));
    if (T < 1) return po_fail(PO_E_ARG, me + "T " + std::to_string(T) + " (at least 1)");
    if (H < 16 || H > H_MAX || H % 16 != 0)
        return po_fail(PO_E_ARG, me + "H " + std::to_string(H) + " units (16, 32, 48, 64, 80, 96, 112 or 128)");
    if (kind != PO_CALL_BIGRU && kind != PO_CALL_GRU && kind != PO_CALL_GRU_BACK)
        return po_fail(PO_E_ARG, me + "kind " + std::to_string(kind) + " (PO_CALL_BIGRU, PO_CALL_GRU or PO_CALL_GRU_BACK)");
    if (precision != PO_RECUR_F32 && precision != PO_RECUR_BF16X3)
        return po_fail(PO_E_ARG, me + "precision " + std::to_string(precision) + " (PO_RECUR_F32 or PO_RECUR_BF16X3)");
    if (n == 0) return PO_OK;
    const int nd = kind == PO_CALL_BIGRU ? 2 : 1, G = 3 * H;
    const int64_t M = (int64_t)n * T;
    PoDev dP, dU, db, dout, drec;   // (drec stays NULL without a rec output)
    PO_HIPCHK(dP.up(P_h, (size_t)nd * M * G * 4));
    PO_HIPCHK(dU.up(U_h, (size_t)nd * H * G * 4));
    PO_HIPCHK(db.up(brec_h, (size_t)nd * G * 4));
    PO_HIPCHK(dout.up(nullptr, (size_t)M * nd * H * 4));
    if (rec_h) PO_HIPCHK(drec.up(nullptr, (size_t)nd * M * G * 4));
    RecurArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    for (int d = 0; d < nd; ++d) {   // (as po_call_batch fills it)
        ra.dir[d].P = dP.as<float>() + (int64_t)d * M * G;
        ra.dir[d].U = dU.as<float>() + (int64_t)d * H * G;
        ra.dir[d].brec = db.as<float>() + (int64_t)d * G;
        ra.dir[d].backward = (d == 1 || kind == PO_CALL_GRU_BACK) ? 1 : 0;
        ra.dir[d].rev_out = kind == PO_CALL_GRU_BACK ? 1 : 0;
        ra.dir[d].col = d * H;
    }
    ra.out = dout.as<float>();
    ra.out_stride = nd * H;
    ra.n = n;
    ra.T = T;
    launch_gru_recur(nullptr, H, nd, ra, precision, rec_h ? drec.as<float>() : nullptr);
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(dout.down(out_h, (size_t)M * nd * H * 4));
    if (rec_h) PO_HIPCHK(drec.down(rec_h, (size_t)nd * M * G * 4));
    return PO_OK;
}

}  // extern "C"
