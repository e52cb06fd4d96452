// The two kernels under poreover_amd/tensors.py: tables on the device in, strings out.
//
//   po_ingest_strided   a model's output as it lies in memory — a padded batch, time-major or batch-major, f32 / f16 / bf16 /
//                       f64, any view — to the engine's ragged float64 tables, with po_ingest.hip's bits: the per-frame
//                       arithmetic is po_ingest_rules.h's, called, not restated.
//   po_pack_strings     a decode's strings, each in a slot sized for the longest possible answer, put back to back, so that
//                       the copy to the host is the text.
//
// Both are enqueue-only: no allocation, no synchronisation, no host read of device memory.  The *_h twins at the end reach
// them from host arrays (po_hostbuf.h).
#include <algorithm>
#include <string>

#include "po_device.h"
#include "po_hostbuf.h"
#include "po_ingest_rules.h"

namespace {
__device__ __forceinline__ int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t imax64(int64_t a, int64_t b) { return a > b ? a : b; }

// ------------------------------------------------------------------------------------------------------------ ingest
struct ISArgs {
    const po_ingest_item* items; const int64_t* row_off; int n, C, dtype, reverse;
    int perm[8];
    double* out; int64_t total_rows;
};

__device__ __forceinline__ int elem_bytes(int dtype) { return dtype == PO_DTYPE_F64 ? 8 : (dtype == PO_DTYPE_F32 ? 4 : 2); }

// one element widened to float32 (exact for f16 and bf16; dtype is one of the three) / to double
__device__ __forceinline__ float load_f32(const char* p, int dtype) {
    if (dtype == PO_DTYPE_F32) return *(const float*)p;
    if (dtype == PO_DTYPE_F16) return (float)*(const _Float16*)p;
    return __uint_as_float((uint32_t)*(const uint16_t*)p << 16);
}
__device__ __forceinline__ double load_f64(const char* p, int dtype) {
    return dtype == PO_DTYPE_F64 ? *(const double*)p : (double)load_f32(p, dtype);
}

// v[0..C) of source row `srow` of an item, in the source's column order
template <bool NORM, int CT>
__device__ __forceinline__ void frame_values(const po_ingest_item& it, int64_t srow, int C, int dtype, double* v) {
    const int eb = elem_bytes(dtype);
    const char* p = (const char*)it.base + srow * it.row_stride * eb;
    const int64_t cs = it.col_stride * eb;
    if (NORM) {
        float x[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = (c < C) ? load_f32(p + c * cs, dtype) : 0.f;
        po_ingest_log_softmax_f32(x, CT ? CT : C, v);   // (po_ingest_rules.h)
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < C) v[c] = load_f64(p + c * cs, dtype);
    }
}

// v[k] by a chain of selects: the frame stays in registers
__device__ __forceinline__ double pick(const double* v, int k) {
    double r = v[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) r = (k == c) ? v[c] : r;
    return r;
}

// One frame per lane, consecutive lanes along `out` (ingest_kernel's shape): an item's rows are where its strides put them.
// CT: C as a compile-time constant, 0 = a.C
template <bool NORM, int CT>
__global__ __launch_bounds__(64) void ingest_strided_kernel(ISArgs a) {
    const int C = CT ? CT : a.C;
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < a.total_rows;
         row += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = a.n;   // the item of this row
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.row_off[mid] <= row) lo = mid; else hi = mid; }
        const int64_t t = row - a.row_off[lo];
        const int64_t srow = a.reverse ? a.row_off[lo + 1] - a.row_off[lo] - 1 - t : t;
        const po_ingest_item it = a.items[lo];
        double v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = 0.0;
        frame_values<NORM, CT>(it, srow, C, a.dtype, v);
        double* o = a.out + row * C;
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < C) o[c] = pick(v, a.perm[c]);
    }
}

// The tiled form, for sources whose items interleave (time-major): a workgroup takes TILE_I consecutive items x TILE_T source
// time steps.  Phase 1: a frame per lane with lanes running along the ITEMS — at one time step the frames of adjacent items
// are adjacent in the source, so a wave reads whole lines — and its float64 values go to the LDS tile, one row per item.  Phase
// 2: lanes run along an item's rows of `out` (TILE_T * C contiguous doubles per item; the column permutation and the time
// reversal are applied here, as LDS addresses).  The tile's rows are padded by one double: in phase 1 the lanes of a wave write
// at a stride of one row, TILE_T * C doubles (80 at C = 5: two LDS banks would take them all; 81: thirty-two).
// A workgroup walks the time tiles t0 = blockIdx.x * TILE_T, + gridDim.x * TILE_T, ... of its items up to the longest of them.
constexpr int TILE_I = 32, TILE_T = 16, TILE_THREADS = 256;

template <bool NORM, int CT>
__global__ __launch_bounds__(TILE_THREADS) void ingest_tiled_kernel(ISArgs a) {
    extern __shared__ double tile[];            // TILE_I rows of TILE_T * C + 1
    __shared__ int64_t s_off[TILE_I + 1];
    __shared__ int s_perm[8];
    const int C = CT ? CT : a.C, W = TILE_T * C, LD = W + 1;
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * TILE_I, ni = min(TILE_I, a.n - i0);
    if (tid <= ni) s_off[tid] = a.row_off[i0 + tid];
    if (tid < 8) s_perm[tid] = a.perm[tid];
    __syncthreads();
    int64_t Tmax = 0;
    for (int j = 0; j < ni; ++j) Tmax = imax64(Tmax, s_off[j + 1] - s_off[j]);
    for (int64_t t0 = (int64_t)blockIdx.x * TILE_T; t0 < Tmax; t0 += (int64_t)gridDim.x * TILE_T) {
        for (int f = tid; f < TILE_I * TILE_T; f += TILE_THREADS) {
            const int j = f % TILE_I, tt = f / TILE_I;
            if (j < ni && t0 + tt < s_off[j + 1] - s_off[j]) {
                const po_ingest_item it = a.items[i0 + j];
                double v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] = 0.0;
                frame_values<NORM, CT>(it, t0 + tt, C, a.dtype, v);
                double* d = tile + j * LD + tt * C;
#pragma unroll
                for (int c = 0; c < 8; ++c) if (c < C) d[c] = v[c];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < TILE_I * W; idx += TILE_THREADS) {
            const int j = idx / W, e = idx - j * W;
            if (j >= ni) break;
            const int64_t T = s_off[j + 1] - s_off[j];
            const int nv = (int)imin64(TILE_T, T - t0);   // the item's time steps in this tile (may be <= 0)
            if (e < nv * C) {
                const int lr = e / C, c = e - lr * C;
                const int tt = a.reverse ? nv - 1 - lr : lr;
                const int64_t row0 = s_off[j] + (a.reverse ? T - t0 - nv : t0);
                a.out[row0 * C + e] = tile[j * LD + tt * C + s_perm[c]];
            }
        }
        __syncthreads();
    }
}

template <bool NORM, int CT>
void launch_ingest_strided(const ISArgs& a, bool tiled, hipStream_t stream) {
    if (tiled) {
        const int64_t mean = (a.total_rows + a.n - 1) / a.n;
        const unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>((mean + TILE_T - 1) / TILE_T, 1), 65535);
        const unsigned gy = (unsigned)((a.n + TILE_I - 1) / TILE_I);
        const size_t lds = sizeof(double) * TILE_I * (TILE_T * a.C + 1);
        hipLaunchKernelGGL((ingest_tiled_kernel<NORM, CT>), dim3(gx, gy), dim3(TILE_THREADS), lds, stream, a);
    } else {
        const int64_t blocks = std::min<int64_t>((a.total_rows + 63) / 64, 256 * 32);
        hipLaunchKernelGGL((ingest_strided_kernel<NORM, CT>), dim3((unsigned)blocks), dim3(64), 0, stream, a);
    }
}

// the refusals of po_ingest_strided (and of its twin), before any device work
int ingest_strided_check(const char* who, const void* items, const void* row_off, int n, int C, int dtype, int normalize,
                         const int* perm_h, int64_t total_rows, const void* out) {
    const std::string w(who);
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (total_rows < 0) return po_fail(PO_E_ARG, w + ": negative total_rows");
    if (C < 1 || C > 8) return po_fail(PO_E_ARG, w + ": C must be 1..8");
    const int dt = dtype & ~(PO_INGEST_TILED | PO_INGEST_PER_FRAME);
    if (dt < PO_DTYPE_F32 || dt > PO_DTYPE_F64) return po_fail(PO_E_ARG, w + ": unknown dtype");
    if (perm_h) for (int c = 0; c < C; ++c) if (perm_h[c] < 0 || perm_h[c] >= C) return po_fail(PO_E_ARG, w + ": perm entry outside [0, C)");
    if (normalize && dt == PO_DTYPE_F64) return po_fail(PO_E_UNSUPPORTED, w + ": normalize with float64 input (the reference normalises in the array's own precision)");
    if (n > 0 && total_rows > 0 && (!items || !row_off || !out)) return po_fail(PO_E_ARG, w + ": null items, row_off or out");
    return PO_OK;
}

// ------------------------------------------------------------------------------------------------------------ strings
constexpr int PK_THREADS = 256, PK_PER = 4, PK_TILE = PK_THREADS * PK_PER;   // a scan tile: 1024 strings
struct PKArgs {
    const char* seq; const int64_t* seq_off; const int32_t* seq_len; const int32_t* status; int n;
    char* packed; int64_t* packed_off; int64_t* tsum;   // tsum: tiles + 1 int64 of the workspace
};

// the bytes string i contributes: 0 where its status is not 0, and never more than its slot holds
__device__ __forceinline__ int64_t packed_len(const PKArgs& a, int i) {
    if (i >= a.n || (a.status && a.status[i] != 0)) return 0;
    const int64_t room = a.seq_off[i + 1] - a.seq_off[i];
    return imax64(0, imin64(a.seq_len[i], room));
}

// workgroup-wide exclusive scan of one value per thread (sh: PK_THREADS int64); *total = the sum
__device__ int64_t pk_excl_scan(int64_t v, int64_t* sh, int64_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < PK_THREADS; d <<= 1) {
        const int64_t add = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const int64_t incl = sh[tid];
    *total = sh[PK_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(PK_THREADS) void pack_tile_sum_kernel(PKArgs a) {
    __shared__ int64_t sh[PK_THREADS];
    const int first = blockIdx.x * PK_TILE + threadIdx.x * PK_PER;
    int64_t s = 0, tot;
    for (int k = 0; k < PK_PER; ++k) s += packed_len(a, first + k);
    pk_excl_scan(s, sh, &tot);
    if (threadIdx.x == 0) a.tsum[blockIdx.x] = tot;
}

// one workgroup: the nt tile sums scanned in place (exclusive), the grand total at tsum[nt]
__global__ __launch_bounds__(PK_THREADS) void pack_tiles_scan_kernel(int64_t* tsum, int nt) {
    __shared__ int64_t sh[PK_THREADS];
    int64_t carry = 0;
    for (int b = 0; b < nt; b += PK_THREADS) {
        const int i = b + threadIdx.x;
        int64_t tot;
        const int64_t ex = pk_excl_scan(i < nt ? tsum[i] : 0, sh, &tot);
        if (i < nt) tsum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) tsum[nt] = carry;
}

__global__ __launch_bounds__(PK_THREADS) void pack_offsets_kernel(PKArgs a, int nt) {
    __shared__ int64_t sh[PK_THREADS];
    const int first = blockIdx.x * PK_TILE + threadIdx.x * PK_PER;
    int64_t len[PK_PER], s = 0, tot;
    for (int k = 0; k < PK_PER; ++k) { len[k] = packed_len(a, first + k); s += len[k]; }
    int64_t run = (nt ? a.tsum[blockIdx.x] : 0) + pk_excl_scan(s, sh, &tot);
    for (int k = 0; k < PK_PER; ++k) {
        if (first + k < a.n) a.packed_off[first + k] = run;
        run += len[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.packed_off[a.n] = a.tsum[nt];
}

// a wave per string, its lanes along the bytes
__global__ __launch_bounds__(PK_THREADS) void pack_copy_kernel(PKArgs a) {
    const int lane = threadIdx.x & 63, waves = PK_THREADS / 64;
    for (int i = blockIdx.x * waves + (threadIdx.x >> 6); i < a.n; i += gridDim.x * waves) {
        const int64_t len = packed_len(a, i);
        const char* s = a.seq + a.seq_off[i];
        char* d = a.packed + a.packed_off[i];
        for (int64_t k = lane; k < len; k += 64) d[k] = s[k];
    }
}

int pack_strings_check(const char* who, const void* seq, const void* seq_off, const void* seq_len, int n, const void* packed,
                       const void* packed_off) {
    const std::string w(who);
    if (n < 0) return po_fail(PO_E_ARG, w + ": negative n");
    if (!packed_off) return po_fail(PO_E_ARG, w + ": null packed_off");
    if (n > 0 && (!seq || !seq_off || !seq_len || !packed)) return po_fail(PO_E_ARG, w + ": null seq, seq_off, seq_len or packed");
    return PO_OK;
}
}  // namespace

extern "C" {

int po_ingest_strided(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, int normalize,
                      const int* perm_h, int reverse, int64_t total_rows, double* out, void* stream) {
    po_fail(PO_OK, "");
    int rc = ingest_strided_check("po_ingest_strided", items, row_off, n, C, dtype, normalize, perm_h, total_rows, out);
    if (rc != PO_OK) return rc;
    if (n == 0 || total_rows == 0) return PO_OK;
    ISArgs a;
    a.items = items; a.row_off = row_off; a.n = n; a.C = C; a.reverse = reverse ? 1 : 0;
    a.dtype = dtype & ~(PO_INGEST_TILED | PO_INGEST_PER_FRAME);
    for (int c = 0; c < 8; ++c) a.perm[c] = (perm_h && c < C) ? perm_h[c] : (c < C ? c : 0);
    a.out = out; a.total_rows = total_rows;
    // (the tiled grid has a row of workgroups per 32 items)
    const bool tiled = (dtype & PO_INGEST_TILED) && !(dtype & PO_INGEST_PER_FRAME) && (n + TILE_I - 1) / TILE_I <= 65535;
    hipStream_t s = (hipStream_t)stream;
    if (normalize) { if (C == 5) launch_ingest_strided<true, 5>(a, tiled, s); else launch_ingest_strided<true, 0>(a, tiled, s); }
    else { if (C == 5) launch_ingest_strided<false, 5>(a, tiled, s); else launch_ingest_strided<false, 0>(a, tiled, s); }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

size_t po_pack_strings_workspace_bytes(int n) {
    po_fail(PO_OK, "");
    return al256(sizeof(int64_t) * ((size_t)(std::max(n, 0) + PK_TILE - 1) / PK_TILE + 1));
}

int po_pack_strings(const char* seq, const int64_t* seq_off, const int32_t* seq_len, const int32_t* status, int n,
                    char* packed, int64_t* packed_off, void* ws, size_t ws_bytes, void* stream) {
    po_fail(PO_OK, "");
    int rc = pack_strings_check("po_pack_strings", seq, seq_off, seq_len, n, packed, packed_off);
    if (rc != PO_OK) return rc;
    if (!ws || ws_bytes < po_pack_strings_workspace_bytes(n)) return po_fail(PO_E_CAP, "po_pack_strings: workspace too small");
    const int nt = (n + PK_TILE - 1) / PK_TILE;
    PKArgs a{seq, seq_off, seq_len, status, n, packed, packed_off, (int64_t*)ws};
    hipStream_t s = (hipStream_t)stream;
    if (nt) hipLaunchKernelGGL(pack_tile_sum_kernel, dim3(nt), dim3(PK_THREADS), 0, s, a);
    hipLaunchKernelGGL(pack_tiles_scan_kernel, dim3(1), dim3(PK_THREADS), 0, s, a.tsum, nt);
    hipLaunchKernelGGL(pack_offsets_kernel, dim3(std::max(nt, 1)), dim3(PK_THREADS), 0, s, a, nt);
    if (n) hipLaunchKernelGGL(pack_copy_kernel, dim3(std::min((n + 3) / 4, 256 * 32)), dim3(PK_THREADS), 0, s, a);
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// ---- host twins
int po_ingest_strided_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                        const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, int normalize,
                        const int* perm_h, int reverse, double* out_h) {
    po_fail(PO_OK, "");
    const char* who = "po_ingest_strided_h";
    if (n > 0 && !row_off_h) return po_fail(PO_E_ARG, std::string(who) + ": null items, row_off or out");
    const int64_t rows = n > 0 ? row_off_h[n] : 0;
    const bool have = src_h && item_off_h && row_stride_h && col_stride_h;
    int rc = ingest_strided_check(who, have ? src_h : nullptr, row_off_h, n, C, dtype, normalize, perm_h, rows, out_h);
    if (rc != PO_OK) return rc;
    if (n == 0 || rows == 0) return PO_OK;
    if (row_off_h[0] != 0) return po_fail(PO_E_ARG, std::string(who) + ": row_off[0] must be 0");
    const int dt = dtype & ~(PO_INGEST_TILED | PO_INGEST_PER_FRAME);
    const size_t eb = dt == PO_DTYPE_F64 ? 8 : (dt == PO_DTYPE_F32 ? 4 : 2);
    bool interleaved = n > 1;   // time-major: item i + 1 starts C elements after item i, frames contiguous
    for (int i = 0; i < n; ++i) {
        const int64_t T = row_off_h[i + 1] - row_off_h[i];
        if (T < 0) return po_fail(PO_E_ARG, std::string(who) + ": offsets must not decrease");
        if (item_off_h[i] < 0 || row_stride_h[i] < 0 || col_stride_h[i] < 0) return po_fail(PO_E_ARG, std::string(who) + ": negative offset or stride");
        if (T > 0 && (src_elems <= 0 || (T > 1 && row_stride_h[i] > (src_elems - 1) / (T - 1)) || (C > 1 && col_stride_h[i] > (src_elems - 1) / (C - 1)) ||
                      item_off_h[i] + (T - 1) * row_stride_h[i] + (C - 1) * col_stride_h[i] >= src_elems))
            return po_fail(PO_E_ARG, std::string(who) + ": item " + std::to_string(i) + " reaches past src_elems");
        if (col_stride_h[i] != 1 || (i > 0 && item_off_h[i] != item_off_h[i - 1] + C)) interleaved = false;
    }
    std::vector<po_ingest_item> items(n);
    PoDev src, it, ro, o;
    PO_HIPCHK(src.up(src_h, (size_t)src_elems * eb));
    for (int i = 0; i < n; ++i) items[i] = {src.as<char>() + (size_t)item_off_h[i] * eb, row_stride_h[i], col_stride_h[i]};
    PO_HIPCHK(it.up(items.data(), sizeof(po_ingest_item) * n));
    PO_HIPCHK(ro.up(row_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(o.up(nullptr, sizeof(double) * rows * C));
    const int route = (dtype & (PO_INGEST_TILED | PO_INGEST_PER_FRAME)) ? dtype : (interleaved ? dtype | PO_INGEST_TILED : dtype);
    rc = po_ingest_strided(it.as<po_ingest_item>(), ro, n, C, route, normalize, perm_h, reverse, rows, o, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(o.down(out_h, sizeof(double) * rows * C));
    return PO_OK;
}

int po_pack_strings_h(const char* seq_h, const int64_t* seq_off_h, const int32_t* seq_len_h, const int32_t* status_h, int n,
                      char* packed_h, int64_t* packed_off_h) {
    po_fail(PO_OK, "");
    int rc = pack_strings_check("po_pack_strings_h", seq_h, seq_off_h, seq_len_h, n, packed_h, packed_off_h);
    if (rc != PO_OK) return rc;
    if (n == 0) { packed_off_h[0] = 0; return PO_OK; }
    const PoRagged r(seq_off_h, n, true);
    if (!r.ordered) return po_fail(PO_E_ARG, "po_pack_strings_h: offsets must not decrease");
    PoDev seq, off, len, st, packed, poff, ws;
    PO_HIPCHK(seq.up(seq_h + r.base, (size_t)r.total));
    PO_HIPCHK(off.up(r.off.data(), r.bytes()));
    PO_HIPCHK(len.up(seq_len_h, sizeof(int32_t) * n));
    if (status_h) PO_HIPCHK(st.up(status_h, sizeof(int32_t) * n));
    PO_HIPCHK(packed.up(nullptr, (size_t)r.total));
    PO_HIPCHK(poff.up(nullptr, sizeof(int64_t) * (n + 1)));
    const size_t wsb = po_pack_strings_workspace_bytes(n);
    PO_HIPCHK(ws.up(nullptr, wsb));
    rc = po_pack_strings(seq, off, len, status_h ? st.as<int32_t>() : nullptr, n, packed, poff, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(poff.down(packed_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(packed.down(packed_h, (size_t)std::min<int64_t>(packed_off_h[n], r.total)));
    return PO_OK;
}

}  // extern "C"
