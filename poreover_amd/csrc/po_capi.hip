// C-ABI of libporeover_hip.so (include/poreover_hip.h): argument checks, workspace carving,
// kernel launches, host-buffer conveniences and the HIP-event profiling aid used by bench.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/poreover_hip.h"
#include "po_hostbuf.h"

namespace {
thread_local std::string g_err;   // the one error message of a thread: po_last_error reads it, po_fail / po_set_error write it
}  // namespace
int po_fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int po_fail_hip(hipError_t e, const char* what) { return po_fail(PO_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

namespace {
// alphabet string -> (A, packed bytes); NULL means "ACGT"
inline int pack_alphabet(const char* a, uint32_t* packed) {
    if (!a) a = "ACGT";
    const size_t n = std::strlen(a);
    if (n < 1 || n > 4) return -1;
    uint32_t p = 0;
    for (size_t i = 0; i < n; ++i) p |= (uint32_t)(unsigned char)a[i] << (8 * i);
    *packed = p;
    return (int)n;
}

// ---- per-launch event timing (bench.py's roofline leg) ----
struct ProfRec { hipEvent_t a, b; int kernel; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
double g_prof_ms[PO_K_COUNT];
int64_t g_prof_n[PO_K_COUNT];

struct ProfScope {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    int k;
    bool on;
    ProfScope(int kernel, hipStream_t stream) : s(stream), k(kernel), on(g_prof_on) {
        if (on) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(b, s);
            std::lock_guard<std::mutex> lk(g_prof_mu);
            g_prof.push_back({a, b, k});
        }
    }
};
// brackets the main pair beam kernel (handed to the pair beam launches by po_beam2d_route.hip)
hipEvent_t g_mark_a = nullptr;
void b2_mark(int begin, hipStream_t s) {
    if (!g_prof_on) return;
    if (begin) {
        (void)hipEventCreate(&g_mark_a);
        (void)hipEventRecord(g_mark_a, s);
    } else if (g_mark_a) {
        hipEvent_t b = nullptr;
        (void)hipEventCreate(&b);
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back({g_mark_a, b, PO_K_BEAM2D_MAIN});
        g_mark_a = nullptr;
    }
}
void prof_drain() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) {
        float ms = 0;
        (void)hipEventSynchronize(r.b);
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { g_prof_ms[r.kernel] += ms; g_prof_n[r.kernel]++; }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof.clear();
}
}  // namespace

extern "C" {

int po_version(void) { return 100; }

int po_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int po_set_device(int device) {
    g_err.clear();
    PO_HIPCHK(hipSetDevice(device));
    return PO_OK;
}

const char* po_last_error(void) { return g_err.c_str(); }
// internal: lets the other translation units (po_stream.hip) leave a message for po_last_error
void po_set_error(const char* msg) { g_err = msg ? msg : ""; }

int po_device_info(int device, char* name, int name_cap, int* cus, int* clock_khz, size_t* total_mem) {
    g_err.clear();
    hipDeviceProp_t p;
    PO_HIPCHK(hipGetDeviceProperties(&p, device));
    if (name && name_cap > 0) { std::strncpy(name, p.name, name_cap - 1); name[name_cap - 1] = 0; }
    if (cus) *cus = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    if (total_mem) *total_mem = p.totalGlobalMem;
    return PO_OK;
}

// -------------------------------------------------------------------------------- ingest
int po_ingest_batch(const void* src, const int64_t* row_off, int n, int C, int mode, const int* perm_h, int reverse,
                    double* out, void* stream) {
    g_err.clear();
    if (n < 0 || !src || !row_off || !out) { g_err = "po_ingest_batch: null argument"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    int64_t ends[2] = {0, 0};
    PO_HIPCHK(po_read_ends(row_off, n, (hipStream_t)stream, ends));
    if (ends[0] != 0) { g_err = "po_ingest_batch: row_off[0] must be 0"; return PO_E_ARG; }
    int rc = po_launch_ingest(src, row_off, n, C, mode, perm_h, reverse, ends[1], out, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_ingest_batch: bad C / mode / permutation"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- viterbi
size_t po_viterbi_workspace_bytes(int n, int64_t total_rows, int C, int kind) {
    g_err.clear();
    if (kind != PO_KIND_FLIPFLOP) return 256;
    return al256((size_t)total_rows * 8) + al256((size_t)total_rows) + 256;  // ptr[T][8] + path[T]
}

int po_viterbi_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int kind,
                     int8_t* path, char* seq,
                     const int64_t* seq_off, int32_t* seq_len, int32_t* map, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y || !y_off || !seq || !seq_off || !seq_len || !status) { g_err = "po_viterbi_batch: null argument"; return PO_E_ARG; }
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) { g_err = "po_viterbi_batch: alphabet must have 1..4 symbols"; return PO_E_ARG; }
    int8_t *ff_ptr = nullptr, *ff_path = nullptr;
    if (kind == PO_KIND_FLIPFLOP) {
        if (!ws) { g_err = "po_viterbi_batch: flip-flop needs a workspace"; return PO_E_CAP; }
        int64_t ends[2] = {0, 0};  // total rows, to split and bounds-check the workspace
        PO_HIPCHK(po_read_ends(y_off, n, (hipStream_t)stream, ends));
        const size_t rows = (size_t)(ends[1] - ends[0]);
        if (ws_bytes < al256(rows * 8) + al256(rows)) { g_err = "po_viterbi_batch: workspace too small"; return PO_E_CAP; }
        ff_ptr = (int8_t*)ws;
        ff_path = ff_ptr + al256(rows * 8);
    }
    ProfScope ps(PO_K_VITERBI, (hipStream_t)stream);
    int rc = po_launch_viterbi(y, y_off, n, C, A, ap, kind, path, seq, seq_off, seq_len, map, status, ff_ptr, ff_path,
                               (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_viterbi_batch: unsupported C/kind"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- beam 1-D
size_t po_beam1d_workspace_bytes(int n, int64_t total_rows, int64_t max_rows, int C, int W, int model) {
    g_err.clear();
    (void)max_rows; (void)C; (void)model;
    return 2 * al256(sizeof(int) * (size_t)po_beam1d_arena_nodes(n, total_rows, W)) + 256;
}

// The arena is sized from the rows the CALLER declared when sizing the workspace; the kernel
// bounds-checks every allocation against its own per-read share, so a short workspace yields
// PO_E_CAP here rather than a stray write.
int po_beam1d_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int W, int model,
                    char* seq,
                    const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes,
                    void* stream) {
    g_err.clear();
    if (n < 0 || !y || !y_off || !seq || !seq_off || !seq_len || !status || !ws) { g_err = "po_beam1d_batch: null argument"; return PO_E_ARG; }
    if (ws_bytes < 512) { g_err = "po_beam1d_batch: workspace too small"; return PO_E_CAP; }
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) { g_err = "po_beam1d_batch: alphabet must have 1..4 symbols"; return PO_E_ARG; }
    const size_t half = ((ws_bytes - 256) / 2) / 256 * 256;
    int* apl = (int*)ws;
    int* afc = (int*)((char*)ws + half);
    // total rows, for the capacity check (one small D2H; the rest of the call stays asynchronous)
    int64_t ends[2] = {0, 0};
    PO_HIPCHK(po_read_ends(y_off, n, (hipStream_t)stream, ends));
    if (sizeof(int) * (size_t)po_beam1d_arena_nodes(n, ends[1] - ends[0], W) > half) { g_err = "po_beam1d_batch: workspace too small"; return PO_E_CAP; }
    ProfScope ps(PO_K_BEAM1D, (hipStream_t)stream);
    int rc = po_launch_beam1d(y, y_off, n, C, A, ap, W, model, apl, afc, seq, seq_off, seq_len, status, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_beam1d_batch: unsupported C/model/beam_width"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- beam 2-D
size_t po_beam2d_workspace_bytes(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, int W,
                                 int model, int method) {
    g_err.clear();
    return po_beam2d_ws_bytes_impl(n, tr1, tr2, mr1, mr2, C, W, model, method);
}

int po_beam2d_batch(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                    const int32_t* env, int n, int C, const char* alphabet, int W, int model, int method,
                    char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws,
                    size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y1 || !y1_off || !y2 || !y2_off || !seq || !seq_off || !seq_len || !status || !ws) { g_err = "po_beam2d_batch: null argument"; return PO_E_ARG; }
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) { g_err = "po_beam2d_batch: alphabet must have 1..4 symbols"; return PO_E_ARG; }
    ProfScope ps(PO_K_BEAM2D, (hipStream_t)stream);
    int rc = po_launch_beam2d(y1, y1_off, y2, y2_off, env, n, C, A, ap, W, model, method, seq, seq_off, seq_len, status,
                              ws, ws_bytes, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_beam2d_batch: launch refused"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- forward / acceptor
namespace {
// the largest item of each of two device offset tables (rows and labels, or the two reads of a pair), read back
int batch_maxima(const int64_t* y_off, const int64_t* label_off, int n, hipStream_t s, int64_t* mr, int64_t* ml) {
    std::vector<int64_t> h(2 * (size_t)(n + 1));
    PO_HIPCHK(po_read_tables(y_off, label_off, n, s, h.data()));
    *mr = 0; *ml = 0;
    for (int i = 0; i < n; ++i) {
        *mr = std::max<int64_t>(*mr, h[i + 1] - h[i]);
        *ml = std::max<int64_t>(*ml, h[n + 1 + i + 1] - h[n + 1 + i]);
    }
    return PO_OK;
}
}  // namespace

size_t po_forward_workspace_bytes(int n, int64_t max_rows, int model) {
    g_err.clear(); return po_lattice_ws_bytes(n, max_rows, 0, model, 0); }

int po_forward_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int model,
                     const char* labels, const int64_t* label_off, double* logp, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y || !y_off || !labels || !label_off || !logp || !status || !ws) { g_err = "po_forward_batch: null argument"; return PO_E_ARG; }
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) { g_err = "po_forward_batch: alphabet must have 1..4 symbols"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    int64_t mr = 0, ml = 0;
    int rc = batch_maxima(y_off, label_off, n, (hipStream_t)stream, &mr, &ml);
    if (rc != PO_OK) return rc;
    rc = po_launch_forward(y, y_off, n, C, A, ap, model, labels, label_off, mr, logp, status, ws, ws_bytes, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_forward_batch: unsupported C/model or workspace too small"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

size_t po_viterbi_acceptor_workspace_bytes(int n, int64_t max_rows, int64_t max_label) {
    g_err.clear();
    return po_lattice_ws_bytes(n, max_rows, max_label, PO_MODEL_CTC, 1);
}

int po_viterbi_acceptor_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int band_size,
                              const char* labels, const int64_t* label_off, int32_t* path, int32_t* status, void* ws,
                              size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y || !y_off || !labels || !label_off || !path || !status || !ws) { g_err = "po_viterbi_acceptor_batch: null argument"; return PO_E_ARG; }
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) { g_err = "po_viterbi_acceptor_batch: alphabet must have 1..4 symbols"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    int64_t mr = 0, ml = 0;
    int rc = batch_maxima(y_off, label_off, n, (hipStream_t)stream, &mr, &ml);
    if (rc != PO_OK) return rc;
    rc = po_launch_acceptor(y, y_off, n, C, A, ap, band_size, labels, label_off, mr, ml, path, status, ws, ws_bytes,
                            (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_viterbi_acceptor_batch: unsupported C or workspace too small"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- prefix search
size_t po_prefix_search_workspace_bytes(int n, int64_t max_rows) {
    g_err.clear(); return po_prefix_ws_bytes(n, max_rows); }

int po_prefix_search_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, char* seq,
                           const int64_t* seq_off, int32_t* seq_len, double* logp, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y || !y_off || !seq || !seq_off || !seq_len || !logp || !status || !ws) { g_err = "po_prefix_search_batch: null argument"; return PO_E_ARG; }
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) { g_err = "po_prefix_search_batch: alphabet must have 1..4 symbols"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    std::vector<int64_t> h((size_t)n + 1);
    PO_HIPCHK(hipMemcpyAsync(h.data(), y_off, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, (hipStream_t)stream));
    PO_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int64_t mr = 0;
    for (int i = 0; i < n; ++i) mr = std::max<int64_t>(mr, h[i + 1] - h[i]);
    int rc = po_launch_prefix_search(y, y_off, n, C, A, ap, mr, seq, seq_off, seq_len, logp, status, ws, ws_bytes,
                                     (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_prefix_search_batch: unsupported C / window longer than the LDS rows / workspace too small"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- align / envelope
size_t po_align_workspace_bytes(int n, int64_t ml1, int64_t ml2, int band) {
    g_err.clear(); return po_align_ws_bytes(n, ml1, ml2, band); }

int po_align_batch(const char* seqs, const int64_t* seq_off, int n, int band_width, char* aln1, char* aln2,
                   const int64_t* aln_off, int32_t* ncol, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !seqs || !seq_off || !aln1 || !aln2 || !aln_off || !ncol || !status || !ws) { g_err = "po_align_batch: null argument"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    std::vector<int64_t> h(2 * (size_t)n + 1);
    PO_HIPCHK(hipMemcpyAsync(h.data(), seq_off, sizeof(int64_t) * (2 * n + 1), hipMemcpyDeviceToHost, (hipStream_t)stream));
    PO_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int64_t m1 = 0, m2 = 0;
    for (int i = 0; i < n; ++i) { m1 = std::max<int64_t>(m1, h[2 * i + 1] - h[2 * i]); m2 = std::max<int64_t>(m2, h[2 * i + 2] - h[2 * i + 1]); }
    int rc = po_launch_align(seqs, seq_off, n, band_width, m1, m2, aln1, aln2, aln_off, ncol, status, ws, ws_bytes, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_align_batch: workspace too small"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

size_t po_envelope_workspace_bytes(int n, int64_t max_ncol) {
    g_err.clear(); return po_envelope_ws_bytes(n, max_ncol); }

int po_envelope_batch(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol, int n,
                      const int32_t* map1, const int64_t* map1_off, const int32_t* map2, const int64_t* map2_off,
                      const int32_t* U, const int32_t* V, int padding, int32_t* env, const int64_t* env_off,
                      int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !aln1 || !aln2 || !aln_off || !ncol || !map1 || !map1_off || !map2 || !map2_off || !U || !V || !env ||
        !env_off || !status || !ws) { g_err = "po_envelope_batch: null argument"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    std::vector<int32_t> h((size_t)n);
    PO_HIPCHK(hipMemcpyAsync(h.data(), ncol, sizeof(int32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    PO_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int64_t mc = 0;
    for (int i = 0; i < n; ++i) mc = std::max<int64_t>(mc, h[i]);
    int rc = po_launch_envelope(aln1, aln2, aln_off, ncol, n, map1, map1_off, map2, map2_off, U, V, padding, mc, env,
                                env_off, status, ws, ws_bytes, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_envelope_batch: workspace too small"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- pair gamma
size_t po_pair_gamma_workspace_bytes(int n, int64_t max_cells, int64_t mr1, int64_t mr2) {
    g_err.clear(); return po_gamma_ws_bytes(n, max_cells, mr1, mr2); }

int po_pair_gamma_batch(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                        const int32_t* env, const int64_t* env_off, int n, int C, int flavor, int64_t max_cells,
                        double* gamma00, double* dense_out, const int64_t* dense_off, int32_t* status, void* ws,
                        size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y1 || !y1_off || !y2 || !y2_off || !gamma00 || !status || !ws || (env && !env_off) ||
        (dense_out && !dense_off)) { g_err = "po_pair_gamma_batch: null argument"; return PO_E_ARG; }
    if (n == 0) return PO_OK;
    int64_t m1 = 0, m2 = 0;
    int rc = batch_maxima(y1_off, y2_off, n, (hipStream_t)stream, &m1, &m2);
    if (rc != PO_OK) return rc;
    rc = po_launch_gamma(y1, y1_off, y2, y2_off, env, env_off, n, C, flavor, max_cells, m1, m2, gamma00, dense_out,
                             dense_off, status, ws, ws_bytes, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_pair_gamma_batch: bad C or workspace too small"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- pair decode
size_t po_pair_decode_workspace_bytes(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C,
                                      const po_pair_options* opt) {
    g_err.clear();
    return po_pair_ws_bytes_impl(n, tr1, tr2, mr1, mr2, C, opt);
}

int po_pair_decode_batch(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n,
                         int C, const po_pair_options* opt, char* seq1d, const int64_t* seq1d_off, int32_t* len1,
                         int32_t* len2, double* identity, int32_t* env_out, char* seq, const int64_t* seq_off,
                         int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y1 || !y1_off || !y2 || !y2_off || !opt || !seq1d || !seq1d_off || !len1 || !len2 || !identity ||
        !seq || !seq_off || !seq_len || !status || !ws) { g_err = "po_pair_decode_batch: null argument"; return PO_E_ARG; }
    int rc = po_launch_pair_decode(y1, y1_off, y2, y2_off, n, C, opt, seq1d, seq1d_off, len1, len2, identity,
                                   env_out, seq, seq_off, seq_len, status, ws, ws_bytes, (hipStream_t)stream);
    if (rc != PO_OK) { g_err = "po_pair_decode_batch: launch refused"; return rc; }
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

// -------------------------------------------------------------------------------- host-buffer forms
// Every twin is its arrays going up (po_hostbuf.h), one launch on the null stream, hipDeviceSynchronize, its outputs coming down;
// a return on the way frees what was allocated.  Input tables are rebased by PoRagged; output tables start at 0.
static size_t ingest_elem_bytes(int mode) { return mode == PO_INGEST_LOGITS_F32 ? 4 : (mode == PO_INGEST_TRACE_U8 ? 1 : 8); }

// stored cells of the largest gamma DP of a batch: the dense box, or the envelope's rows (Gamma.h: end - start + 1 each)
static int64_t gamma_max_cells(const PoRagged& r1, const PoRagged& r2, const int32_t* env_h, const int64_t* env_off_h, int n) {
    int64_t mc = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t U = r1.off[i + 1] - r1.off[i], V = r2.off[i + 1] - r2.off[i];
        int64_t cells = env_h ? 0 : (U + 1) * (V + 1);
        if (env_h) for (int64_t u = 0; u <= U; ++u) { const int64_t w = (int64_t)env_h[2 * (env_off_h[i] + u) + 1] - env_h[2 * (env_off_h[i] + u)] + 1; cells += w > 0 ? w : 0; }
        mc = std::max(mc, cells);
    }
    return mc;
}

int po_ingest_batch_h(const void* src_h, const int64_t* row_off_h, int n, int C, int mode, const int* perm_h, int reverse,
                      double* out_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const size_t rows = (size_t)row_off_h[n];
    PoDev s, ro, o;
    PO_HIPCHK(s.up(src_h, ingest_elem_bytes(mode) * rows * C));
    PO_HIPCHK(ro.up(row_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(o.up(nullptr, sizeof(double) * rows * C));
    int rc = po_ingest_batch(s, ro, n, C, mode, perm_h, reverse, o, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(o.down(out_h, sizeof(double) * rows * C));
    return PO_OK;
}

int po_viterbi_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int kind,
                       int8_t* path_h,
                       char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* map_h,
                       int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r(y_off_h, n);
    PoRows y;
    PoSeqOut out;
    PoDev pt, mp, ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(out.up(seq_off_h, n));
    PO_HIPCHK(pt.up(nullptr, (size_t)r.total));
    PO_HIPCHK(mp.up(nullptr, sizeof(int32_t) * r.total));
    const size_t wsb = po_viterbi_workspace_bytes(n, r.total, C, kind);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_viterbi_batch(y.data, y.off, n, C, alphabet, kind, pt, out.seq, out.off, out.len,
                              map_h ? mp.as<int32_t>() : nullptr, out.status, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    PO_HIPCHK(pt.down(path_h, (size_t)r.total));
    PO_HIPCHK(mp.down(map_h, sizeof(int32_t) * r.total));
    return PO_OK;
}

// decode driver in one call: raw basecaller output up, ingest on the device, Viterbi (beam_width <= 0) or 1-D beam
// search, strings down — `poreover decode` for a batch of files without a host-side log-softmax or a float64 upload
int po_decode_1d_batch_h(const void* src_h, const int64_t* row_off_h, int n, int C, int in_mode, const int* perm_h, int reverse,
                         const char* alphabet, int kind, int beam_width, int model, char* seq_h, const int64_t* seq_off_h,
                         int32_t* seq_len_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    if (!src_h || !row_off_h || !seq_h || !seq_off_h || !seq_len_h || !status_h) return po_fail(PO_E_ARG, "po_decode_1d_batch_h: null argument");
    if (in_mode < 0 || in_mode > 2 || row_off_h[0] != 0) return po_fail(PO_E_ARG, "po_decode_1d_batch_h: bad input mode / offsets");
    const PoRagged r(row_off_h, n);
    PoRows src;
    PoSeqOut out;
    PoDev y, ws;
    PO_HIPCHK(src.up(src_h, r, ingest_elem_bytes(in_mode) * C));
    PO_HIPCHK(y.up(nullptr, sizeof(double) * (size_t)r.total * C));
    PO_HIPCHK(out.up(seq_off_h, n));
    int rc = po_launch_ingest(src.data, src.off, n, C, in_mode, perm_h, reverse, r.total, y, nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_decode_1d_batch_h: bad C / mode / permutation");
    const size_t wsb = beam_width <= 0 ? po_viterbi_workspace_bytes(n, r.total, C, kind)
                                       : po_beam1d_workspace_bytes(n, r.total, r.max, C, beam_width, model);
    PO_HIPCHK(ws.up(nullptr, wsb));
    rc = beam_width <= 0 ? po_viterbi_batch(y, src.off, n, C, alphabet, kind, nullptr, out.seq, out.off, out.len, nullptr,
                                            out.status, ws, wsb, nullptr)
                         : po_beam1d_batch(y, src.off, n, C, alphabet, beam_width, model, out.seq, out.off, out.len, out.status,
                                           ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    return PO_OK;
}

int po_beam1d_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int W,
                      int model, char* seq_h,
                      const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r(y_off_h, n);
    PoRows y;
    PoSeqOut out;
    PoDev ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(out.up(seq_off_h, n));
    const size_t wsb = po_beam1d_workspace_bytes(n, r.total, r.max, C, W, model);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_beam1d_batch(y.data, y.off, n, C, alphabet, W, model, out.seq, out.off, out.len, out.status, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    return PO_OK;
}

int po_pair_gamma_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                          const int32_t* env_h, const int64_t* env_off_h, int n, int C, int flavor, double* gamma00_h,
                          double* dense_out_h, const int64_t* dense_off_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r1(y1_off_h, n), r2(y2_off_h, n);
    const int64_t mc = gamma_max_cells(r1, r2, env_h, env_off_h, n);
    PoRows a, b;
    PoDev ev, eo, g0, dn, dof, st, ws;   // (ev, eo and dn, dof stay NULL without an envelope / a dense output)
    PO_HIPCHK(a.up(y1_h, r1, sizeof(double) * C));
    PO_HIPCHK(b.up(y2_h, r2, sizeof(double) * C));
    if (env_h) { PO_HIPCHK(ev.up(env_h, sizeof(int32_t) * 2 * (size_t)env_off_h[n])); PO_HIPCHK(eo.up(env_off_h, sizeof(int64_t) * (n + 1))); }
    PO_HIPCHK(g0.up(nullptr, sizeof(double) * n));
    if (dense_out_h) { PO_HIPCHK(dn.up(nullptr, sizeof(double) * (size_t)dense_off_h[n])); PO_HIPCHK(dof.up(dense_off_h, sizeof(int64_t) * (n + 1))); }
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_pair_gamma_workspace_bytes(n, mc, r1.max, r2.max);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_pair_gamma_batch(a.data, a.off, b.data, b.off, ev, eo, n, C, flavor, mc, g0, dn, dof, st, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(g0.down(gamma00_h, sizeof(double) * n));
    if (dense_out_h) PO_HIPCHK(dn.down(dense_out_h, sizeof(double) * (size_t)dense_off_h[n]));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_pair_prefix_search_env_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                                      const int32_t* env_h, const int64_t* env_off_h, int n, int C, const char* alphabet,
                                      int flavor, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, double* logp_h,
                                      int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    uint32_t ap = 0;
    const int A = pack_alphabet(alphabet, &ap);
    if (A < 0) return po_fail(PO_E_ARG, "po_pair_prefix_search_env_batch_h: alphabet must have 1..4 symbols");
    const PoRagged r1(y1_off_h, n), r2(y2_off_h, n);
    const int64_t mc = gamma_max_cells(r1, r2, env_h, env_off_h, n);
    std::vector<int64_t> dof((size_t)n + 1, 0);   // gamma goes to the search as full (U + 1) x (V + 1) matrices
    for (int i = 0; i < n; ++i) dof[i + 1] = dof[i] + (r1.off[i + 1] - r1.off[i] + 1) * (r2.off[i + 1] - r2.off[i] + 1);
    PoRows a, b;
    PoSeqOut out;
    PoDev ev, eo, g0, dn, dfo, st, ws, ws2;
    if (env_h) { PO_HIPCHK(ev.up(env_h, sizeof(int32_t) * 2 * (size_t)env_off_h[n])); PO_HIPCHK(eo.up(env_off_h, sizeof(int64_t) * (n + 1))); }
    PO_HIPCHK(a.up(y1_h, r1, sizeof(double) * C));
    PO_HIPCHK(b.up(y2_h, r2, sizeof(double) * C));
    PO_HIPCHK(g0.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(dn.up(nullptr, sizeof(double) * (size_t)dof[n]));
    PO_HIPCHK(dfo.up(dof.data(), sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_pair_gamma_workspace_bytes(n, mc, r1.max, r2.max);
    PO_HIPCHK(ws.up(nullptr, wsb));
    // gamma: dense in the Python paths' own arithmetic (flavor 0, prefix_search.pair_gamma_log: gamma flavour 3; flavor 1,
    // decoding_cy.pair_gamma_log: gamma flavour 1), or the envelope DP of Gamma.h (its own arithmetic: logaddexp, -inf)
    // written out as a full matrix with -inf outside the stored ranges
    int rc = po_pair_gamma_batch(a.data, a.off, b.data, b.off, ev, eo, n, C, env_h ? 0 : (flavor ? 1 : 3), mc, g0, dn, dfo, st, ws,
                                 wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(out.up(seq_off_h, n, true));
    const int64_t mr = std::max(r1.max, r2.max);
    const size_t wsb2 = po_pair_prefix_ws_bytes(n, mr);
    PO_HIPCHK(ws2.up(nullptr, wsb2));
    rc = po_launch_pair_prefix_search(a.data, a.off, b.data, b.off, dn, dfo, n, C, A, ap, flavor, mr, out.seq, out.off, out.len,
                                      out.logp, out.status, ws2, wsb2, nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_pair_prefix_search_env_batch_h: box too long for the LDS rows, or bad C");
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h, logp_h));
    return PO_OK;
}

int po_pair_prefix_search_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                                  int n, int C, const char* alphabet, int flavor, char* seq_h, const int64_t* seq_off_h,
                                  int32_t* seq_len_h, double* logp_h, int32_t* status_h) {
    return po_pair_prefix_search_env_batch_h(y1_h, y1_off_h, y2_h, y2_off_h, nullptr, nullptr, n, C, alphabet, flavor, seq_h,
                                             seq_off_h, seq_len_h, logp_h, status_h);
}

int po_forward_vec_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, int s, int i, int flavor,
                           const double* previous_h, double* out_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    if (!y_h || !y_off_h || !out_h) return po_fail(PO_E_ARG, "po_forward_vec_batch_h: null argument");
    const PoRagged r(y_off_h, n);
    PoRows y;
    PoDev pv, out;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    if (previous_h) PO_HIPCHK(pv.up(previous_h, sizeof(double) * r.total));   // (the n items' rows from previous_h[0] on)
    PO_HIPCHK(out.up(nullptr, sizeof(double) * r.total));
    int rc = po_launch_forward_vec(y.data, y.off, n, C, s, i, flavor, pv, out, nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_forward_vec_batch_h: bad symbol / label length, or previous row missing");
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(out_h, sizeof(double) * r.total));
    return PO_OK;
}

int po_align_scores_batch_h(const char* seqs_h, const int64_t* seq_off_h, int n, int band_width, int match, int mismatch,
                            int gap_cost, char* aln1_h, char* aln2_h, const int64_t* aln_off_h, int32_t* ncol_h,
                            int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    int64_t m1 = 0, m2 = 0;
    for (int i = 0; i < n; ++i) {
        m1 = std::max<int64_t>(m1, seq_off_h[2 * i + 1] - seq_off_h[2 * i]);
        m2 = std::max<int64_t>(m2, seq_off_h[2 * i + 2] - seq_off_h[2 * i + 1]);
    }
    PoDev sq, so, a1, a2, ao, nc, st, ws;
    PO_HIPCHK(sq.up(seqs_h, (size_t)seq_off_h[2 * n]));
    PO_HIPCHK(so.up(seq_off_h, sizeof(int64_t) * (2 * n + 1)));
    PO_HIPCHK(a1.up(nullptr, (size_t)aln_off_h[n]));
    PO_HIPCHK(a2.up(nullptr, (size_t)aln_off_h[n]));
    PO_HIPCHK(ao.up(aln_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(nc.up(nullptr, sizeof(int32_t) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_align_workspace_bytes(n, m1, m2, band_width);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_launch_align_scores(sq, so, n, band_width, match, mismatch, gap_cost, m1, m2, a1, a2, ao, nc, st, ws, wsb, nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_align_scores_batch_h: workspace too small");
    PO_HIPCHK(hipGetLastError());
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(a1.down(aln1_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(a2.down(aln2_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(nc.down(ncol_h, sizeof(int32_t) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_nw_matrix_batch(const char* seqs, const int64_t* seq_off, int n, int match, int mismatch, int gap_cost, int32_t* dp,
                       const int64_t* dp_off, int32_t* status, void* stream) {
    g_err.clear();
    if (n < 0 || !seqs || !seq_off || !dp || !dp_off) { g_err = "po_nw_matrix_batch: null argument"; return PO_E_ARG; }
    return po_launch_nw_matrix(seqs, seq_off, n, match, mismatch, gap_cost, dp, dp_off, status, (hipStream_t)stream);
}
int po_nw_matrix_batch_h(const char* seqs_h, const int64_t* seq_off_h, int n, int match, int mismatch, int gap_cost, int32_t* dp_h,
                         const int64_t* dp_off_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    PoDev sq, so, dp, dpo, st;
    PO_HIPCHK(sq.up(seqs_h, (size_t)seq_off_h[2 * n]));
    PO_HIPCHK(so.up(seq_off_h, sizeof(int64_t) * (2 * n + 1)));
    PO_HIPCHK(dp.up(nullptr, sizeof(int32_t) * (size_t)dp_off_h[n]));
    PO_HIPCHK(dpo.up(dp_off_h, sizeof(int64_t) * (n + 1)));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const int rc = po_launch_nw_matrix(sq, so, n, match, mismatch, gap_cost, dp, dpo, st, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(dp.down(dp_h, sizeof(int32_t) * (size_t)dp_off_h[n]));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_align_batch_h(const char* seqs_h, const int64_t* seq_off_h, int n, int band_width, char* aln1_h, char* aln2_h,
                     const int64_t* aln_off_h, int32_t* ncol_h, int32_t* status_h) {
    return po_align_scores_batch_h(seqs_h, seq_off_h, n, band_width, 2, -1, -1, aln1_h, aln2_h, aln_off_h, ncol_h, status_h);
}

int po_envelope_batch_h(const char* aln1_h, const char* aln2_h, const int64_t* aln_off_h, const int32_t* ncol_h, int n,
                        const int32_t* map1_h, const int64_t* map1_off_h, const int32_t* map2_h,
                        const int64_t* map2_off_h, const int32_t* U_h, const int32_t* V_h, int padding, int32_t* env_h,
                        const int64_t* env_off_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    int64_t mc = 0;
    for (int i = 0; i < n; ++i) mc = std::max<int64_t>(mc, ncol_h[i]);
    const size_t tab = sizeof(int64_t) * (n + 1), per = sizeof(int32_t) * n;
    PoDev a1, a2, ao, nc, m1, m1o, m2, m2o, u, v, ev, eo, st, ws;
    PO_HIPCHK(a1.up(aln1_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(a2.up(aln2_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(ao.up(aln_off_h, tab));
    PO_HIPCHK(nc.up(ncol_h, per));
    PO_HIPCHK(m1.up(map1_h, sizeof(int32_t) * (size_t)map1_off_h[n]));
    PO_HIPCHK(m1o.up(map1_off_h, tab));
    PO_HIPCHK(m2.up(map2_h, sizeof(int32_t) * (size_t)map2_off_h[n]));
    PO_HIPCHK(m2o.up(map2_off_h, tab));
    PO_HIPCHK(u.up(U_h, per));
    PO_HIPCHK(v.up(V_h, per));
    PO_HIPCHK(ev.up(nullptr, sizeof(int32_t) * 2 * (size_t)env_off_h[n]));
    PO_HIPCHK(eo.up(env_off_h, tab));
    PO_HIPCHK(st.up(nullptr, per));
    const size_t wsb = po_envelope_workspace_bytes(n, mc);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_envelope_batch(a1, a2, ao, nc, n, m1, m1o, m2, m2o, u, v, padding, ev, eo, st, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(ev.down(env_h, sizeof(int32_t) * 2 * (size_t)env_off_h[n]));
    PO_HIPCHK(st.down(status_h, per));
    return PO_OK;
}

int po_prefix_search_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, char* seq_h,
                             const int64_t* seq_off_h, int32_t* seq_len_h, double* logp_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r(y_off_h, n);
    PoRows y;
    PoSeqOut out;
    PoDev ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(out.up(seq_off_h, n, true));
    const size_t wsb = po_prefix_search_workspace_bytes(n, r.max);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_prefix_search_batch(y.data, y.off, n, C, alphabet, out.seq, out.off, out.len, out.logp, out.status, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h, logp_h));
    return PO_OK;
}

int po_forward_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int model,
                       const char* labels_h, const int64_t* label_off_h, double* logp_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r(y_off_h, n), l(label_off_h, n);
    PoRows y, lb;
    PoDev out, st, ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(lb.up(labels_h, l, 1));
    PO_HIPCHK(out.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_forward_workspace_bytes(n, r.max, model);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_forward_batch(y.data, y.off, n, C, alphabet, model, lb.data, lb.off, out, st, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(logp_h, sizeof(double) * n));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_viterbi_acceptor_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                                int band_size, const char* labels_h, const int64_t* label_off_h, int32_t* path_h,
                                int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r(y_off_h, n), l(label_off_h, n);
    PoRows y, lb;
    PoDev pt, st, ws;
    PO_HIPCHK(y.up(y_h, r, sizeof(double) * C));
    PO_HIPCHK(lb.up(labels_h, l, 1));
    PO_HIPCHK(pt.up(nullptr, sizeof(int32_t) * r.total));
    PO_HIPCHK(st.up(nullptr, sizeof(int32_t) * n));
    const size_t wsb = po_viterbi_acceptor_workspace_bytes(n, r.max, l.max);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_viterbi_acceptor_batch(y.data, y.off, n, C, alphabet, band_size, lb.data, lb.off, pt, st, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(pt.down(path_h, sizeof(int32_t) * r.total));
    PO_HIPCHK(st.down(status_h, sizeof(int32_t) * n));
    return PO_OK;
}

int po_viterbi_acceptor_cy_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                                   int band_size, const char* labels_h, const int64_t* label_off_h, int32_t* path_h,
                                   int32_t* status_h) {
    g_err.clear();
    if (band_size < 0) return po_fail(PO_E_ARG, "po_viterbi_acceptor_cy_batch_h: negative band");
    return po_viterbi_acceptor_batch_h(y_h, y_off_h, n, C, alphabet, -(band_size + 1), labels_h, label_off_h, path_h, status_h);
}

int po_beam2d_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                      const int32_t* env_h, int n, int C, const char* alphabet, int W, int model, int method,
                      char* seq_h,
                      const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r1(y1_off_h, n), r2(y2_off_h, n);
    PoRows a, b;
    PoSeqOut out;
    PoDev ev, ws;
    PO_HIPCHK(a.up(y1_h, r1, sizeof(double) * C));
    PO_HIPCHK(b.up(y2_h, r2, sizeof(double) * C));
    if (env_h) PO_HIPCHK(ev.up(env_h + 2 * r1.base, sizeof(int32_t) * 2 * r1.total));   // one [start, end) per row of read 1
    PO_HIPCHK(out.up(seq_off_h, n));
    // (without an envelope everything but "row" runs the grid method, as in the reference's dispatcher)
    const size_t wsb = po_beam2d_workspace_bytes(n, r1.total, r2.total, r1.max, r2.max, C, W, model,
                                                 (!env_h && method != PO_METHOD_ROW) ? PO_METHOD_GRID_NOENV : method);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc = po_beam2d_batch(a.data, a.off, b.data, b.off, ev, n, C, alphabet, W, model, method, out.seq, out.off, out.len,
                             out.status, ws, wsb, nullptr);
    if (rc != PO_OK) return rc;
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    return PO_OK;
}

// The two pair-decode twins.  from_1d: the caller's 1-D basecalls, lengths and frame maps go up and po_launch_pair_decode_from_1d
// runs; otherwise the basecalls are outputs of po_pair_decode_batch, allocated here and brought down with the rest.
static int pair_decode_h(bool from_1d, const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h, int n,
                  int C, const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h,
                  const int32_t* map1_h, const int32_t* map2_h, double* identity_h, int32_t* env_out_h, char* seq_h,
                  const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h) {
    g_err.clear();
    if (n <= 0) return PO_OK;
    const PoRagged r1(y1_off_h, n), r2(y2_off_h, n);
    const size_t s1b = (size_t)seq1d_off_h[2 * n], per = sizeof(int32_t) * n;
    PoRows a, b;
    PoSeqOut out;
    PoDev s1o, s1, l1, l2, mp1, mp2, idn, ev, ws;
    PO_HIPCHK(a.up(y1_h, r1, sizeof(double) * C));
    PO_HIPCHK(b.up(y2_h, r2, sizeof(double) * C));
    PO_HIPCHK(out.up(seq_off_h, n));
    PO_HIPCHK(s1o.up(seq1d_off_h, sizeof(int64_t) * (2 * n + 1)));
    PO_HIPCHK(s1.up(from_1d ? seq1d_h : nullptr, s1b));
    PO_HIPCHK(l1.up(from_1d ? len1_h : nullptr, per));
    PO_HIPCHK(l2.up(from_1d ? len2_h : nullptr, per));
    if (from_1d) PO_HIPCHK(mp1.up(map1_h + r1.base, sizeof(int32_t) * r1.total));   // one frame per base, at the read's rows
    if (from_1d) PO_HIPCHK(mp2.up(map2_h + r2.base, sizeof(int32_t) * r2.total));
    PO_HIPCHK(idn.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(ev.up(nullptr, sizeof(int32_t) * 2 * r1.total));
    const size_t wsb = po_pair_decode_workspace_bytes(n, r1.total, r2.total, r1.max, r2.max, C, opt);
    PO_HIPCHK(ws.up(nullptr, wsb));
    int rc;
    if (from_1d) {
        rc = po_launch_pair_decode_from_1d(a.data, a.off, b.data, b.off, n, C, opt, r1.total, r2.total, r1.max, r2.max, mp1, mp2,
                                           s1, s1o, l1, l2, idn, ev, out.seq, out.off, out.len, out.status, ws, wsb, nullptr);
        if (rc != PO_OK) return po_fail(rc, "po_pair_decode_from_1d_batch_h: launch refused");
        PO_HIPCHK(hipGetLastError());
    } else {
        rc = po_pair_decode_batch(a.data, a.off, b.data, b.off, n, C, opt, s1, s1o, l1, l2, idn, ev, out.seq, out.off, out.len,
                                  out.status, ws, wsb, nullptr);
        if (rc != PO_OK) return rc;
    }
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    if (!from_1d) {
        PO_HIPCHK(s1.down(seq1d_h, s1b));
        PO_HIPCHK(l1.down(len1_h, per));
        PO_HIPCHK(l2.down(len2_h, per));
    }
    PO_HIPCHK(idn.down(identity_h, sizeof(double) * n));
    PO_HIPCHK(ev.down(env_out_h, sizeof(int32_t) * 2 * r1.total));
    return PO_OK;
}

int po_pair_decode_from_1d_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                                   int n, int C, const po_pair_options* opt, const char* seq1d_h,
                                   const int64_t* seq1d_off_h, const int32_t* len1_h, const int32_t* len2_h,
                                   const int32_t* map1_h, const int32_t* map2_h, double* identity_h, int32_t* env_out_h,
                                   char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h) {
    return pair_decode_h(true, y1_h, y1_off_h, y2_h, y2_off_h, n, C, opt, const_cast<char*>(seq1d_h), seq1d_off_h,
                         const_cast<int32_t*>(len1_h), const_cast<int32_t*>(len2_h), map1_h, map2_h, identity_h, env_out_h, seq_h,
                         seq_off_h, seq_len_h, status_h);
}

int po_pair_decode_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h,
                           const int64_t* y2_off_h, int n, int C, const po_pair_options* opt, char* seq1d_h,
                           const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h, double* identity_h,
                           int32_t* env_out_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h,
                           int32_t* status_h) {
    return pair_decode_h(false, y1_h, y1_off_h, y2_h, y2_off_h, n, C, opt, seq1d_h, seq1d_off_h, len1_h, len2_h, nullptr, nullptr,
                         identity_h, env_out_h, seq_h, seq_off_h, seq_len_h, status_h);
}

// -------------------------------------------------------------------------------- pair decode --skip_matches
namespace {
// total and largest rows of the two reads of a batch whose tables are on the device
struct SkipRows { int64_t t1, t2, m1, m2; };
int skip_rows(const int64_t* y1_off, const int64_t* y2_off, int n, hipStream_t s, SkipRows* r) {
    std::vector<int64_t> h(2 * (size_t)(n + 1));
    PO_HIPCHK(po_read_tables(y1_off, y2_off, n, s, h.data()));
    *r = SkipRows{h[n] - h[0], h[2 * n + 1] - h[n + 1], 0, 0};
    for (int i = 0; i < n; ++i) {
        r->m1 = std::max<int64_t>(r->m1, h[i + 1] - h[i]);
        r->m2 = std::max<int64_t>(r->m2, h[n + 1 + i + 1] - h[n + 1 + i]);
    }
    return PO_OK;
}
}  // namespace

size_t po_pair_skip_plan_workspace_bytes(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, const po_pair_options* opt,
                                         int skip_threshold, int indel_threshold) {
    g_err.clear();
    return po_skip_plan_ws_bytes(n, tr1, tr2, mr1, mr2, C, opt, skip_threshold, indel_threshold);
}

int po_pair_skip_plan(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                      const po_pair_options* opt, int skip_threshold, int indel_threshold, char* seq1d, const int64_t* seq1d_off,
                      int32_t* len1, int32_t* len2, double* identity, int32_t* status, int32_t* n_anchors, int32_t* n_boxes,
                      void* plan_ws, size_t plan_ws_bytes, po_skip_totals* totals, void* stream) {
    g_err.clear();
    if (n < 0 || !y1 || !y1_off || !y2 || !y2_off || !opt || !seq1d || !seq1d_off || !len1 || !len2 || !identity || !status ||
        !n_anchors || !n_boxes || !plan_ws || !totals) return po_fail(PO_E_ARG, "po_pair_skip_plan: null argument");
    if (opt->diagonal_envelope) return po_fail(PO_E_UNSUPPORTED, "po_pair_skip_plan: diagonal_envelope has no alignment to take anchors from");
    if (skip_threshold < 1 || indel_threshold < 1) return po_fail(PO_E_ARG, "po_pair_skip_plan: thresholds must be at least 1");
    *totals = po_skip_totals{0, 0, 0, 0, 0};
    if (n == 0) return PO_OK;
    SkipRows r;
    int rc = skip_rows(y1_off, y2_off, n, (hipStream_t)stream, &r);
    if (rc != PO_OK) return rc;
    rc = po_launch_skip_plan(y1, y1_off, y2, y2_off, n, C, opt, skip_threshold, indel_threshold, r.t1, r.t2, r.m1, r.m2, seq1d, seq1d_off,
                             len1, len2, identity, status, n_anchors, n_boxes, plan_ws, plan_ws_bytes, totals, (hipStream_t)stream);
    if (rc != PO_OK) return po_fail(rc, "po_pair_skip_plan: launch refused (options, or workspace too small)");
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

size_t po_pair_skip_run_workspace_bytes(int n, int C, const po_pair_options* opt, const po_skip_totals* totals) {
    g_err.clear();
    return po_skip_run_ws_bytes(n, C, opt, totals);
}

int po_pair_skip_run(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                     const po_pair_options* opt, int skip_threshold, int indel_threshold, const po_skip_totals* totals, void* plan_ws,
                     size_t plan_ws_bytes, char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* run_ws,
                     size_t run_ws_bytes, void* stream) {
    g_err.clear();
    if (n < 0 || !y1 || !y1_off || !y2 || !y2_off || !opt || !totals || !plan_ws || !seq || !seq_off || !seq_len || !status || !run_ws)
        return po_fail(PO_E_ARG, "po_pair_skip_run: null argument");
    if (n == 0) return PO_OK;
    SkipRows r;
    int rc = skip_rows(y1_off, y2_off, n, (hipStream_t)stream, &r);
    if (rc != PO_OK) return rc;
    rc = po_launch_skip_run(y1, y1_off, y2, y2_off, n, C, opt, skip_threshold, indel_threshold, r.t1, r.t2, r.m1, r.m2, totals, plan_ws,
                            plan_ws_bytes, seq, seq_off, seq_len, status, run_ws, run_ws_bytes, nullptr, (hipStream_t)stream);
    if (rc != PO_OK) return po_fail(rc, "po_pair_skip_run: launch refused (options, totals, or a workspace too small)");
    PO_HIPCHK(hipGetLastError());
    return PO_OK;
}

int po_pair_skip_decode_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h, int n, int C,
                                const po_pair_options* opt, int skip_threshold, int indel_threshold, char* seq1d_h,
                                const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h, double* identity_h, int32_t* env_out_h,
                                char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h, int32_t* n_anchors_h,
                                int32_t* n_boxes_h, int64_t* tab_rows_h, int32_t* anchors_h, int32_t* boxes_h, po_skip_totals* totals_h,
                                float* stage_ms_h) {
    g_err.clear();
    if (!opt || !n_anchors_h || !n_boxes_h) return po_fail(PO_E_ARG, "po_pair_skip_decode_batch_h: null argument");
    if (opt->diagonal_envelope) return po_fail(PO_E_UNSUPPORTED, "po_pair_skip_decode_batch_h: diagonal_envelope has no alignment to take anchors from");
    if (skip_threshold < 1 || indel_threshold < 1) return po_fail(PO_E_ARG, "po_pair_skip_decode_batch_h: thresholds must be at least 1");
    if (n <= 0) return PO_OK;
    const PoRagged r1(y1_off_h, n), r2(y2_off_h, n);
    const size_t s1b = (size_t)seq1d_off_h[2 * n], per = sizeof(int32_t) * n;
    PoRows a, b;
    PoSeqOut out;
    PoDev s1o, s1, l1, l2, idn, na, nb, pws, rws;
    PO_HIPCHK(a.up(y1_h, r1, sizeof(double) * C));
    PO_HIPCHK(b.up(y2_h, r2, sizeof(double) * C));
    PO_HIPCHK(out.up(seq_off_h, n));
    PO_HIPCHK(s1o.up(seq1d_off_h, sizeof(int64_t) * (2 * n + 1)));
    PO_HIPCHK(s1.up(nullptr, s1b));
    PO_HIPCHK(l1.up(nullptr, per));
    PO_HIPCHK(l2.up(nullptr, per));
    PO_HIPCHK(idn.up(nullptr, sizeof(double) * n));
    PO_HIPCHK(na.up(nullptr, per));
    PO_HIPCHK(nb.up(nullptr, per));
    const size_t pwsb = po_skip_plan_ws_bytes(n, r1.total, r2.total, r1.max, r2.max, C, opt, skip_threshold, indel_threshold);
    if (pwsb == 0) return po_fail(PO_E_ARG, "po_pair_skip_decode_batch_h: model and column count do not fit");
    PO_HIPCHK(pws.up(nullptr, pwsb));
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 5; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
    if (stage_ms_h) {
        for (int i = 0; i < 5; ++i) PO_HIPCHK(hipEventCreate(&ev[i]));
        PO_HIPCHK(hipEventRecord(ev[4], nullptr));
    }
    po_skip_totals tot;
    int rc = po_launch_skip_plan(a.data, a.off, b.data, b.off, n, C, opt, skip_threshold, indel_threshold, r1.total, r2.total, r1.max, r2.max,
                                 s1, s1o, l1, l2, idn, out.status, na, nb, pws, pwsb, &tot, nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_pair_skip_decode_batch_h: plan refused");
    PO_HIPCHK(hipGetLastError());
    const size_t rwsb = po_skip_run_ws_bytes(n, C, opt, &tot);
    PO_HIPCHK(rws.up(nullptr, rwsb));
    rc = po_launch_skip_run(a.data, a.off, b.data, b.off, n, C, opt, skip_threshold, indel_threshold, r1.total, r2.total, r1.max, r2.max, &tot,
                            pws, pwsb, out.seq, out.off, out.len, out.status, rws, rwsb, stage_ms_h ? ev : nullptr, nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_pair_skip_decode_batch_h: run refused");
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(hipGetLastError());
    if (stage_ms_h) {
        PO_HIPCHK(hipEventElapsedTime(&stage_ms_h[0], ev[4], ev[0]));
        for (int k = 0; k < 3; ++k) PO_HIPCHK(hipEventElapsedTime(&stage_ms_h[1 + k], ev[k], ev[k + 1]));
    }
    PO_HIPCHK(out.down(seq_h, seq_len_h, status_h));
    PO_HIPCHK(s1.down(seq1d_h, s1b));
    PO_HIPCHK(l1.down(len1_h, per));
    PO_HIPCHK(l2.down(len2_h, per));
    PO_HIPCHK(idn.down(identity_h, sizeof(double) * n));
    PO_HIPCHK(na.down(n_anchors_h, per));
    PO_HIPCHK(nb.down(n_boxes_h, per));
    const int32_t *anc = nullptr, *box = nullptr, *env = nullptr;
    int64_t rows = 0;
    rc = po_skip_plan_tables(pws, n, r1.total, r2.total, r1.max, r2.max, C, opt, skip_threshold, indel_threshold, &anc, &box, &env, &rows);
    if (rc != PO_OK) return po_fail(rc, "po_pair_skip_decode_batch_h: tables");
    if (env_out_h) PO_HIPCHK(hipMemcpy(env_out_h, env, sizeof(int32_t) * 2 * (size_t)r1.total, hipMemcpyDeviceToHost));
    if (anchors_h) PO_HIPCHK(hipMemcpy(anchors_h, anc, sizeof(int32_t) * 4 * (size_t)rows, hipMemcpyDeviceToHost));
    if (boxes_h) PO_HIPCHK(hipMemcpy(boxes_h, box, sizeof(int32_t) * 4 * (size_t)(rows + n), hipMemcpyDeviceToHost));
    if (tab_rows_h)
        for (int i = 0; i <= n; ++i) tab_rows_h[i] = (r1.off[i] + r2.off[i] + 16ll * i) / std::min(skip_threshold, indel_threshold) + i;
    if (totals_h) *totals_h = tot;
    return PO_OK;
}

int po_skip_boxes_batch_h(const char* aln1_h, const char* aln2_h, const int64_t* aln_off_h, const int32_t* ncol_h, int n,
                          const int32_t* map1_h, const int64_t* map1_off_h, const int32_t* map2_h, const int64_t* map2_off_h,
                          const int32_t* U_h, const int32_t* V_h, const int32_t* env_h, const int64_t* env_off_h, int skip_threshold,
                          int indel_threshold, int32_t* n_anchors_h, int32_t* n_boxes_h, int64_t* tab_rows_h, int32_t* anchors_h,
                          int32_t* boxes_h, int32_t* status_h) {
    g_err.clear();
    if (skip_threshold < 1 || indel_threshold < 1) return po_fail(PO_E_ARG, "po_skip_boxes_batch_h: thresholds must be at least 1");
    if (n <= 0) return PO_OK;
    const int m = std::min(skip_threshold, indel_threshold);
    for (int i = 0; i < n; ++i) {
        if (aln_off_h[i + 1] < aln_off_h[i] || map1_off_h[i + 1] < map1_off_h[i] || map2_off_h[i + 1] < map2_off_h[i] ||
            env_off_h[i + 1] - env_off_h[i] < U_h[i] || U_h[i] < 0)
            return po_fail(PO_E_ARG, "po_skip_boxes_batch_h: pair " + std::to_string(i) + ": a table decreases, or fewer envelope rows than frames");
    }
    const size_t tab = sizeof(int64_t) * (n + 1), per = sizeof(int32_t) * n;
    const int64_t rows = (aln_off_h[n] - aln_off_h[0]) / m + n;
    PoDev a1, a2, ao, nc, m1, m1o, m2, m2o, u, v, ev, eo, st, na, nb, anc, box, pinfo;
    PO_HIPCHK(a1.up(aln1_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(a2.up(aln2_h, (size_t)aln_off_h[n]));
    PO_HIPCHK(ao.up(aln_off_h, tab));
    PO_HIPCHK(nc.up(ncol_h, per));
    PO_HIPCHK(m1.up(map1_h, sizeof(int32_t) * (size_t)map1_off_h[n]));
    PO_HIPCHK(m1o.up(map1_off_h, tab));
    PO_HIPCHK(m2.up(map2_h, sizeof(int32_t) * (size_t)map2_off_h[n]));
    PO_HIPCHK(m2o.up(map2_off_h, tab));
    PO_HIPCHK(u.up(U_h, per));
    PO_HIPCHK(v.up(V_h, per));
    PO_HIPCHK(ev.up(env_h, sizeof(int32_t) * 2 * (size_t)env_off_h[n]));
    PO_HIPCHK(eo.up(env_off_h, tab));
    PO_HIPCHK(st.up(nullptr, per));
    PO_HIPCHK(hipMemset(st.p, 0, per));
    PO_HIPCHK(na.up(nullptr, per));
    PO_HIPCHK(nb.up(nullptr, per));
    PO_HIPCHK(anc.up(nullptr, sizeof(int32_t) * 4 * (size_t)(rows + 1)));
    PO_HIPCHK(box.up(nullptr, sizeof(int32_t) * 4 * (size_t)(rows + n + 1)));
    PO_HIPCHK(pinfo.up(nullptr, sizeof(long long) * 6 * (size_t)n));
    int rc = po_launch_skip_boxes(a1, a2, ao, nc, n, m1, m1o, m2, m2o, u, v, ev, eo, skip_threshold, indel_threshold, na, nb, anc, box, st,
                                  pinfo.as<long long>(), nullptr);
    if (rc != PO_OK) return po_fail(rc, "po_skip_boxes_batch_h: launch refused");
    PO_HIPCHK(hipDeviceSynchronize());
    PO_HIPCHK(na.down(n_anchors_h, per));
    PO_HIPCHK(nb.down(n_boxes_h, per));
    PO_HIPCHK(anc.down(anchors_h, sizeof(int32_t) * 4 * (size_t)rows));
    PO_HIPCHK(box.down(boxes_h, sizeof(int32_t) * 4 * (size_t)(rows + n)));
    PO_HIPCHK(st.down(status_h, per));
    if (tab_rows_h)
        for (int i = 0; i <= n; ++i) tab_rows_h[i] = (aln_off_h[i] - aln_off_h[0]) / m + i;
    return PO_OK;
}

// -------------------------------------------------------------------------------- events / profile
void* po_event_create(void) {
    hipEvent_t e;
    return hipEventCreate(&e) == hipSuccess ? (void*)e : nullptr;
}
int po_event_record(void* ev, void* stream) {
    g_err.clear();
    PO_HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return PO_OK;
}
int po_event_elapsed_ms(void* start, void* stop, float* ms) {
    g_err.clear();
    PO_HIPCHK(hipEventSynchronize((hipEvent_t)stop));
    PO_HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return PO_OK;
}
void po_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }

int po_profile_update_counter(uint64_t* device_counter) {
    g_err.clear();
    po_b2_set_update_counter((unsigned long long*)device_counter);
    return PO_OK;
}
int po_lae_peak(int iters, double* lae_per_s, void* stream) {
    g_err.clear();
    if (iters < 1 || !lae_per_s) { g_err = "po_lae_peak: bad argument"; return PO_E_ARG; }
    int rc = po_launch_lae_peak(iters, lae_per_s, (hipStream_t)stream);
    if (rc != PO_OK) g_err = "po_lae_peak: launch failed";
    return rc;
}
void po_profile_enable(int on) {
    g_prof_on = on != 0;
    po_b2_set_mark(g_prof_on ? b2_mark : nullptr);
}
void po_profile_reset(void) {
    prof_drain();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    std::memset(g_prof_ms, 0, sizeof(g_prof_ms));
    std::memset(g_prof_n, 0, sizeof(g_prof_n));
}
int po_profile_get(int kernel, double* total_ms, int64_t* launches) {
    g_err.clear();
    if (kernel < 0 || kernel >= PO_K_COUNT) return PO_E_ARG;
    prof_drain();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (total_ms) *total_ms = g_prof_ms[kernel];
    if (launches) *launches = g_prof_n[kernel];
    return PO_OK;
}
// internal: lets the pair pipeline time its own stages under their kernel ids
void po_prof_stage(int kernel, hipStream_t s, int begin, void** tok) {
    if (!g_prof_on) return;
    if (begin) {
        auto* r = new ProfRec{nullptr, nullptr, kernel};
        (void)hipEventCreate(&r->a);
        (void)hipEventCreate(&r->b);
        (void)hipEventRecord(r->a, s);
        *tok = r;
    } else if (*tok) {
        auto* r = (ProfRec*)*tok;
        (void)hipEventRecord(r->b, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back(*r);
        delete r;
        *tok = nullptr;
    }
}

}  // extern "C"
