/* poreover_hip.h — C-ABI of libporeover_hip.so, the MI355X (gfx950) decoding engine.
 *
 * This is the drop-in boundary for PoreOver's native decode path.  In the reference the
 * boundary is the set of Python-callable functions that Cython exports from
 * poreover/decoding/decoding_cpp.pyx, poreover/decoding/decoding_cy.pyx and
 * poreover/align/align.pyx; each entry point below names the reference interface it
 * replaces.  The reference decodes ONE read / pair per call and gets its parallelism from
 * multiprocessing.Pool (decode.py:158-162, pair_decode.py:292-297); here every entry point is
 * BATCHED — one launch decodes n independent reads / pairs — which is the natural shape for a
 * GPU.  The single-item Python wrappers with the reference's exact signatures
 * (poreover_amd/decoding/decoding_cpp.py) call these with n == 1.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless the name ends in _h
 *   - the device-pointer calls enqueue their kernels on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and return without waiting for them; scratch comes from `ws`, and none allocates or frees device memory —
 *     except that the first pair beam search (method row_col with an envelope, W <= 12) of a process on a device creates,
 *     per tree model, a pool of value-store slices that the library keeps (5.3 GB for the default model).
 *     The calls whose geometry depends on batch maxima they are not given (po_pair_decode_batch, po_beam2d_batch,
 *     po_beam1d_batch, the lattice / alignment calls) first read the offset tables back (one small D2H copy and a
 *     stream synchronise) — enqueue the inputs before calling; po_viterbi_batch (CTC kinds) and po_ingest_batch do
 *     not.  The *_h forms and po_pipeline_pair_decode are synchronous.
 *   - a workspace may be reused from call to call and its contents need not be preserved (beam2d_kernel keeps
 *     per-workgroup epoch counters in it and clears what it finds untagged: first use)
 *   - po_last_error() is per host thread and refers to the last failing call of that thread; the profiling aid at
 *     the end of this header (po_profile_*) is process-wide and meant for one measuring thread
 *   - y:       concatenated C-contiguous (T_i, C) float64 natural-log probabilities
 *     y_off:   int64[n+1] ROW offsets into y (read i owns rows [y_off[i], y_off[i+1]))
 *   - env:     concatenated (U_i, 2) int32 half-open column ranges, row-aligned with y1
 *   - seq:     output characters; read/pair i writes at seq + seq_off[i], at most
 *              seq_off[i+1]-seq_off[i] bytes (no terminator); seq_len[i] gets the length
 *   - status:  int32[n], 0 on success or a PO_E_* code for that item (the launch itself
 *              returns 0 unless the arguments are unusable)
 *   - model:   PO_MODEL_CTC ('ctc'), PO_MODEL_MERGE ('ctc_merge_repeats'),
 *              PO_MODEL_FLIPFLOP ('ctc_flipflop')       (decode.py:172, pair_decode.py:147)
 *   - alphabet: HOST string of A <= 4 symbols (the reference's alphabet_ argument, default
 *              "ACGT"); C == A + 1 for the CTC models (blank last), C == 2A for flip-flop
 */
#ifndef POREOVER_HIP_H
#define POREOVER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PO_MODEL_CTC 0
#define PO_MODEL_MERGE 1
#define PO_MODEL_FLIPFLOP 2

#define PO_METHOD_ROW 0
#define PO_METHOD_ROW_COL 1
#define PO_METHOD_GRID 2
#define PO_METHOD_GRID_NOENV 3 /* po_beam2d_workspace_bytes only: grid without an envelope (env == NULL, method != row) */

#define PO_KIND_POREOVER 0
#define PO_KIND_BONITO 1
#define PO_KIND_FLIPFLOP 2

#define PO_OK 0
#define PO_E_CAP (-1)        /* an output or workspace buffer is too small                    */
#define PO_E_ARG (-2)        /* unusable argument                                             */
#define PO_E_ENVELOPE (-3)   /* envelope on which the reference itself is undefined           */
#define PO_E_NOMEM (-4)      /* per-item node arena / band capacity exceeded                  */
#define PO_E_DIVERGE (-5)    /* input on which the reference never terminates                 */
#define PO_E_UNSUPPORTED (-6)/* valid for the reference, not yet handled by this engine       */
#define PO_E_HIP (-7)        /* HIP runtime error (see po_last_error)                         */
#define PO_SKIP_LENGTH (-10) /* pair skipped: |len1 - len2| > 1000   (pair_decode.py:372-375) */
#define PO_SKIP_IDENTITY (-11)/* pair skipped: identity < 0.5        (pair_decode.py:395-398) */
#define PO_E_NO_ANCHOR (-12) /* --skip_matches: no run of matches / indels long enough (the reference's assert) */
#define PO_E_BOX (-13)       /* --skip_matches: a box the reference raises IndexError on (empty, or past a basecall's end) */

/* ---- library / device ----------------------------------------------------------------- */
int po_version(void);
int po_device_count(void);
int po_set_device(int device);
const char* po_last_error(void);
/* name, compute units and clock of `device`; returns 0 on success */
int po_device_info(int device, char* name, int name_cap, int* compute_units, int* clock_khz,
                   size_t* total_mem);

/* test / tuning hook: which kernel serves the pair beam search.  PO_ROUTE_AUTO = the engine's choice (DESIGN.md §3.3:
 * beam2d_reg_kernel for row_col with an envelope, every tree model, W <= 12; beam2d_kernel elsewhere); PO_ROUTE_REG = the
 * same, named; PO_ROUTE_LEGACY = always beam2d_kernel; defer_odd != 0: the register-state kernel hands every odd pair to
 * beam2d_kernel (exercises the hand-over).  Process-wide; results are identical on every route.
 * (Values 1 and 3 named the two-pairs-per-wave and LDS-ring kernels of rounds 1 - 4, retired in round 5: PO_E_ARG.) */
#define PO_ROUTE_AUTO 0
#define PO_ROUTE_LEGACY 2
#define PO_ROUTE_REG 4   /* beam2d_reg_kernel: element state in registers, values in the (tag-free) HBM store */
/* defer_odd bits 1 and 2 (values 2, 4) are further test hooks of that hand-over: the kernel runs with a dozen row groups /
 * with a tree arena of a few nodes, so that pairs run out of them and are handed on (tests/test_gpu_parity_2d.py). */
int po_set_pair_route(int route, int defer_odd);
/* How the register-state pair kernel computes the window of a NEW element (the children of a node that entered the beam:
 * BeamSearch.h:342-375 -> update_prob over the whole window, PrefixTree.h:518-531).
 *   PO_CHAIN_SERIAL (default): the reference's serial logaddexp chain, operation for operation.
 *   PO_CHAIN_CLOSED_FORM: x_t = B_t + log(sum_{s<=t} exp(p_{s-1} + y_s - B_s)), B = running sum of the stay (blank) column —
 *        one exp per (element, time), a prefix sum in the probability domain, one log; time-parallel (8 lanes per chain).
 *        The VALUES differ from the serial chain's by ~ 1e-12 (they are closer to the exact value than the chain's:
 *        scripts/check_chain_scan.cpp); decoded strings are held to north_star's tolerance (<= 0.1 % edit distance; measured:
 *        0 differing pairs of the bench's 10 000 and of the parity suite).  A chain whose finite terms span more than 600 nats
 *        sends its step to the kernel's general scan (the serial chain).  Round 6 built it as the one remaining lever on the
 *        headline — and measured it SLOWER than the serial chain (65 vs 52 ms per 10 000 pairs: profiles/r06_ab_chain_scan.txt,
 *        DESIGN.md 3.3 says why), so it is opt-in (also: environment variable PO_CHAIN_CLOSED as the initial value).
 *   PO_CHAIN_CLOSED_GUARD3: test hook — the closed form with its 600-nat guard at 3 nats, so that most steps take the hand-over.
 * Applies to the one-value tree model (ctc) on the register-state route.  Process-wide. */
#define PO_CHAIN_SERIAL 0
#define PO_CHAIN_CLOSED_FORM 1
#define PO_CHAIN_CLOSED_GUARD3 2
int po_set_chain_mode(int mode);
int po_get_chain_mode(void);
/* The register-state pair kernel has one instantiation compiled for the default shape — the ctc model, beam_width 5, four
 * bases (A = 4, C = 5) — with the three numbers as compile-time constants: the same arithmetic in the same
 * order, fewer vector instructions per pair.  on != 0 (default): launches of that shape take it; on == 0: they run the
 * run-time kernel every other shape runs — for the tests, which compare the two, and for A/B timing from one library.
 * The environment variable PO_REG_FIXED_SHAPE=0 gives the initial value "off".  Process-wide; results are identical. */
int po_set_reg_fixed_shape(int on);
int po_get_reg_fixed_shape(void);
/* The register-state pair kernel keeps its value stores and tree arenas in a slice POOL the library owns: one per device, tree
 * model and lane layout (beam_width <= 6 / 7..12), as many slices as the device holds pair waves (<ctc, W <= 6>: 4 096 x 1.28 MB
 * = 5.3 GB), made by the first workspace-size query that selects the route and kept for the life of the process.
 * po_reg_pool_prewarm makes the pool of (model, beam_width) on the current device ahead of time (PO_E_NOMEM if it cannot be
 * allocated: beam2d_kernel then serves the route, with results identical); po_reg_pool_release waits for the device and frees
 * every pool of the current device — a long-lived process that has used several models and widths holds tens of GB otherwise. */
int po_reg_pool_prewarm(int model, int beam_width);
int po_reg_pool_release(void);
/* test hook: pairs the register-state kernel or its pre-pass handed to beam2d_kernel on the current device since the last
 * reset (windows beyond its store geometry or its packed walk records, row groups or arena exhausted, non-monotone envelopes,
 * the defer_odd hooks); reset != 0 clears the count.  Synchronises the device; -1 on a HIP error. */
long long po_debug_deferred_pairs(int reset);
/* test / tuning hook: legacy != 0 -> the banded aligner (align.pyx:100-178) runs the row-at-a-time kernel that stores the
 * score table instead of the skewed-wavefront kernel.  Process-wide; results are identical. */
int po_set_align_route(int legacy);

/* test hooks of the lattice's routing.  po_qual_batch_route is po_qual_batch (below: its arguments, refusals
 * and results) with the choice of lattice kernel as a last argument:
 *   PO_QUAL_ROUTE_GENERAL  qual_kernel by its four launch classes: what po_qual_batch launches
 *   PO_QUAL_ROUTE_AUTO     what po_fastq_tables and po_pair_qual pass by default.  Today the same as GENERAL: neither
 *                          instantiation of qual_reg_kernel is on the automatic route
 *   PO_QUAL_ROUTE_REG      the reads whose ring holds at most 64 indices (a band of 1 to 31, or no band and at most 63
 *                          labels) on qual_reg_kernel, the rest as before: for the tests and scripts/bench_tensors_fastq.py
 * The workspace is po_qual_workspace_bytes' on every route, and so are the bits of odds, logp and status.
 * po_set_qual_route: the route that po_fastq_tables and po_pair_qual pass from now on, process-wide (any other value: PO_E_ARG).
 * po_debug_qual_reg_reads: the reads that were launched on qual_reg_kernel since the last reset (reset != 0 clears the count);
 * counted on the host at the launch, no synchronise. */
#define PO_QUAL_ROUTE_GENERAL 0
#define PO_QUAL_ROUTE_AUTO 1
#define PO_QUAL_ROUTE_REG 2
int po_set_qual_route(int route);
long long po_debug_qual_reg_reads(int reset);
int po_qual_batch_route(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int model, const char* labels,
                        const int64_t* label_off, const int32_t* guide, int band_size, double* odds, double* logp,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream, int route);

/* ---- trace ingest ------------------------------------------------------------------------------
 * replaces decode.logit_to_log_likelihood (decode.py:34-39), the uint8 trace scaling of
 * model_from_trace (decode.py:89-93,99-103), the Bonito column order (decode.py:79) and
 * transducer.reverse_complement (transducer.py:68-70,104-106) — one streaming pass on the device.
 *   mode PO_INGEST_LOGITS_F32: src float32 (rows, C) logits -> x - logsumexp(x), in float32 like the
 *        reference, widened to float64;  PO_INGEST_TRACE_U8: src uint8 -> log((x+1e-7)/(255+1e-7));
 *        PO_INGEST_F64: src float64, copied.   perm (host, C ints or NULL): out[:, c] = value[:, perm[c]].
 *   reverse != 0: every item [row_off[i], row_off[i+1]) is time-reversed.   out: float64 (rows, C). */
#define PO_INGEST_LOGITS_F32 0
#define PO_INGEST_TRACE_U8 1
#define PO_INGEST_F64 2
int po_ingest_batch(const void* src, const int64_t* row_off, int n, int C, int mode, const int* perm_h,
                    int reverse, double* out, void* stream);

/* ---- ingest of a model's output as it lies in memory (poreover_amd/tensors.py) ---------------------------
 * Item i is a (T_i, C) view of `dtype` elements: element (t, c) at base + (t * row_stride + c * col_stride) * sizeof(dtype),
 * T_i = row_off[i+1] - row_off[i].  A padded batch in either layout, a slice, a transposed or an expanded view (stride 0) are
 * all item tables.  out[(row_off[i] + t) * C + c] = v[perm[c]] of source row t (reverse != 0: of row T_i - 1 - t), where v is
 *   normalize != 0, F32 / F16 / BF16: the row widened to float32 (exact), x - logsumexp(x) in float32, widened: the bits of
 *                  po_ingest_batch(PO_INGEST_LOGITS_F32) on the widened rows;   F64: PO_E_UNSUPPORTED
 *   normalize == 0: the values widened to double (F64: the bits of PO_INGEST_F64).
 * items and row_off are DEVICE arrays (n and n + 1 entries); total_rows = row_off[n] (row_off[0] == 0), given by the caller,
 * so that the call is enqueue-only: no allocation, no synchronisation, no read of device memory by the host.
 * Two kernels give the same bits.  The default takes one frame per lane, consecutive lanes along `out`: right where an item's
 * rows are adjacent in the source (batch-major).  PO_INGEST_TILED or-ed into dtype selects the tiled kernel: a workgroup takes
 * 32 consecutive items x 16 time steps and reads with lanes running along the ITEMS, for sources whose items interleave
 * (time-major, (T, N, C): item i + 1 starts C elements after item i), and writes through LDS along out's rows.  The caller
 * knows its strides; the host twin below looks at them itself (PO_INGEST_PER_FRAME or-ed in keeps it from choosing).
 * PO_E_ARG before any launch: n < 0 or total_rows < 0, C outside 1..8, an unknown dtype, a perm entry outside [0, C), null
 * items / row_off / out with total_rows > 0.  n == 0 or total_rows == 0: PO_OK, nothing launched. */
typedef struct { const void* base; int64_t row_stride; int64_t col_stride; } po_ingest_item;  /* strides in ELEMENTS, >= 0 */
#define PO_DTYPE_F32 0
#define PO_DTYPE_F16 1
#define PO_DTYPE_BF16 2
#define PO_DTYPE_F64 3
#define PO_INGEST_TILED 0x100
#define PO_INGEST_PER_FRAME 0x200
int po_ingest_strided(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, int normalize,
                      const int* perm_h, int reverse, int64_t total_rows, double* out, void* stream);
/* host twin: src_h is one host block of src_elems elements; item i's element (0, 0) is element item_off_h[i] of it, its strides
 * row_stride_h[i] / col_stride_h[i].  Also PO_E_ARG: row_off_h[0] != 0 or decreasing, a negative offset or stride, an item that
 * reaches past src_elems. */
int po_ingest_strided_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                        const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, int normalize,
                        const int* perm_h, int reverse, double* out_h);

/* ---- compaction of a decode's strings -----------------------------------------------------------------------------------
 * The decoders write string i at seq + seq_off[i] in a buffer sized for the longest possible answer.  po_pack_strings puts the
 * strings back to back: packed_off (device, n + 1) = exclusive scan of (status[i] == 0 ? seq_len[i] : 0) (status NULL: every
 * length counts; a length is taken as at least 0 and at most the string's room seq_off[i+1] - seq_off[i], so `packed` never
 * needs more than seq's own size), packed + packed_off[i] = the string.  Enqueue-only.  The 1-D basecalls of a pair decode have
 * no status of their own: status NULL, n = 2 * pairs.  PO_E_ARG: n < 0, a null seq / seq_off / seq_len / packed with n > 0, a
 * null packed_off; PO_E_CAP: ws_bytes < po_pack_strings_workspace_bytes(n). */
size_t po_pack_strings_workspace_bytes(int n);
int po_pack_strings(const char* seq, const int64_t* seq_off, const int32_t* seq_len, const int32_t* status, int n,
                    char* packed, int64_t* packed_off, void* ws, size_t ws_bytes, void* stream);
/* host twin: packed_h has room for seq_off_h[n] - seq_off_h[0] bytes (what is past packed_off_h[n] is left alone) */
int po_pack_strings_h(const char* seq_h, const int64_t* seq_off_h, const int32_t* seq_len_h, const int32_t* status_h, int n,
                      char* packed_h, int64_t* packed_off_h);

/* ---- CTC loss and gradient on tensors where they lie (po_ctc.hip) ------------------------------------------
 * Item i: logits x [T_i][C] at items[i] (po_ingest_strided's table and dtypes; f64 with normalize = 0 only), rows
 * row_off[i] .. row_off[i+1]; labels int32 [L_i] at labels + label_off[i], values 0 .. C-2 (the alphabet's order; blank is
 * canonical column C-1).  perm_h (host, or NULL): canonical column c is source column perm_h[c], a permutation.
 * lp = log_softmax(x) per frame in float64 (normalize = 0: x holds log-probabilities, widened as they are).
 *   loss[i]    = -log P(l_i | lp) over 2L+1 states; PO_MODEL_CTC: label states do not loop and every blank may be skipped;
 *                PO_MODEL_MERGE: standard CTC.  First frame in state 0 or 1, last frame in one of the last two states.
 *   grad[t][c] = softmax(x[t])[c] - sum_{s: label(s) = c} exp(alpha_t(s) + beta_t(s) - log Z)   (normalize = 0: -occupancy),
 *                written through grad_items (a second item table, grad_dtype f32 / f16 / bf16, column perm_h[c]).
 *                grad_items NULL: loss only, no backward pass.
 *   status[i]  (or NULL): 0; PO_E_ENVELOPE: no path (L > T; merge: L + adjacent equal labels > T): loss +inf, gradient rows
 *                zero; PO_E_ARG: a label outside [0, C-2] or offsets that decrease: loss NaN; PO_E_UNSUPPORTED / PO_E_CAP: an
 *                item whose label is longer than PO_CTC_MAX_LABEL / than max_states admits: loss NaN.  T = 0 with L = 0: 0.
 * The caller passes total_rows = row_off[n], total_states = sum T_i * (2 L_i + 1) (read with a gradient only) and
 * max_states = max 2 L_i + 1.  Enqueue-only on `stream`: the entry reads no device memory and does not synchronise.
 * Before any launch: PO_E_UNSUPPORTED for PO_MODEL_FLIPFLOP, f64 with normalize, max_states > 2 * PO_CTC_MAX_LABEL + 1 (the
 * lattice rows are kept in LDS); PO_E_ARG for C outside 2..8, negative sizes, an unknown dtype, a perm that is no
 * permutation, null pointers with n > 0, ws_bytes < po_ctc_loss_workspace_bytes(...).  n == 0: PO_OK. */
#define PO_CTC_MAX_LABEL 1200
size_t po_ctc_loss_workspace_bytes(int n, int64_t total_rows, int64_t total_states, int C, int with_grad);
int po_ctc_loss(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, int normalize, const int* perm_h,
                const int32_t* labels, const int64_t* label_off, int model, int64_t total_rows, int64_t total_states,
                int max_states, float* loss, int32_t* status, const po_ingest_item* grad_items, int grad_dtype, void* ws,
                size_t ws_bytes, void* stream);
/* host twin: the source as po_ingest_strided_h takes it; grad_h (or NULL): row_off_h[n] dense rows of C values of grad_dtype,
 * in the source's column order */
int po_ctc_loss_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                  const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, int normalize,
                  const int* perm_h, const int32_t* labels_h, const int64_t* label_off_h, int model, float* loss_h,
                  int32_t* status_h, void* grad_h, int grad_dtype);

/* ---- CTC forced alignment on tensors where they lie (po_falign.hip) ----------------------------------------
 * Where in time a known sequence sits: the best path of po_ctc_loss's lattice.  Items, dtypes, normalize, perm_h, labels and
 * model are po_ctc_loss's (f64 with normalize = 0 only; blank is canonical column C-1); lp = log_softmax(x) per frame in
 * float64.  States 0 .. 2L (even: blank, odd 2k+1: symbol k); V_0(s) = lp[0][col(s)] for s < 2, -inf otherwise;
 * V_t(s) = max over the admitted predecessors {s, s-1, s-2} of V_{t-1} + lp[t][col(s)], float64, one addition per frame in
 * frame order.  TIES GO TO THE LARGER PREDECESSOR STATE (stay before step before skip), and to state 2L over 2L-1 at the end:
 * the outputs are a function of the input alone and a numpy restatement gives the same bits.
 *   score[i]   = max(V_{T-1}(2L), V_{T-1}(2L-1)), float64
 *   states     (or NULL) int32, row i at states + i * states_stride: the best path's state in frames t < T_i, -1 in frames
 *              T_i <= t < states_stride (written here: the caller may pass uninitialised memory)
 *   starts, stops (or NULL) int32 [total labels] at label_off[i]: the first frame of symbol k's label state and one past its
 *              last (PO_MODEL_CTC: stops = starts + 1)
 *   status[i]  (or NULL): 0; PO_E_ENVELOPE: no path of finite score (L > T; merge: L + adjacent equal labels > T; or the best
 *              score is -inf): score -inf, path outputs -1; PO_E_ARG: a label outside [0, C-2] or offsets that decrease: score
 *              NaN, path outputs -1; PO_E_UNSUPPORTED / PO_E_CAP: a label longer than PO_CTC_MAX_LABEL / than max_states
 *              admits, an item with more frames than states_stride, or bit rows that do not fit total_words: score NaN, path
 *              outputs -1.  T = 0 with L = 0: score 0, status 0.  The entry is not told how many values starts and stops hold:
 *              label_off is the caller's word for that, and an item whose label_off entries decrease or span more than
 *              PO_CTC_MAX_LABEL symbols has its states row set to -1 and its starts / stops left untouched.
 * The caller passes total_rows = row_off[n], total_words = sum T_i * ceil((2 L_i + 1) / 64) (the trace-back keeps two bits
 * per cell, 16 bytes per 64 states of a frame) and max_states = max 2 L_i + 1.  Enqueue-only on `stream`: the entry reads no
 * device memory and does not synchronise.
 * Before any launch: PO_E_UNSUPPORTED for PO_MODEL_FLIPFLOP, f64 with normalize, max_states > 2 * PO_CTC_MAX_LABEL + 1 (the
 * lattice rows are kept in LDS); PO_E_ARG for C outside 2..8, negative sizes, an unknown dtype, a perm that is no
 * permutation, null pointers with n > 0, states with a states_stride that cannot hold the longest item (it has
 * ceil(total_rows / n) frames at least), ws_bytes < po_forced_align_workspace_bytes(...).  n == 0: PO_OK. */
size_t po_forced_align_workspace_bytes(int n, int64_t total_rows, int64_t total_words, int C);
int po_forced_align(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, int normalize,
                    const int* perm_h, const int32_t* labels, const int64_t* label_off, int model, int64_t total_rows,
                    int64_t total_words, int max_states, double* score, int32_t* states, int64_t states_stride, int32_t* starts,
                    int32_t* stops, int32_t* status, void* ws, size_t ws_bytes, void* stream);
/* host twin: the source as po_ctc_loss_h takes it; states_h (or NULL): n rows of states_stride, which must hold the longest
 * item (PO_E_ARG naming both otherwise); starts_h / stops_h (or NULL): label_off_h[n] - label_off_h[0] values */
int po_forced_align_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                      const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, int normalize,
                      const int* perm_h, const int32_t* labels_h, const int64_t* label_off_h, int model, double* score_h,
                      int32_t* states_h, int64_t states_stride, int32_t* starts_h, int32_t* stops_h, int32_t* status_h);

/* ---- read accuracy against truth on tensors where they lie (po_acc.hip) ------------------------------------
 * po_logits_path: the argmax path of every item as uint8 codes 0..3.  Items, row_off and dtypes are po_ingest_strided's (f64
 * too: nothing is normalised), C must be 5, perm_h (host, or NULL) as po_ctc_loss takes it: canonical column c (A, C, G, T,
 * blank) is source column perm_h[c].  Per frame the class of the first maximum of the 5 raw values in canonical order: a later
 * value replaces the best only when it is strictly greater, or when it is NaN and the best is not.  PO_KIND_POREOVER: every
 * frame whose class is no blank emits it, repeats kept; PO_KIND_BONITO: a frame emits when its class is no blank and differs
 * from the previous frame's class.  Item i's codes go to pred + i * pred_stride, their count to pred_len[i]; what lies past
 * the count is left alone.  An item with more frames than pred_stride writes no code and pred_len[i] = -1.
 * Enqueue-only on `stream`.  Before any HIP call: PO_E_UNSUPPORTED for PO_KIND_FLIPFLOP; PO_E_ARG for an unknown kind, negative
 * n, C != 5, an unknown dtype, a perm that is no permutation, a negative pred_stride, null pointers with n > 0; the host twin
 * (the source as po_ingest_strided_h takes it) knows the lengths and also refuses a pred_stride that cannot hold the longest
 * item, naming both.  n == 0: PO_OK.
 *
 * po_edit_stats: global unit-cost alignment of hypothesis a against truth b, pair i = a[a_off[i] ..) of a_len[i] bytes
 * against b[b_off[i] ..) of b_len[i] bytes (a_len / b_len device int32, or NULL for off[i+1] - off[i]; bytes are compared for
 * equality).  dist[i] = the edit distance d; matches[i] = the most matches m over all alignments of distance d.  With the
 * lengths la, lb: mismatches = la + lb - 2m - d, insertions (bytes of a that b lacks) = d - lb + m, deletions = d - la + m,
 * alignment length = m + d, identity = m / (m + d).  status[i]: 0; PO_E_CAP with dist = matches = -1 where the shorter
 * string has more than PO_EDIT_MAX_SHORT = 4095 bytes or the longer more than PO_EDIT_STATS_MAX_LONG; PO_E_ARG with -1, -1
 * for a negative length.  The rest of the batch is answered; the same pair gives the same bits at every batch position.
 * Enqueue-only on `stream`.  PO_E_ARG before any HIP call: negative n, null pointers with n > 0; the host twin also refuses
 * tables that decrease and a length outside its offsets' room (its tables' first entry need not be 0).  n == 0: PO_OK. */
#define PO_EDIT_STATS_MAX_LONG 262142
int po_logits_path(const po_ingest_item* items, const int64_t* row_off, int n, int C, int dtype, const int* perm_h, int kind,
                   uint8_t* pred, int64_t pred_stride, int32_t* pred_len, void* stream);
int po_logits_path_h(const void* src_h, int64_t src_elems, const int64_t* item_off_h, const int64_t* row_stride_h,
                     const int64_t* col_stride_h, const int64_t* row_off_h, int n, int C, int dtype, const int* perm_h, int kind,
                     uint8_t* pred_h, int64_t pred_stride, int32_t* pred_len_h);
int po_edit_stats(const uint8_t* a, const int64_t* a_off, const int32_t* a_len, const uint8_t* b, const int64_t* b_off,
                  const int32_t* b_len, int n, int32_t* dist, int32_t* matches, int32_t* status, void* stream);
int po_edit_stats_h(const uint8_t* a_h, const int64_t* a_off_h, const int32_t* a_len_h, const uint8_t* b_h, const int64_t* b_off_h,
                    const int32_t* b_len_h, int n, int32_t* dist_h, int32_t* matches_h, int32_t* status_h);

/* ---- where the edits sit: ops, confusion (po_aln.hip) -------------------------------------------------------
 * po_edit_align: po_edit_stats' alignment with its columns.  Pairs, lengths, dist, matches and the caps are po_edit_stats'.
 * The ops of pair i go to ops + i * ops_stride, one byte a column, front to back: 0 '=' (equal bytes), 1 'X' (unequal), 2 'I'
 * (a byte of a that b lacks), 3 'D' (a byte of b that a lacks); ops_len[i] = m + d of them, exactly m of them 0; bytes at and
 * past ops_len[i] are left untouched.  With D the key table of §23.1 (rows a, columns b) the walk goes from (la, lb) to (0, 0)
 * and takes at (i, j) the first move that holds: the diagonal if D[i][j] == D[i-1][j-1] + (a[i-1] != b[j-1] ? 4096 : -1), else
 * I if D[i][j] == D[i-1][j] + 4096, else D.  So the ops are a function of the two strings alone, whichever string the kernel
 * puts on its lanes; a gap in a homopolymer goes to its left end.
 * trace: device words the kernels use between them; pair i's room is trace_off[i+1] - trace_off[i] words from trace +
 * trace_off[i] (trace_off: device int64[n + 1], non-decreasing), and po_edit_align_trace_words(la, lb) words hold a pair of la
 * against lb bytes.  That function (host, no HIP call) is non-decreasing in both arguments (lengths past the caps count as the
 * caps), so a bound on the lengths bounds the room.
 * confusion (or NULL): n tables of 5 x 5 int32, confusion[i * 25 + r * 5 + h] = the columns of pair i whose b byte is r and
 * whose a byte is h, 4 standing for a gap: '=' counts [c][c], 'X' [b][a], 'I' [4][a], 'D' [b][4]; [4][4] is 0.  A column that
 * consumes a byte above 3 is counted in no cell.
 * status[i]: 0; PO_E_CAP with dist = matches = ops_len = -1 at po_edit_stats' caps; PO_E_CAP with dist and matches answered
 * and ops_len = -1 where the pair's room is below po_edit_align_trace_words(la, lb) or m + d > ops_stride: nothing is written
 * to that pair's trace, ops or confusion; PO_E_ARG with -1 everywhere for a negative length.  The rest of the batch is
 * answered; the same pair gives the same bits at every batch position.
 * Enqueue-only on `stream`: no allocation, no host read of device memory, no synchronisation.  PO_E_ARG before any HIP call:
 * negative n, negative ops_stride, null pointers with n > 0 (confusion may be NULL).  n == 0: PO_OK.  The host twin sizes and
 * owns the trace; ops_h and confusion_h go up as they are, so untouched bytes come back as they were; it also refuses tables
 * that decrease and a length outside its offsets' room. */
#define PO_EDIT_ALIGN_CELLS 25
size_t po_edit_align_trace_words(int64_t la_max, int64_t lb_max);
int po_edit_align(const uint8_t* a, const int64_t* a_off, const int32_t* a_len, const uint8_t* b, const int64_t* b_off,
                  const int32_t* b_len, int n, uint32_t* trace, const int64_t* trace_off, uint8_t* ops, int64_t ops_stride,
                  int32_t* ops_len, int32_t* dist, int32_t* matches, int32_t* confusion, int32_t* status, void* stream);
int po_edit_align_h(const uint8_t* a_h, const int64_t* a_off_h, const int32_t* a_len_h, const uint8_t* b_h, const int64_t* b_off_h,
                    const int32_t* b_len_h, int n, uint8_t* ops_h, int64_t ops_stride, int32_t* ops_len_h, int32_t* dist_h,
                    int32_t* matches_h, int32_t* confusion_h, int32_t* status_h);

/* ---- transducer.argmax_decode / viterbi_decode ------------------------------------------
 * replaces transducer.py:27-33 (argmax), :72-73 (poreover), :83-89 (bonito), :35-59 +
 * :94-103 (flip-flop Viterbi) and pair_decode.get_sequence_mapping (pair_decode.py:114-142).
 *   path    int8[total_rows]   per-frame state                          (may be NULL)
 *   map     int32[total_rows]  frame index of each emitted base, written at map + y_off[i]
 *                              for read i, seq_len[i] entries            (may be NULL)
 * seq capacity per read must be >= T_i.  */
size_t po_viterbi_workspace_bytes(int n, int64_t total_rows, int C, int kind);
int po_viterbi_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int kind,
                     int8_t* path,
                     char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* map,
                     int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- decoding_cpp.cpp_beam_search ---------------------------------------------------------
 * replaces decoding_cpp.pyx:88-103 -> BeamSearch.h:400-408 beam_search(y, t_max, alphabet,
 * beam_width, model) -> beam_search_<Tree,Beam> (BeamSearch.h:18-58).  */
size_t po_beam1d_workspace_bytes(int n, int64_t total_rows, int64_t max_rows, int C, int beam_width,
                                 int model);
int po_beam1d_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int beam_width,
                    int model, char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- decoding_cpp.cpp_beam_search_2d ------------------------------------------------------
 * replaces decoding_cpp.pyx:107-139 -> BeamSearch.h:411-458 beam_search(y1, y2, U, V, alphabet,
 * envelope_ranges, beam_width, model, method): method row_col = :262-397 (CLI default,
 * __main__.py:89), row = :110-172 / :175-260, grid = BeamSearch2.h:33-184 (hidden upstream option).
 * env rows are [lo, hi) per row of y1; env == NULL: "row" runs its no-envelope form and every other
 * method runs grid without an envelope, as the reference's dispatcher does (BeamSearch.h:441-458) —
 * size the workspace with PO_METHOD_GRID_NOENV in that case.  grid needs row starts that do not move
 * backwards (PO_E_UNSUPPORTED otherwise) and keeps 2 x V x beam_width nodes of cell beams per pair in
 * flight; without an envelope every read-1 time of a node stays readable, so it only fits short reads
 * (PO_E_NOMEM otherwise).
 * The size query is where the register-state route's slice pool is made (first query per device, tree model and lane layout
 * that selects the route: po_reg_pool_prewarm above) — so that the launch that follows allocates nothing.  */
size_t po_beam2d_workspace_bytes(int n, int64_t total_rows1, int64_t total_rows2, int64_t max_rows1,
                                 int64_t max_rows2, int C, int beam_width, int model, int method);
int po_beam2d_batch(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                    const int32_t* env, int n, int C, const char* alphabet, int beam_width, int model,
                    int method, char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status,
                    void* ws, size_t ws_bytes, void* stream);

/* ---- decoding_cpp.cpp_forward ---------------------------------------------------------------
 * replaces decoding_cpp.pyx:49-65 -> forward(y, t_max, label, alphabet, model) (PrefixTree.h:751-759):
 * log P(label | y) under the model's tree recurrence.  labels: concatenated characters (device),
 * label_off int64[n+1]; characters outside the alphabet count as its first symbol, as upstream. */
size_t po_forward_workspace_bytes(int n, int64_t max_rows, int model);
int po_forward_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int model,
                     const char* labels, const int64_t* label_off, double* logp, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream);

/* ---- decoding_cpp.cpp_viterbi_acceptor -------------------------------------------------------
 * replaces decoding_cpp.pyx:69-84 -> viterbi_acceptor_poreover (Forward.h:14-121): best alignment
 * path of a known label, band +-band_size around the diagonal.  path int32[total_rows] (blank = A). */
size_t po_viterbi_acceptor_workspace_bytes(int n, int64_t max_rows, int64_t max_label);
int po_viterbi_acceptor_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet,
                              int band_size, const char* labels, const int64_t* label_off, int32_t* path,
                              int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- prefix_search.prefix_search_log_cy -----------------------------------------------------
 * replaces prefix_search.py:176-238 (with decoding_cy.forward_vec_log, decoding_cy.pyx:127-156):
 * Graves prefix search of each item; an item is any row range [y_off[i], y_off[i+1]) of y, so the
 * windows of `decode --algorithm prefix` (decode.py:182-188) are just finer offsets into one matrix.
 * logp: log-probability of the returned label.  CTC model ('poreover') only, as upstream. */
size_t po_prefix_search_workspace_bytes(int n, int64_t max_rows);
int po_prefix_search_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, char* seq,
                           const int64_t* seq_off, int32_t* seq_len, double* logp, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream);

/* ---- align.global_pair / align.global_pair_banded -------------------------------------------
 * replaces align/align.pyx:29-98 (band_width <= 0: full Needleman-Wunsch) and :100-178 (banded, as
 * written upstream), match 2 / mismatch -1 / gap -1.  seqs: concatenated characters, pair i =
 * [seq_off[2i], seq_off[2i+1]) and [seq_off[2i+1], seq_off[2i+2]).  Outputs: the two alignment rows
 * (same length ncol[i], '-' for gaps) at aln1/aln2 + aln_off[i]; capacity len1 + len2 + 8 suffices. */
size_t po_align_workspace_bytes(int n, int64_t max_len1, int64_t max_len2, int band_width);
int po_align_batch(const char* seqs, const int64_t* seq_off, int n, int band_width, char* aln1, char* aln2,
                   const int64_t* aln_off, int32_t* ncol, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* the third item align.global_pair returns (align.pyx:34-52,98): its dense DP matrix, (len1 + 1) x (len2 + 1) int32 row-major
 * at dp + dp_off[i] (dp_off[n] = total cells), with the reference's score arguments.  Enqueue-only, no workspace. */
int po_nw_matrix_batch(const char* seqs, const int64_t* seq_off, int n, int match, int mismatch, int gap_cost, int32_t* dp,
                       const int64_t* dp_off, int32_t* status, void* stream);

/* ---- envelope.get_alignment_columns + build_envelope -----------------------------------------
 * replaces decoding/envelope.py:26-87: alignment rows + the frame index of every base of both reads
 * (map*, get_sequence_mapping) + signal lengths U, V -> per-row column range [lo, hi) of read 2,
 * padded and fixed up as upstream.  env rows of pair i at env + 2 * env_off[i] (U[i] rows). */
size_t po_envelope_workspace_bytes(int n, int64_t max_ncol);
int po_envelope_batch(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol, int n,
                      const int32_t* map1, const int64_t* map1_off, const int32_t* map2, const int64_t* map2_off,
                      const int32_t* U, const int32_t* V, int padding, int32_t* env, const int64_t* env_off,
                      int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- decoding_cpp.cpp_pair_gamma_log_envelope / decoding_cy.pair_gamma_log -------------------
 * replaces decoding_cpp.pyx:168-188 -> pair_gamma_log_envelope (Gamma.h:15-98) and the dense
 * decoding_cy.pair_gamma_log (decoding_cy.pyx:177-220): gamma(0,0) = log P(both reads emit the same
 * label).  env: (U_i + 1) rows per pair with INCLUSIVE column ends (Gamma.h:26-30), rows of pair i at
 * env + 2 * env_off[i]; env == NULL: dense.  flavor 0 = Gamma.h arithmetic (logaddexp, -inf),
 * 1 = decoding_cy arithmetic (log(exp+exp), LOG_0 = -9999), 2 = decoding_cy.pair_gamma_log_envelope
 * (decoding_cy.pyx:224-271; envelope only: log(exp+exp), -inf defaults, cells [start, min(end, V-1)] computed).
 * 3 = prefix_search.pair_gamma_log (prefix_search.py:35-65), the dense matrix of the reference's Python path: -inf defaults,
 * the base sum log sum_c exp(y1[u][c] + y2[v][c]) shifted by its maximum as scipy.special.logsumexp shifts it (by 0 where the
 * maximum is not finite), np.logaddexp.  Flavours 0 and 3 differ where every base sum of a cell is below exp's range (two
 * log-probabilities that add up to less than about -745): flavour 0 then has log(0) = -inf, flavour 3 the value.
 * dense_out (optional): the full (U+1) x (V+1) gamma matrices at dense_out + dense_off[i] (-inf outside an envelope).  max_cells = largest per-pair number of
 * stored cells (sum over rows of end - start + 1), as used to size the workspace. */
size_t po_pair_gamma_workspace_bytes(int n, int64_t max_cells, int64_t max_rows1, int64_t max_rows2);
int po_pair_gamma_batch(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                        const int32_t* env, const int64_t* env_off, int n, int C, int flavor, int64_t max_cells,
                        double* gamma00, double* dense_out, const int64_t* dense_off, int32_t* status, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- pair_decode.pair_decode_helper stage chain -------------------------------------------
 * replaces pair_decode.py:305-529 for the default route (--method envelope --algorithm beam
 * --single viterbi): 1-D Viterbi of both reads (:360-362) -> length skip (:372-375) ->
 * get_sequence_mapping (:377-382) -> align.global_pair_banded / global_pair
 * (align.pyx:100-178 / :29-98; :385-389) -> identity skip (:391-398) ->
 * envelope.get_alignment_columns + build_envelope (envelope.py:26-87; :500-501) ->
 * cpp_beam_search_2d (:166-173,511).  All stages run on the device.
 *   seq1d / seq1d_off / len1 / len2: the two 1-D basecalls (read 1 at seq1d + seq1d_off[2i],
 *                                    read 2 at seq1d + seq1d_off[2i+1])
 *   identity  float64[n]  matches / alignment columns
 *   env_out   int32[2*total_rows1]  the envelope that was used (may be NULL) */
typedef struct {
    int beam_width;        /* --beam_width 5                     */
    int model;             /* PO_MODEL_*                         */
    int method;            /* --beam_search_method row_col       */
    int padding;           /* --padding 5                        */
    int full_alignment;    /* --alignment full (0 = banded, 500): read 2's basecall of at most 2048 bases,
                              a longer one gives that pair PO_E_UNSUPPORTED (read 1's is not limited) */
    int diagonal_envelope; /* --diagonal_envelope                */
    int diagonal_width;    /* --diagonal_width 50                */
} po_pair_options;
size_t po_pair_decode_workspace_bytes(int n, int64_t total_rows1, int64_t total_rows2, int64_t max_rows1,
                                      int64_t max_rows2, int C, const po_pair_options* opt);
int po_pair_decode_batch(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                         int n, int C, const po_pair_options* opt, char* seq1d, const int64_t* seq1d_off,
                         int32_t* len1, int32_t* len2, double* identity, int32_t* env_out, char* seq,
                         const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- pair-decode --skip_matches on the device (pair_decode.py:412-467,512-522) ----------------------
 * Runs of at least skip_threshold matching alignment columns (and of at least indel_threshold gap columns; the reference
 * passes 100) are ANCHORS, copied from the 1-D basecalls; the stretches between them (BOXES) go through the pair beam search
 * inside their slice of the envelope, and the pieces are joined in signal order.  The rule is csrc/po_skip_rules.h's.  The
 * size of the box phase depends on the data, so the route is two calls, neither of which allocates device memory:
 *   po_pair_skip_plan   Viterbi of both reads, alignment + skips + envelope (as po_pair_decode_batch), anchors and boxes.  It
 *                       SYNCHRONISES the stream (one small D2H read of the box totals) and returns them in *totals (host).
 *                       status[i]: 0, a skip, PO_E_NO_ANCHOR, PO_E_BOX, or what po_pair_decode_batch's pre-stages give.
 *                       n_anchors / n_boxes: int32[n] (a pair with a non-zero status has 0 boxes).
 *   po_pair_skip_run    gathers the boxes' rows and shifted envelopes, runs the pair beam search on all boxes of the batch,
 *                       and stitches anchors and box consensuses into seq.  plan_ws must still hold what the plan left in
 *                       it (same n, offsets, options and thresholds).  A box whose beam status is non-zero gives its pair
 *                       that status (the first such box) and no consensus; a consensus longer than its room is PO_E_CAP.
 * opt->diagonal_envelope is PO_E_UNSUPPORTED; opt->full_alignment and all three tree models work.  The anchor and box tables
 * (int32 x 4 per row: cs, ce, type 0 mat / 1 ins / 2 del, position | b0, b1, lo, hi) live in plan_ws; the host twin below
 * copies them out.  Pair i's anchors start at row (rows1 before i + rows2 before i + 16 i) /
 * min(skip_threshold, indel_threshold) + i of the anchor table, its boxes at that row + i of the box table. */
typedef struct {
    int64_t n_boxes;      /* boxes of all pairs whose status is 0                */
    int64_t total_rows1;  /* their rows of read 1 / read 2 (read 2's overlap)    */
    int64_t total_rows2;
    int64_t max_rows1;    /* the largest box                                     */
    int64_t max_rows2;
} po_skip_totals;
size_t po_pair_skip_plan_workspace_bytes(int n, int64_t total_rows1, int64_t total_rows2, int64_t max_rows1, int64_t max_rows2,
                                         int C, const po_pair_options* opt, int skip_threshold, int indel_threshold);
int po_pair_skip_plan(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                      const po_pair_options* opt, int skip_threshold, int indel_threshold, char* seq1d,
                      const int64_t* seq1d_off, int32_t* len1, int32_t* len2, double* identity, int32_t* status,
                      int32_t* n_anchors, int32_t* n_boxes, void* plan_ws, size_t plan_ws_bytes, po_skip_totals* totals,
                      void* stream);
size_t po_pair_skip_run_workspace_bytes(int n, int C, const po_pair_options* opt, const po_skip_totals* totals);
int po_pair_skip_run(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                     const po_pair_options* opt, int skip_threshold, int indel_threshold, const po_skip_totals* totals,
                     void* plan_ws, size_t plan_ws_bytes, char* seq, const int64_t* seq_off, int32_t* seq_len,
                     int32_t* status, void* run_ws, size_t run_ws_bytes, void* stream);

/* ---- host-buffer conveniences (numpy callers): allocate, copy in, launch, copy out, free ----
 * Same semantics as the device-pointer forms with every pointer a HOST pointer; synchronous.
 * INPUT offset tables (y_off_h, y1_off_h, y2_off_h, label_off_h, and the tables of sequences, alignments, maps and
 * envelopes that a call reads) need not start at 0: a call may be given items k..k+n of a larger batch as off + k and the
 * batch's own data pointers.  Arrays with one entry per row or per label of an input (env_h of po_beam2d_batch_h, the frame
 * maps of po_pair_decode_from_1d_batch_h, guide_h) are read at the same offsets, and po_label_align_batch_h / po_qual_batch_h
 * write map_h / odds_h at label_off_h[0] on, the labels' own places.  (previous_h of po_forward_vec_batch_h is the
 * exception: the n items' rows from previous_h[0] on.)  Every other output starts at element 0 of its array, and OUTPUT
 * offset tables (seq_off_h, seq1d_off_h, aln_off_h, env_off_h of po_envelope_batch_h, dense_off_h, dp_off_h) start at 0.
 * Three calls require row_off_h[0] / off_h[0] == 0 on input and answer PO_E_ARG otherwise: po_ingest_batch_h,
 * po_decode_1d_batch_h and po_map_sketch_h (as do the mapper's po_map_batch_h and po_map_pairs_h further down). */
int po_ingest_batch_h(const void* src_h, const int64_t* row_off_h, int n, int C, int mode, const int* perm_h,
                      int reverse, double* out_h);
/* `poreover decode` for a batch of traces in one call (decode.py:114-192: model_from_trace + viterbi_decode /
 * cpp_beam_search): src_h = the basecaller's own output (float32 logits, uint8 trace or float64 log-probabilities, rows of
 * all reads back to back, row_off_h[0] == 0), ingest on the device as po_ingest_batch, then Viterbi (beam_width <= 0,
 * `kind`) or the 1-D beam search (`model`, beam_width) — no host log-softmax, 4 or 1 bytes per value over PCIe. */
int po_decode_1d_batch_h(const void* src_h, const int64_t* row_off_h, int n, int C, int in_mode, const int* perm_h, int reverse,
                         const char* alphabet, int kind, int beam_width, int model, char* seq_h, const int64_t* seq_off_h,
                         int32_t* seq_len_h, int32_t* status_h);
int po_viterbi_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int kind,
                       int8_t* path_h,
                       char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* map_h,
                       int32_t* status_h);
int po_beam1d_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                      int beam_width, int model,
                      char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h);
int po_forward_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int model,
                       const char* labels_h, const int64_t* label_off_h, double* logp_h, int32_t* status_h);
int po_viterbi_acceptor_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                                int band_size, const char* labels_h, const int64_t* label_off_h, int32_t* path_h,
                                int32_t* status_h);
/* decoding_cy.viterbi_acceptor (decoding_cy.pyx:60-123), the Cython twin of the acceptor, reproduced as written
 * (dense, '>' tie rule, its own band expression; band_size 0 = whole matrix).  A label character outside the
 * alphabet is PO_E_ARG (KeyError upstream).  (Device-pointer form: po_viterbi_acceptor_batch with
 * band_size = -(band + 1).) */
int po_viterbi_acceptor_cy_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                                   int band_size, const char* labels_h, const int64_t* label_off_h, int32_t* path_h,
                                   int32_t* status_h);
int po_prefix_search_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                             char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, double* logp_h,
                             int32_t* status_h);
int po_align_batch_h(const char* seqs_h, const int64_t* seq_off_h, int n, int band_width, char* aln1_h, char* aln2_h,
                     const int64_t* aln_off_h, int32_t* ncol_h, int32_t* status_h);
int po_nw_matrix_batch_h(const char* seqs_h, const int64_t* seq_off_h, int n, int match, int mismatch, int gap_cost,
                         int32_t* dp_h, const int64_t* dp_off_h, int32_t* status_h);
/* the same with the reference's score arguments (align.pyx:29,100: match, mismatch, gap_cost) */
int po_align_scores_batch_h(const char* seqs_h, const int64_t* seq_off_h, int n, int band_width, int match, int mismatch,
                            int gap_cost, char* aln1_h, char* aln2_h, const int64_t* aln_off_h, int32_t* ncol_h,
                            int32_t* status_h);
int po_envelope_batch_h(const char* aln1_h, const char* aln2_h, const int64_t* aln_off_h, const int32_t* ncol_h, int n,
                        const int32_t* map1_h, const int64_t* map1_off_h, const int32_t* map2_h,
                        const int64_t* map2_off_h, const int32_t* U_h, const int32_t* V_h, int padding,
                        int32_t* env_h, const int64_t* env_off_h, int32_t* status_h);
/* prefix_search.pair_prefix_search_log / _cy (prefix_search.py:247-385) on small boxes: dense gamma
 * (pair_gamma_log of the same flavour) computed on the device, then the pair prefix search.
 * flavor 0: prefix_search.py arithmetic, 1: decoding_cy.  seq at seq_h + seq_off_h[i], capacity
 * seq_off_h[i+1] - seq_off_h[i] (max(U, V) + 1 always suffices). */
int po_pair_prefix_search_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                                  int n, int C, const char* alphabet, int flavor, char* seq_h, const int64_t* seq_off_h,
                                  int32_t* seq_len_h, double* logp_h, int32_t* status_h);
/* The pair prefix search WITH AN ENVELOPE — the working form of decoding_cpp.cpp_pair_prefix_search_log
 * (decoding_cpp.pyx:143-164 -> pair_prefix_search_log, PairPrefixSearch.cpp:79-229; upstream passes its gamma matrices by
 * value and crashes): gamma from the envelope DP of Gamma.h:15-98 (env_h: U_i + 1 rows with INCLUSIVE column ends, rows of
 * pair i at env_h + 2 * env_off_h[i]; -inf outside the stored ranges), the search itself as in the Python paths
 * (prefix_search.py:247-385; flavor selects the arithmetic of the forward rows).  env_h == NULL: the dense search above. */
int po_pair_prefix_search_env_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                                      const int32_t* env_h, const int64_t* env_off_h, int n, int C, const char* alphabet,
                                      int flavor, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, double* logp_h,
                                      int32_t* status_h);
/* decoding_cy.forward_vec_log (decoding_cy.pyx:127-156; flavor 1) / prefix_search.forward_vec_log
 * (prefix_search.py:81-96; flavor 0): one row of the CTC forward matrix for symbol s (-1: blank) and label
 * length i, for every item; previous_h (same layout as out_h: one double per frame, items back to back) is the row
 * of the label without its last symbol and may be NULL for i == 0. */
int po_forward_vec_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, int s, int i, int flavor,
                           const double* previous_h, double* out_h);
int po_pair_gamma_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h,
                          const int32_t* env_h, const int64_t* env_off_h, int n, int C, int flavor, double* gamma00_h,
                          double* dense_out_h, const int64_t* dense_off_h, int32_t* status_h);
int po_beam2d_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h,
                      const int64_t* y2_off_h, const int32_t* env_h, int n, int C, const char* alphabet,
                      int beam_width, int model, int method, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h,
                      int32_t* status_h);
/* pair decode with the 1-D stage supplied by the caller (pair-decode --single beam, pair_decode.py:363-370:
 * cpp_beam_search + cpp_viterbi_acceptor): seq1d / len1 / len2 and the frame maps are INPUTS.
 * map1_h / map2_h: int32, frame index of every base, read i at map + y*_off[i]. */
int po_pair_decode_from_1d_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h,
                                   const int64_t* y2_off_h, int n, int C, const po_pair_options* opt,
                                   const char* seq1d_h, const int64_t* seq1d_off_h, const int32_t* len1_h,
                                   const int32_t* len2_h, const int32_t* map1_h, const int32_t* map2_h,
                                   double* identity_h, int32_t* env_out_h, char* seq_h, const int64_t* seq_off_h,
                                   int32_t* seq_len_h, int32_t* status_h);
int po_pair_decode_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h,
                           const int64_t* y2_off_h, int n, int C, const po_pair_options* opt, char* seq1d_h,
                           const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h, double* identity_h,
                           int32_t* env_out_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h,
                           int32_t* status_h);
/* The whole --skip_matches chain on host buffers: po_pair_decode_batch_h's arguments and outputs (env_out_h: the whole
 * pair's envelope, may be NULL) plus the two thresholds, n_anchors_h / n_boxes_h (int32[n]) and, where anchors_h / boxes_h are
 * not NULL, the anchor and box tables (int32 x 4 per row, rows as po_pair_skip_plan places them: tab_rows_h[i], int64[n + 1], gets
 * pair i's first anchor row; its boxes start at row tab_rows_h[i] + i; anchors_h needs tab_rows_h[n] rows, boxes_h n more).
 * stage_ms_h (float[4] or NULL): device ms of plan, gather, beam, stitch. */
int po_pair_skip_decode_batch_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h, int n,
                                int C, const po_pair_options* opt, int skip_threshold, int indel_threshold, char* seq1d_h,
                                const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h, double* identity_h,
                                int32_t* env_out_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h,
                                int32_t* status_h, int32_t* n_anchors_h, int32_t* n_boxes_h, int64_t* tab_rows_h,
                                int32_t* anchors_h, int32_t* boxes_h, po_skip_totals* totals_h, float* stage_ms_h);
/* The anchor / box stage alone, for given alignments (rows of pair i at aln*_h + aln_off_h[i], ncol_h[i] columns), frame maps,
 * signal lengths and envelopes (rows of pair i at env_h + 2 * env_off_h[i]).  Tables as above with tab_rows_h[i] =
 * (aln_off_h[i] - aln_off_h[0]) / min(thresholds) + i.  status_h: 0, PO_E_NO_ANCHOR, PO_E_BOX (PO_E_ARG: ncol < 1). */
int po_skip_boxes_batch_h(const char* aln1_h, const char* aln2_h, const int64_t* aln_off_h, const int32_t* ncol_h, int n,
                          const int32_t* map1_h, const int64_t* map1_off_h, const int32_t* map2_h, const int64_t* map2_off_h,
                          const int32_t* U_h, const int32_t* V_h, const int32_t* env_h, const int64_t* env_off_h,
                          int skip_threshold, int indel_threshold, int32_t* n_anchors_h, int32_t* n_boxes_h,
                          int64_t* tab_rows_h, int32_t* anchors_h, int32_t* boxes_h, int32_t* status_h);

/* ---- host-to-strings pipeline of the pair decoder ---------------------------------------------------
 * replaces the reference's fan-out of pair_decode_helper over worker processes (pair_decode.py:292-297)
 * together with the trace loading each worker does: decode.load_logits / logit_to_log_likelihood
 * (decode.py:34-51), the Bonito column order (decode.py:79), the uint8 trace scaling (decode.py:89-93) and
 * transducer.reverse_complement of read 2 (transducer.py:68-70,104-106; pair_decode.py:323-329).
 * Inputs are HOST arrays as the basecaller wrote them: y1_h[i] / y2_h[i] point to C-contiguous (rows1[i], C) /
 * (rows2[i], C) matrices of float32 logits (in_mode PO_INGEST_LOGITS_F32), uint8 traces (PO_INGEST_TRACE_U8) or
 * float64 log-probabilities (PO_INGEST_F64); perm1 / perm2 (C ints or NULL): column order of read 1 / read 2
 * (out[:, c] = in[:, perm[c]]), reverse2: read 2 is time-reversed.  The pairs are decoded in waves of at most
 * wave_pairs pairs / wave_rows frames through three slots {stream, pinned staging, device buffers, workspace}:
 * waves k + 1 and k + 2 are packed and uploaded while wave k decodes, device memory is bounded by three waves whatever
 * n is, and nothing is allocated per call once the buffers have grown to the wave size.  wave_pairs 0: a job of at
 * most 4 096 pairs is one wave, a larger one is cut into even waves of about 2 500 pairs.
 * Outputs as po_pair_decode_batch_h (all host); env_out_h may be NULL (rows of pair i at 2 * sum(rows1[:i])).
 * A pipeline belongs to one host thread and one device.  */
typedef struct po_pipeline po_pipeline;
po_pipeline* po_pipeline_create(int device, int wave_pairs, int64_t wave_rows, int host_threads); /* 0 = defaults */
void po_pipeline_destroy(po_pipeline* p);
int po_pipeline_pair_decode(po_pipeline* p, const void* const* y1_h, const int64_t* rows1, const void* const* y2_h,
                            const int64_t* rows2, int n, int C, int in_mode, const int* perm1, const int* perm2,
                            int reverse2, const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h,
                            int32_t* len1_h, int32_t* len2_h, double* identity_h, int32_t* env_out_h, char* seq_h,
                            const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h);
/* host milliseconds of the last call: packing, waiting for the device, whole call; number of waves */
int po_pipeline_stats(po_pipeline* p, double* pack_ms, double* wait_ms, double* total_ms, int* waves);

/* ---- several devices, one process ------------------------------------------------------------
 * Replaces the reference's fan-out over worker processes on a multi-GPU node (pair_decode.py:292-297: a
 * multiprocessing.Pool over pair_decode_helper): one pipeline per entry of `devices` (an index may repeat), each driven
 * by its own host thread inside the call, all taking waves of the batch from one planner — uneven pairs balance
 * themselves — and writing their results straight into the caller's arrays at the pairs' own indices (input order; no
 * gather, no copy between processes, no collective).  Arguments and results as po_pipeline_pair_decode; synchronous.
 * po_multi_stats: pairs decoded and pack / wait / total milliseconds of pipeline i in the last call. */
typedef struct po_multi po_multi;
po_multi* po_multi_create(const int* devices, int ndev, int wave_pairs, int64_t wave_rows, int host_threads);
void po_multi_destroy(po_multi* m);
int po_multi_devices(po_multi* m);
int po_multi_pair_decode(po_multi* m, const void* const* y1_h, const int64_t* rows1, const void* const* y2_h,
                         const int64_t* rows2, int n, int C, int in_mode, const int* perm1, const int* perm2,
                         int reverse2, const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h,
                         int32_t* len1_h, int32_t* len2_h, double* identity_h, int32_t* env_out_h, char* seq_h,
                         const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h);
int po_multi_stats(po_multi* m, int i, int* pairs, double* pack_ms, double* wait_ms, double* total_ms, int* waves);
/* the waves such a call is cut into, in the order they are handed out (touches no device): first[k], count[k] for
 * k < returned number of waves (at most cap are written); wave_pairs / wave_rows 0 = the pipeline's defaults */
int po_wave_plan(const int64_t* rows1, const int64_t* rows2, int n, int wave_pairs, int64_t wave_rows, int ndev, int* first,
                 int* count, int cap);

/* ---- basecalling network forward pass (`call`) ------------------------------------------------
 * Replaces the reference's TensorFlow forward pass of call_helper (network.py:253-282): the Keras models of build_model
 * (network.py:15-55) on windows of scaled FAST5 signal, then tf.nn.softmax.  f32 weights, f32 arithmetic — by default: two
 * opt-in selectors below put bf16 operands under the GRU input projections (po_set_call_precision) and under the
 * recurrence's product h·U (po_set_recur_precision), each with f32 products and sums.
 *   - signal:  n windows of T f32 samples each, window-major (n * T values); each window starts from a zero state
 *   - layers_h: HOST array of n_layers po_call_layer, in the order the model applies them; layer k's cin is layer
 *              k-1's cout (1 for the first); the last layer is PO_CALL_DENSE with cout 5
 *   - weights: every layer's f32 tensors back to back, in Keras' layouts, layer by layer:
 *              PO_CALL_CONV   kernel (kernel, cin, cout), bias (cout)          Conv1D, padding "same", stride 1, ReLU
 *              PO_CALL_BIGRU  forward then backward GRU(H), each: kernel (cin, 3H), recurrent kernel (H, 3H),
 *                             bias (2, 3H) (input bias, recurrent bias; reset_after); gates z, r, h; cout = 2H,
 *                             [forward, backward] with the backward output in forward time order (Bidirectional)
 *              PO_CALL_GRU    one forward GRU(H), tensors as above; cout = H
 *              PO_CALL_GRU_BACK  GRU(H, go_backwards = True): walks the window from its end and writes its outputs in
 *                             that reversed order (the next layer consumes them so); cout = H
 *              PO_CALL_DENSE  kernel (cin, 5), bias (5)
 *              H, the units per direction, is read from cout: 16, 32, 48, 64, 80, 96, 112 or 128 (one wave of the
 *              recurrence per 16 units, at most 8), the same in every GRU layer of a model; a GRU direction holds
 *              cin * 3H + H * 3H + 2 * 3H weights.  Any other width, or layers of different widths, is
 *              PO_E_UNSUPPORTED with the width in the message, from every entry that takes a model (po_train_create too).
 *   - probs:   n * T * 5 softmax probabilities; logits (or NULL): the Dense outputs before the softmax
 *   - stage_ms_h (or NULL): HOST float[4] to which device milliseconds are ADDED per stage — 0 Conv1D, 1 GRU input
 *              projection, 2 GRU recurrence, 3 Dense + softmax — measured with events (the call then synchronises)
 * po_call_workspace_bytes returns 0 for an unusable model.  po_call_batch_h takes host arrays, runs the windows in
 * passes of bounded device memory (a window's output does not depend on the pass it runs in) and is synchronous. */
#define PO_CALL_CONV 0
#define PO_CALL_BIGRU 1
#define PO_CALL_GRU 2
#define PO_CALL_GRU_BACK 3
#define PO_CALL_DENSE 4
typedef struct po_call_layer {
    int kind, cin, cout, kernel; /* kernel: Conv1D kernel size (0 otherwise) */
} po_call_layer;
size_t po_call_workspace_bytes(int n, int T, const po_call_layer* layers_h, int n_layers);
int po_call_batch(const float* signal, int n, int T, const po_call_layer* layers_h, int n_layers, const float* weights,
                  int64_t n_weights, float* probs, float* logits, void* ws, size_t ws_bytes, void* stream,
                  float* stage_ms_h);
int po_call_batch_h(const float* signal_h, int n, int T, const po_call_layer* layers_h, int n_layers,
                    const float* weights_h, int64_t n_weights, float* probs_h, float* logits_h, float* stage_ms_h);

/* The precision of the GRU input projections x·W + b_in, process-wide like po_set_chain_mode and read once per
 * po_call_batch call — so by everything that runs the network through it: po_call_batch_h, po_basecall_batch_h,
 * po_basecall_fastq_batch_h, po_pair_basecall_batch_h (po_train_* is not affected):
 *   PO_CALL_F32   (default) f32 operands on v_mfma_f32_16x16x4_f32
 *   PO_CALL_BF16  x and W rounded to bf16 (round to nearest even, csrc/po_bf16_rules.h), products and sums in f32 on
 *                 v_mfma_f32_16x16x32_bf16, the bias added in f32; P, the recurrence, Conv1D, Dense and the softmax stay f32.
 *                 About one called base in a thousand differs from f32.  po_call_workspace_bytes then includes room for
 *                 the bf16 copy of a layer's W (a constant: what the query answers for n = 0), made anew in every call
 *                 (its time counts in stage 1); a workspace sized
 *                 under PO_CALL_F32 and used under PO_CALL_BF16 is PO_E_CAP.  Built for GRU layers of 128 units alone: a
 *                 model of another width run under PO_CALL_BF16 is PO_E_UNSUPPORTED, naming the precision and the width.
 * Any other value is PO_E_ARG and leaves the mode as it was.  A trainer has a mode of its own, set per trainer with
 * po_train_set_precision (below). */
#define PO_CALL_F32 0
#define PO_CALL_BF16 1
int po_set_call_precision(int precision);
int po_get_call_precision(void);
/* The projection stage alone of a 128-unit layer, on host buffers: P_h[ndir][M][384] = x_h[M][cin] · w_h[ndir][cin][384] + bin_h[ndir][384] by the
 * kernel(s) of `precision` (explicit: the selector above is not read).  M >= 0 (0: PO_OK, nothing written), cin >= 1, ndir 1
 * or 2; a null pointer, another value or another precision is PO_E_ARG naming the argument, before any allocation. */
int po_gru_proj_h(const float* x_h, int64_t M, int cin, int ndir, const float* w_h, const float* bin_h, int precision,
                  float* P_h);

/* The precision of the GRU recurrence's product h·U, process-wide and read once per po_call_batch call,
 * next to the call precision and independent of it — so by po_call_batch_h, po_basecall_batch_h, po_basecall_fastq_batch_h,
 * po_pair_basecall_batch_h, po_pair_basecall_fastq_batch_h and every group of a po_basecaller or po_pair_basecaller engine — set it
 * around the whole run;
 * po_train_* and po_train_eval are not reached:
 *   PO_RECUR_F32     (default) f32 operands on v_mfma_f32_16x16x4_f32
 *   PO_RECUR_BF16X3  h and U each split in two bf16 values (hi = bf16(v), lo = bf16(v - hi), round to nearest even,
 *                    csrc/po_bf16_rules.h) and h·U taken as hh·Uh + hl·Uh + hh·Ul on v_mfma_f32_16x16x32_bf16 with f32 sums;
 *                    the state, the bias, the gates and every store stay f32.  Every GRU width from 16 to 128; no workspace
 *                    beyond PO_RECUR_F32's.  Logits stay within the f32 path's own bound of a float64 model (1e-3).
 * Any other value is PO_E_ARG naming `precision <value>` and leaves the mode as it was. */
#define PO_RECUR_F32 0
#define PO_RECUR_BF16X3 1
int po_set_recur_precision(int precision);
int po_get_recur_precision(void);
/* The recurrence stage alone, on host buffers, by the kernel po_call_batch launches under `precision` (explicit: the
 * selector above is not read): P_h[ndir][n*T][3H] the input projections, U_h[ndir][H][3H], brec_h[ndir][3H], kind
 * PO_CALL_BIGRU (ndir 2: forward, backward), PO_CALL_GRU or PO_CALL_GRU_BACK (ndir 1).  out_h[n*T][ndir*H] is the layer's
 * output as po_call_batch lays it out; rec_h (or NULL) [ndir][n*T][3H] gets h_prev·U + brec of every step, at the frame the
 * step consumed.  n = 0 is PO_OK and writes nothing.  Refused with PO_E_ARG naming the argument, before any allocation: a
 * null required pointer, n < 0, T < 1, H not one of 16, 32 .. 128 (`H <value> units`), another kind, another precision. */
int po_gru_recur_h(const float* P_h, const float* U_h, const float* brec_h, int n, int T, int H, int kind, int precision,
                   float* out_h, float* rec_h);

/* ---- signal preparation: raw int16 reads to scaled f32 signals on the device --------
 * network.parse_fast5's abasic filter and scaling for a ragged batch of raw reads.  A sample x is kept when lo < x < hi
 * (the reference's 200 / 800); the kept samples of a read, in their order, become f32((f64(x) - a) / b) with a and b per
 * read by the rule of poreover_amd/csrc/po_prep_rules.h: every statistic is an exact integer taken from the read's
 * histogram, so a read's bits depend neither on the batch it is in nor on the schedule of the kernels.
 *   - raw_h:      the raw samples of n_reads reads back to back; raw_off_h int64[n_reads + 1] sample offsets, raw_off_h[0]
 *                 == 0, non-decreasing, a read of 0 to 2^31 - 1 samples
 *   - scaling:    PO_SCALE_* below
 *   - lo, hi:     -32769 <= lo < hi <= 32768 and hi - lo - 1 <= 4096 bins; PO_E_ARG naming both otherwise
 *   - offset_h, alpha_h: double[n_reads], the channel's offset and digitisation / range; read (and required) for
 *                 PO_SCALE_CURRENT alone
 *   - signal_h:   room for raw_off_h[n_reads] f32 values; the kept samples of read i are written at sig_off_h[i]
 *   - sig_off_h:  int64[n_reads + 1], written: from 0; a read with no kept sample has length 0
 *   - stats_h (or NULL): po_prep_stats[n_reads]
 *   - ms_h (or NULL): one float, SET to the device milliseconds of the call's kernels (events; the copies are outside)
 * n_reads == 0 is PO_OK (sig_off_h[0] = 0).  A null pointer is PO_E_ARG naming the argument; every argument error is
 * answered before the first device allocation.  Synchronous, on the current device. */
#define PO_SCALE_STANDARD 0 /* a = mean, b = standard deviation (population) */
#define PO_SCALE_CURRENT 1  /* a = -offset, b = alpha: picoamperes */
#define PO_SCALE_MEDIAN 2   /* a = 0, b = median */
#define PO_SCALE_RESCALE 3  /* a = mean, b = max - min */
#define PO_SCALE_RAW 4      /* a = 0, b = 1 */
typedef struct po_prep_stats {
    int64_t n, S, Q;                     /* kept samples, their sum and their sum of squares */
    int32_t min, max, med_lo, med_hi;    /* smallest, largest and the two middle kept values (0 when n == 0) */
    double a, b;                         /* the scaling's subtrahend and divisor */
} po_prep_stats;
int po_signal_prep_h(const int16_t* raw_h, const int64_t* raw_off_h, int n_reads, int scaling, int lo, int hi,
                     const double* offset_h, const double* alpha_h, float* signal_h, int64_t* sig_off_h,
                     po_prep_stats* stats_h, float* ms_h);

/* ---- `basecall`: scaled signals to decoded strings in one device-resident pass --------
 * The forward pass above, the log-softmax of po_ingest_batch (PO_INGEST_LOGITS_F32) and po_viterbi_batch / po_beam1d_batch
 * in one synchronous call: each read's signal goes up once, the strings come down, and nothing per frame returns to the
 * host in between (unless logits_h asks for it).  Windows may overlap.  For a read of L >= 1 samples, window W >= 1 and
 * overlap O (even, 0 <= O < W), S = W - O:
 *     the read has n = 1 window if L <= W, else n = 1 + ceil((L - W) / S);
 *     window j covers samples [jS, jS + W), zeros at and past L (part of the last window's input, as in `call`), and
 *              runs through the network from a zero state;
 *     output frame t (0 <= t < L) is frame t - jS of window j = clamp(floor((t - O/2) / S), 0, n - 1).
 * O = 0 is `call`'s windowing (n = ceil(L / W)) and gives po_call_batch_h's logits bit for bit; a window's bits do not
 * depend on the pass it runs in, nor a read's on the reads it shares the call with.
 *   - signal_h:  the scaled signals of n_reads reads back to back; sig_off_h int64[n_reads + 1] sample offsets,
 *                sig_off_h[0] == 0; a read without samples is PO_E_ARG naming the read
 *   - window, overlap: as above; window < 1 and an odd, negative or >= window overlap are PO_E_ARG naming the value
 *   - layers_h, n_layers, weights_h, n_weights: the model, as for po_call_batch (its refusals and messages; a weight
 *                count that is not the model's is PO_E_ARG naming both counts)
 *   - alphabet:  4 symbols or NULL ("ACGT"); kind (PO_KIND_*), beam_width and model (PO_MODEL_*) as for
 *                po_decode_1d_batch_h: beam_width <= 0 is Viterbi of `kind`, otherwise the 1-D beam search of `model`.
 *                PO_KIND_FLIPFLOP and PO_MODEL_FLIPFLOP are PO_E_UNSUPPORTED (the network emits a CTC table, blank last)
 *   - max_windows_per_pass: <= 0: as many windows per network pass as ~4 GiB of pass buffers hold (po_call_batch_h's
 *                rule); > 0: at most that many (results do not depend on it)
 *   - seq_h, seq_off_h (from 0), seq_len_h, status_h: the strings, as everywhere; a read's capacity must be at least
 *                its number of samples (PO_E_CAP naming the read otherwise)
 *   - logits_h (or NULL): the stitched Dense outputs, (sig_off_h[n_reads], 5) f32, read after read
 *   - stage_ms_h (or NULL): float[6] device milliseconds, SET by the call: [0..3] po_call_batch's stages summed over the
 *                passes, [4] window gather + stitch + ingest, [5] the decoder
 * Every argument error is answered before the first device allocation. */
int po_basecall_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                        const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                        const char* alphabet, int kind, int beam_width, int model, int max_windows_per_pass,
                        char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                        float* logits_h, float* stage_ms_h);

/* ---- `basecall --fastq`: the same pass, with per-base qualities -----------------------
 * po_basecall_batch_h's arguments, refusals and strings (bit for bit), then, behind the decoder on the same stream and on
 * the table and strings that are on the device already: the Viterbi call of `kind` with its frame map (Viterbi of
 * PO_KIND_POREOVER: the decode itself; otherwise a second, cheap call, so that a PO_KIND_BONITO map whose count differs from
 * the string's - PO_E_ARG in po_viterbi_batch's status, the diagonal here - leaves status_h what po_basecall_batch_h gives), the band guide of every read (quality.call_guides' rule: the map where the scored string is the Viterbi
 * call; otherwise the two are aligned by po_align_batch, band_width = 500 + the largest length difference among the
 * call's pairs, and the map is counted in the scored string's bases; the diagonal for an empty string, a failed Viterbi
 * call or a failed alignment), po_qual_batch of the tree model of `kind` (PO_KIND_POREOVER: PO_MODEL_CTC, PO_KIND_BONITO:
 * PO_MODEL_MERGE) and the Phred characters.  Between the upload of the signals and the download of the results only
 * per-read words (lengths, statuses, offsets) cross to the host.
 *   - band_size:     po_qual_batch's; <= 0: no band, no guide
 *   - qual_h:        the FASTQ characters 33 + Q, seq_len_h[i] of them at seq_off_h[i]
 *                    (Q = clip(floor(-10 log10(e) + 0.5), 0, 60), e = the alternatives' share of the odds, float64)
 *   - qual_status_h: int32[n_reads], po_qual_batch's status per read.  PO_E_ENVELOPE (the band admits no path) is reported,
 *                    not retried; a read with a non-zero status gets '!' (Q 0) for every base
 *   - odds_h (or NULL): the log-odds, five float64 per base at seq_off_h[i] * 5
 *   - guide_h (or NULL): the guide, int32 per frame at sig_off_h[i]; untouched for band_size <= 0
 *   - stage_ms_h (or NULL): float[8]: po_basecall_batch_h's six, [6] Viterbi map (beam) + alignment + guides,
 *                    [7] label compaction + lattice + Phred
 * A null qual_h or qual_status_h is PO_E_ARG naming it; every argument error is answered before the first allocation. */
int po_basecall_fastq_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                              const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                              const char* alphabet, int kind, int beam_width, int model, int max_windows_per_pass,
                              char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                              float* logits_h, int band_size, char* qual_h, int32_t* qual_status_h, double* odds_h,
                              int32_t* guide_h, float* stage_ms_h);

/* ---- `basecall` over one or several devices of a node -----------------------------------
 * A po_basecaller holds a model, the decoder's options and a list of devices.  A run cuts the reads, in input order, into
 * groups - contiguous runs of at most min(resident budget, ceil(total samples / (2 ndev))) samples, one read at least, a
 * longer read alone (po_basecall_group_plan, which touches no device) - and deals them from one planner to one host thread
 * per listed device, whichever is free.  Each worker keeps its state on its device - the weights, uploaded once by
 * po_basecaller_create, and every buffer, grow-only between groups and runs - and a stream of its own; a group runs the
 * body of po_basecall_batch_h / po_basecall_fastq_batch_h on it, so every string, logit and quality is what ONE such call
 * over all reads gives, bit for bit.  On the raw route the int16 samples go up and the f32 signal is made and read on the
 * device.
 *   - devices, ndev: 1 to 16 devices, each 0 .. po_device_count() - 1; a device may be named more than once (two workers
 *     then share it)
 *   - options: window, overlap, kind, beam_width, model, max_windows_per_pass as for po_basecall_batch_h; fastq != 0: the
 *     runs make qualities with band_size as po_basecall_fastq_batch_h; scaling (PO_SCALE_*), lo, hi: the raw route's
 *     preparation (po_signal_prep_h); resident_bytes: device bytes one group may hold per-sample state in (0: 16 GiB)
 *   - po_basecaller_create answers every argument error of po_basecall_batch_h / po_basecall_fastq_batch_h (by that
 *     entry, under its name) and of po_signal_prep_h's scaling and range, a device out of range and ndev outside 1 .. 16
 *     (PO_E_ARG naming the value); it returns NULL and po_last_error says why
 *   - po_basecaller_run_f32: scaled f32 signals; inputs and outputs laid out as po_basecall_fastq_batch_h's (qual_h and
 *     qual_status_h are read only by a fastq engine; no odds, guides or stage times)
 *   - po_basecaller_run_raw: raw int16 reads, raw_off_h from 0, offset_h / alpha_h for PO_SCALE_CURRENT.  kept_h[n] gets
 *     the samples each read kept; seq_off_h gives each read room for its RAW length; logits_h (or NULL) holds room for
 *     raw_off_h[n] rows, read i's kept_h[i] rows at row raw_off_h[i].  A read that keeps nothing gets length 0.
 *   - when a group fails the other workers finish what they hold and take no more; the run returns that group's code and
 *     "device d: <message>".  The engine stays usable.
 *   - po_basecaller_stats: reads, samples, groups and busy host milliseconds of worker i in the last run
 * The call precision (po_set_call_precision) and the recurrence precision (po_set_recur_precision) are read by every
 * group: set them around the whole run. */
typedef struct po_basecaller po_basecaller;
typedef struct po_basecaller_options {
    int window, overlap, kind, beam_width, model, max_windows_per_pass;
    int fastq, band_size;
    int scaling, lo, hi;
    int64_t resident_bytes;
} po_basecaller_options;
po_basecaller* po_basecaller_create(const int* devices, int ndev, const po_call_layer* layers_h, int n_layers,
                                    const float* weights_h, int64_t n_weights, const char* alphabet,
                                    const po_basecaller_options* options);
void po_basecaller_destroy(po_basecaller* b);
int po_basecaller_run_f32(po_basecaller* b, const float* signal_h, const int64_t* sig_off_h, int n_reads, char* seq_h,
                          const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h, float* logits_h, char* qual_h,
                          int32_t* qual_status_h);
int po_basecaller_run_raw(po_basecaller* b, const int16_t* raw_h, const int64_t* raw_off_h, int n_reads, const double* offset_h,
                          const double* alpha_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                          float* logits_h, char* qual_h, int32_t* qual_status_h, int64_t* kept_h);
int po_basecaller_stats(po_basecaller* b, int i, int64_t* reads, int64_t* samples, int* groups, double* busy_ms);
/* first[g], count[g] of the groups of n reads of len[i] samples (written for g < cap); returns the number of groups */
int po_basecall_group_plan(const int64_t* len, int n, int64_t group_samples, int ndev, int32_t* first, int32_t* count, int cap);
/* max(1, min(budget_samples, ceil(total / (2 ndev)))) */
int64_t po_basecall_group_samples(int64_t total, int64_t budget_samples, int ndev);

/* The three device stages of the above alone, on host buffers (tables from 0, non-decreasing; PO_E_ARG otherwise).  The
 * per-element rules are poreover_amd/csrc/po_fastq_rules.h.  mode (one int32 per read): 0 the scored string is the Viterbi
 * call (consumed[j] = j + 1), 1 consumed[] is given, 2 the diagonal floor((t + 1) * L / T).
 *   po_fastq_guide_h:    make_labeled_data.guide_from_alignment.  Read i has y_off_h[i+1] - y_off_h[i] frames; its map
 *                        (called_len_h[i] increasing frames), its consumed[] (mode 1) and its guide are at y_off_h[i];
 *                        label_len_h[i] = L.  consumed_h may be NULL when no read has mode 1.
 *   po_fastq_consumed_h: consumed_from_columns + the clip at L.  Pair i has ncol_h[i] columns at aln_off_h[i] of both rows
 *                        ('-' = gap); consumed of its called_len_h[i] bases goes to out_off_h[i]; mode_h[i] = 1, or 2 where
 *                        row 1 does not hold exactly called_len_h[i] bases.
 *   po_fastq_phred_h:    quality.phred + qual_string.  odds five float64 per base, labels and qual at label_off_h[i];
 *                        a read with qual_status_h[i] != 0 gets '!' throughout. */
int po_fastq_guide_h(const int32_t* map_h, const int32_t* consumed_h, const int64_t* y_off_h, int n, const int32_t* called_len_h,
                     const int32_t* label_len_h, const int32_t* mode_h, int32_t* guide_h);
int po_fastq_consumed_h(const char* aln1_h, const char* aln2_h, const int64_t* aln_off_h, const int32_t* ncol_h, int n,
                        const int32_t* called_len_h, const int32_t* label_len_h, const int64_t* out_off_h, int32_t* consumed_h,
                        int32_t* mode_h);
int po_fastq_phred_h(const double* odds_h, const char* labels_h, const int64_t* label_off_h, int n, const char* alphabet,
                     const int32_t* qual_status_h, char* qual_h);

/* ---- `pair-basecall`: scaled signals and a list of read pairs to 1D2 consensus strings in one device-resident pass
 *  -----------------------------------------------------------------------------------------------
 * po_basecall_batch_h's network part (the same windows, passes and stitched logits, bit for bit), then, on the same stream
 * and on the logits that are on the device already: the two pair-major float64 tables of po_pair_decode_batch (the
 * log-softmax of po_ingest_batch, PO_INGEST_LOGITS_F32; read 2 time-reversed with columns [3,2,1,0,4] where
 * reverse_complement is set) and po_pair_decode_batch itself.  Each read's signal goes up once, however many pairs name
 * it and on whichever side; the strings come down; nothing per frame returns to the host in between (unless logits_h asks).
 *   - signal_h, sig_off_h, n_reads, window, overlap, layers_h, n_layers, weights_h, n_weights, max_windows_per_pass:
 *                as for po_basecall_batch_h, with its refusals and messages (every read needs a sample, named or not)
 *   - pair_idx_h: int32[2 * n_pairs]; pair i = reads pair_idx_h[2i] (read 1) and pair_idx_h[2i + 1] (read 2).  An index
 *                outside [0, n_reads) is PO_E_ARG naming the pair; n_pairs < 0 is PO_E_ARG; n_pairs == 0 is PO_OK and
 *                writes no output
 *   - reverse_complement: 0 or 1 (transducer.reverse_complement of read 2, pair_decode.py:323-329)
 *   - opt:       as for po_pair_decode_batch; model PO_MODEL_CTC or PO_MODEL_MERGE.  PO_MODEL_FLIPFLOP is PO_E_UNSUPPORTED
 *                (the network emits a CTC table, blank last); beam_width outside 1..25 and an unknown method are PO_E_ARG
 *   - seq1d_h, seq1d_off_h (2 n_pairs + 1 entries, from 0), len1_h, len2_h, identity_h, seq_h, seq_off_h (from 0),
 *                seq_len_h, status_h: as po_pair_decode_batch_h writes them, PO_SKIP_LENGTH / PO_SKIP_IDENTITY included.
 *                A read's room in seq1d must be at least its number of samples, and seq_off_h must not decrease
 *                (PO_E_CAP naming the pair otherwise); a consensus longer than its room is that pair's PO_E_CAP status
 *   - logits_h (or NULL): the stitched Dense outputs, (sig_off_h[n_reads], 5) f32, read after read
 *   - stage_ms_h (or NULL): float[6] device milliseconds, SET by the call: [0..3] po_call_batch's stages summed over the
 *                passes, [4] window gather + stitch + pair tables, [5] po_pair_decode_batch as a whole
 * Every argument error is answered before the first device allocation.  One device, one stream, synchronous. */
int po_pair_basecall_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                             const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                             int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                             const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                             int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                             int32_t* seq_len_h, int32_t* status_h, float* logits_h, float* stage_ms_h);
/* The same with --skip_matches: the pair chain is po_pair_skip_plan + po_pair_skip_run (above) on the tables the network left on
 * the device; status_h may also be PO_E_NO_ANCHOR, PO_E_BOX or a box's beam status.  opt->diagonal_envelope: PO_E_UNSUPPORTED. */
int po_pair_basecall_skip_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                  const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                  int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                                  const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                                  int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                                  int32_t* seq_len_h, int32_t* status_h, float* logits_h, float* stage_ms_h, int skip_threshold,
                                  int indel_threshold);

/* The table stage of the above alone, on host buffers.  logits_h: (row_off_h[n_reads], 5) f32, read-major; row_off_h from
 * 0, non-decreasing; a read that a pair names needs a row (PO_E_ARG naming the pair).  y1_h / y2_h get, pair after pair, the
 * rows of each pair's first / second read: x - logsumexp(x) per row in float32, widened (po_ingest_batch's bits); table 2
 * time-reversed inside each pair where reverse2 is set, its columns through perm2_h (5 ints or NULL: out[:, c] =
 * value[:, perm2_h[c]]).  The caller sizes y1_h / y2_h: 5 float64 per row of the pairs' first / second reads. */
int po_pair_tables_h(const float* logits_h, const int64_t* row_off_h, int n_reads, const int32_t* pair_idx_h, int n_pairs,
                     int reverse2, const int* perm2_h, double* y1_h, double* y2_h);

/* ---- the pair pass with per-base qualities ----------------------------------------------------
 * po_pair_basecall_batch_h's arguments, refusals, strings, lengths, identities and statuses (bit for bit), then, behind the
 * pair chain on the same stream and on the tables and strings that are on the device already, what `pair-decode --fastq`
 * computes (pair_decode._attach_fastq).  Every pair whose status is 0 has four scored items, k = 0 .. 3: seq1 on table 1,
 * seq2 on table 2 (as the pair decoder saw it: time-reversed and complemented where reverse_complement is set), the
 * consensus on table 1, the consensus on table 2; the items of any other pair are empty (with opt->diagonal_envelope a
 * pair has no 1-D calls: items 0 and 1 are empty).  Per item: the Viterbi call of its table with its frame map (a second,
 * cheap po_viterbi_batch per side), the band guide by quality.call_guides' rule (the map where the scored string is that
 * call; otherwise the two are aligned by po_align_batch, band_width = 500 + the largest length difference among ALL
 * aligned items of the call, both sides together, and the map is counted in the scored string's bases; the diagonal for
 * an empty string, a failed Viterbi call or a failed alignment), po_qual_batch of opt->model (four calls of n_pairs reads,
 * one workspace) and the Phred characters: a 1-D item's own; the consensus from the element-wise sum of its two tables'
 * odds (quality.combine), or from one table's odds alone where the other item's status is not 0.
 *   - band_size:     po_qual_batch's; <= 0: no band, no guides
 *   - unbanded_h (or NULL): int32[4 n_pairs], item k of pair i at 4 i + k; a non-zero entry scores that item without a
 *                    band while the others keep theirs (the retry of a lost lattice; the consensus then mixes a banded
 *                    and an unbanded table)
 *   - qual1d_h:      the 1-D FASTQ characters 33 + Q, len1_h[i] / len2_h[i] of them at seq1d_off_h[2i] / [2i + 1]
 *   - qual_h:        the consensus characters, seq_len_h[i] of them at seq_off_h[i]; a pair that is not decoded gets none
 *                    (the rest of both buffers is zero)
 *   - qual_status_h: int32[4 n_pairs], po_qual_batch's status of item k of pair i at 4 i + k, 0 for an empty item.
 *                    PO_E_ENVELOPE (the band admits no path) is reported, not retried; an item with a non-zero status is '!'
 *                    (Q 0) throughout, and the consensus is '!' throughout where both of its items have one
 *   - odds1d_h (or NULL): the 1-D items' log-odds, five float64 per base at seq1d_off_h[2i + side] * 5
 *   - odds_cons_h (or NULL): the consensus items' log-odds, [2][5 * seq_off_h[n_pairs]]: table 1's at seq_off_h[i] * 5,
 *                    table 2's 5 * seq_off_h[n_pairs] values further on
 *   - guide_h (or NULL): the guides, int32[2 * (rows1 + rows2)] (rows = a table's frames): the four item types one behind
 *                    the other (rows1, rows2, rows1, rows2 values), pair i of a type at its table's row offset; untouched
 *                    for band_size <= 0
 *   - stage_ms_h (or NULL): float[8]: po_pair_basecall_batch_h's six, [6] second Viterbi + alignment + guides,
 *                    [7] label compaction + lattices + Phred
 * A null qual1d_h, qual_h or qual_status_h is PO_E_ARG naming it; every argument error is answered before the first
 * allocation. */
int po_pair_basecall_fastq_batch_h(const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                                   const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                                   int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                                   const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                                   int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h,
                                   int32_t* seq_len_h, int32_t* status_h, float* logits_h, int band_size,
                                   const int32_t* unbanded_h, char* qual1d_h, char* qual_h, int32_t* qual_status_h,
                                   double* odds1d_h, double* odds_cons_h, int32_t* guide_h, float* stage_ms_h);

/* The quality stages of the above alone, on host buffers: what the fused entry runs behind the pair chain.  y1_h / y2_h
 * with y1_off_h / y2_off_h: the two pair-major float64 tables (po_pair_tables_h's, 5 columns); model PO_MODEL_CTC or
 * PO_MODEL_MERGE (PO_MODEL_FLIPFLOP: PO_E_UNSUPPORTED); seq1d_h .. status_h: a pair decode's outputs, read (every table
 * from 0, non-decreasing: PO_E_ARG; a decoded pair's string longer than its room: PO_E_CAP naming the pair).  The outputs
 * as above. */
int po_pair_qual_h(const double* y1_h, const int64_t* y1_off_h, const double* y2_h, const int64_t* y2_off_h, int n, int model,
                   const char* seq1d_h, const int64_t* seq1d_off_h, const int32_t* len1_h, const int32_t* len2_h,
                   const char* seq_h, const int64_t* seq_off_h, const int32_t* seq_len_h, const int32_t* status_h,
                   int band_size, const int32_t* unbanded_h, char* qual1d_h, char* qual_h, int32_t* qual_status_h,
                   double* odds1d_h, double* odds_cons_h, int32_t* guide_h);

/* ---- the quality stages on tables that are on the device already --------------------------------
 * For a caller whose float64 tables and decoded strings are device buffers (poreover_amd.tensors): nothing is uploaded but
 * the stages' small plan tables, and every output is a device buffer of the caller's, written on `stream`.  Both entries
 * run the stage bodies of their host-buffer twins (the same launchers, the same kernels, the same bits).
 *   - They are NOT enqueue-only: like po_qual_batch they read the offset tables and the per-read lengths (po_pair_qual:
 *     the statuses too) back to the host, where the lattices' and the aligner's plans are made, and they return after
 *     a last synchronise of `stream`.
 *   - The stages' intermediate buffers (frame maps, guides, consumed counts, the aligner's rows, labels, lattice rows) are
 *     allocated with hipMalloc for the length of the call and freed when it returns: not from the caller's allocator, the
 *     one departure from the rule of the other device-pointer entries.  (A workspace-query form is not offered yet.)
 *   - PO_MODEL_FLIPFLOP (po_fastq_tables: PO_KIND_FLIPFLOP too) is PO_E_UNSUPPORTED.  Every argument error that can be
 *     told without the device is answered before anything is read back, and every one before the first allocation,
 *     with the entry's name in the text.
 *
 * po_fastq_tables: steps (1) to (6) of po_basecall_fastq_batch_h's quality stages on the table y / y_off (C must be 5;
 * y_off from 0) and the strings seq at seq_off (from 0; a read's room must hold a base per frame and its string, PO_E_CAP
 * naming the read) with their lengths seq_len and the decode's status.
 *   - model, kind:   PO_MODEL_CTC with PO_KIND_POREOVER or PO_MODEL_MERGE with PO_KIND_BONITO (any other combination:
 *                    PO_E_ARG); kind selects the Viterbi call that makes the frame map
 *   - scored_is_viterbi: 1: seq / seq_len / status are po_viterbi_batch's of `kind` WITH its frame map, passed as `map`
 *                    (int32 per frame at y_off): no second Viterbi call, no alignment.  0: the strings are something else (a
 *                    beam search's); map is not read; a second Viterbi call with its map, then the mode, gather, align and
 *                    consumed stages, as po_basecall_fastq_batch_h runs them behind its beam search
 *   - band_size:     po_qual_batch's; <= 0: no band, no guide
 *   - unbanded_h (or NULL): HOST int32[n]; with a band, a non-zero entry scores that read without one while the others
 *                    keep theirs (the retry of a lost lattice).  A flagged read has L = 0 in the banded po_qual_batch call
 *                    and is scored by a second call without a band
 *   - qual:          the FASTQ characters 33 + Q, seq_len[i] of them at seq_off[i]; other bytes are left as they are
 *   - qual_status:   int32[n], po_qual_batch's status per read (a flagged read: the unbanded call's); PO_E_ENVELOPE is
 *                    reported, not retried; a read with a non-zero status gets '!' throughout
 *   - odds (or NULL): the log-odds, five float64 per base, DENSE: read i's rows start at the sum of max(seq_len, 0) of the
 *                    unflagged reads before it; the flagged reads' rows follow behind all of those, in read order
 *   - guide (or NULL): the guide, int32 per frame at y_off[i]; untouched for band_size <= 0 */
int po_fastq_tables(const double* y, const int64_t* y_off, int n, int C, int model, int kind, const char* seq,
                    const int64_t* seq_off, const int32_t* seq_len, const int32_t* status, const int32_t* map,
                    int scored_is_viterbi, int band_size, const int32_t* unbanded_h, char* qual, int32_t* qual_status,
                    double* odds, int32_t* guide, void* stream);

/* po_pair_qual: po_pair_qual_h with every _h buffer a device buffer, except unbanded_h, which stays on the host.  The four
 * items per pair, the layouts of qual1d, qual, qual_status[4 n], odds1d, odds_cons and guide, the refusals (after the
 * tables have been read back) and the bits are po_pair_qual_h's.  qual1d (seq1d_off[2 n] bytes) and qual (seq_off[n] bytes)
 * are overwritten WHOLE, with zeros outside the strings (as po_pair_qual_h's host buffers are).  The odds come with one small
 * copy per item. */
int po_pair_qual(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int model,
                 const char* seq1d, const int64_t* seq1d_off, const int32_t* len1, const int32_t* len2, const char* seq,
                 const int64_t* seq_off, const int32_t* seq_len, const int32_t* status, int band_size,
                 const int32_t* unbanded_h, char* qual1d, char* qual, int32_t* qual_status, double* odds1d, double* odds_cons,
                 int32_t* guide, void* stream);

/* ---- `pair-basecall` over one or several devices of a node ----------------------------------
 * A po_pair_basecaller holds a model, the pair decoder's options and a list of devices, as a po_basecaller does for
 * `basecall`.  A run cuts the pairs, in input order, into groups (po_pair_basecall_group_plan, which touches no device) and
 * deals them from one planner to one host thread per listed device, whichever is free.  A group's distinct reads are
 * compacted and indexed locally; a read that pairs of two groups name runs in each.  Each worker keeps its state on its
 * device - the weights, uploaded once by po_pair_basecaller_create, and every buffer, grow-only between groups and runs -
 * and a stream of its own; a group runs the body of po_pair_basecall_batch_h / po_pair_basecall_fastq_batch_h on it, so
 * every string, identity, status, logit and quality is what ONE such call over all pairs gives, bit for bit.  The
 * --skip_matches chain is not carried: it stays on po_pair_basecall_skip_batch_h.
 *   - devices, ndev: 1 to 16 devices, each 0 .. po_device_count() - 1; a device may be named more than once
 *   - options: window, overlap, max_windows_per_pass, reverse_complement and pair as for po_pair_basecall_batch_h; fastq != 0:
 *     the runs make qualities with band_size as po_pair_basecall_fastq_batch_h; scaling (PO_SCALE_*), lo, hi: the raw route's
 *     preparation (po_signal_prep_h); resident_bytes: the device bytes one group may hold (0: 16 GiB)
 *   - groups: a pair joins the run while the run's resident bytes with it - 24 per sample of its distinct reads, 40 per
 *     frame of every pair side, po_pair_decode_workspace_bytes and, for a fastq engine, the quality stages' bytes - stay
 *     within resident_bytes and, with ndev > 1, its pair-side frames within ceil(all pair-side frames / (2 ndev)); a pair
 *     that does not fit alone goes alone.  The raw route plans on raw lengths.
 *   - po_pair_basecaller_create answers every argument error of po_pair_basecall_batch_h / po_pair_basecall_fastq_batch_h
 *     (by that entry, under its name) and of po_signal_prep_h's scaling and range, a device out of range and ndev outside
 *     1 .. 16 (PO_E_ARG naming the value); it returns NULL and po_last_error says why
 *   - po_pair_basecaller_run_f32: scaled f32 signals and index pairs; outputs laid out as po_pair_basecall_fastq_batch_h's
 *     (unbanded_h, qual1d_h, qual_h and qual_status_h are read only by a fastq engine; no odds, guides or stage times;
 *     logits_h or NULL: a read no pair names gets no logits).  Only the reads that pairs name need a sample.
 *   - po_pair_basecaller_run_raw: raw int16 reads, raw_off_h from 0, offset_h / alpha_h for PO_SCALE_CURRENT.  kept_h[n_reads]
 *     gets the samples each read kept (-1: no pair names it, it was not prepared); the rooms of seq1d_off_h are for the RAW
 *     lengths; logits_h (or NULL) holds room for raw_off_h[n_reads] rows, read i's kept_h[i] rows at row raw_off_h[i].  A
 *     pair that names a read which keeps nothing is not run: its status is PO_E_ARG, its lengths are 0; its neighbours
 *     are not affected.
 *   - per-pair statuses (PO_SKIP_*, PO_E_NOMEM, ...) come back as from the one-call entry and do not fail the run.  When a
 *     group fails as a call the other workers finish what they hold and take no more; the run returns that group's code
 *     and "device d: <message>".  The engine stays usable.
 *   - po_pair_basecaller_stats: pairs, reads (distinct per group, summed), their samples, groups and busy host
 *     milliseconds of worker i in the last run
 * The call precision (po_set_call_precision) and the recurrence precision (po_set_recur_precision) are read by every
 * group: set them around the whole run. */
typedef struct po_pair_basecaller po_pair_basecaller;
typedef struct po_pair_basecaller_options {
    int window, overlap, max_windows_per_pass, reverse_complement;
    po_pair_options pair;
    int fastq, band_size;
    int scaling, lo, hi;
    int64_t resident_bytes;
} po_pair_basecaller_options;
po_pair_basecaller* po_pair_basecaller_create(const int* devices, int ndev, const po_call_layer* layers_h, int n_layers,
                                              const float* weights_h, int64_t n_weights,
                                              const po_pair_basecaller_options* options);
void po_pair_basecaller_destroy(po_pair_basecaller* b);
int po_pair_basecaller_run_f32(po_pair_basecaller* b, const float* signal_h, const int64_t* sig_off_h, int n_reads,
                               const int32_t* pair_idx_h, int n_pairs, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h,
                               int32_t* len2_h, double* identity_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h,
                               int32_t* status_h, float* logits_h, const int32_t* unbanded_h, char* qual1d_h, char* qual_h,
                               int32_t* qual_status_h);
int po_pair_basecaller_run_raw(po_pair_basecaller* b, const int16_t* raw_h, const int64_t* raw_off_h, int n_reads,
                               const double* offset_h, const double* alpha_h, const int32_t* pair_idx_h, int n_pairs,
                               char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h, double* identity_h,
                               char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h, float* logits_h,
                               const int32_t* unbanded_h, char* qual1d_h, char* qual_h, int32_t* qual_status_h, int64_t* kept_h);
int po_pair_basecaller_stats(po_pair_basecaller* b, int i, int64_t* pairs, int64_t* reads, int64_t* samples, int* groups,
                             double* busy_ms);
/* first[g], count[g] of the groups of n_pairs pairs over reads of len[r] samples (written for g < cap); band_size: the
 * quality lattice's band the groups are sized for (fastq != 0; <= 0: no band); resident_bytes 0: 16 GiB.  Returns the
 * number of groups, or PO_E_ARG. */
int po_pair_basecall_group_plan(const int64_t* len, int n_reads, const int32_t* pair_idx, int n_pairs, const po_pair_options* opt,
                                int fastq, int band_size, int64_t resident_bytes, int ndev, int32_t* first, int32_t* count, int cap);

/* The consensus Phred kernel alone (poreover_amd/csrc/po_fastq_rules.h: po_fq_pair_phred).  odds1_h / odds2_h: five
 * float64 per base, labels and qual at label_off_h[i] (from 0, non-decreasing); item i gets quality.phred of
 * quality.combine(odds1, odds2) where st1_h[i] and st2_h[i] are 0, of one table alone where only its status is 0, '!'
 * throughout where neither is. */
int po_fastq_pair_phred_h(const double* odds1_h, const double* odds2_h, const char* labels_h, const int64_t* label_off_h, int n,
                          const char* alphabet, const int32_t* st1_h, const int32_t* st2_h, char* qual_h);

/* ---- CTC training of the basecalling network (`train`) -------------------------------------------
 * Replaces the reference's TensorFlow training step (train_ctc_model, network.py:78-131): the forward pass above,
 * tf.compat.v1.nn.ctc_loss (blank = class 4, softmax inside the loss) averaged over the batch, its gradient and Keras
 * Adam.  A trainer holds the model (layers_h as for po_call_batch), its f32 parameters, their gradient and Adam's m, v
 * on the current device, all in po_call_batch's flat weight layout, and workspace for max_batch windows of T samples.
 *   - po_train_create returns NULL on an unusable model or a failed allocation (po_last_error says which)
 *   - po_train_set_params loads n = the model's weight count parameters and resets Adam (m = v = 0, step 0);
 *     po_train_get_params copies them back
 *   - po_train_step runs one step on n (1 .. max_batch) windows: signal_h n * T f32 samples, labels_h the windows'
 *     labels back to back (0..3 = A C G T), label_len_h[n] their lengths.  merge_repeated 0: the reference's default
 *     lattice (ctc_merge_repeated = False: repeated labels are separate emissions, no blank needed between them); 1:
 *     standard CTC.  A label must fit the window: L <= T (merge off), L + the number of adjacent equal labels <= T (on);
 *     labels outside 0..3 and labels that do not fit are PO_E_ARG naming the window.  Writes loss_h[n] (-log P(label |
 *     window) per window), grad_h (or NULL: the gradient of the batch-mean loss, flat layout).  update = 1 then applies
 *     Adam: m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); p -= lr sqrt(1 - beta2^t) / (1 - beta1^t) m / (sqrt(v) + eps)
 *     with t the trainer's step count after the increment; update = 0 leaves the parameters and Adam as they are.
 *   - stage_ms_h (or NULL): HOST float[5] set to device milliseconds per stage, by events: 0 forward, 1 CTC loss and
 *     gradient, 2 GRU backward recurrences, 3 weight and input gradients (GEMMs, bias sums, Dense / Conv1D backward), 4 Adam
 *   - po_train_last copies the last step's logits (the Dense outputs, as po_call_batch's) and/or the gradient of the
 *     batch-mean loss with respect to them (n * T * 5 f32 each, NULL skips) of its first n windows
 * A step is synchronous, and its gradient is the same bits on every run (no float atomics). */
typedef struct po_trainer po_trainer;
po_trainer* po_train_create(const po_call_layer* layers_h, int n_layers, int max_batch, int T);
void po_train_destroy(po_trainer* tr);
int po_train_set_params(po_trainer* tr, const float* w_h, int64_t n);
int po_train_get_params(po_trainer* tr, float* w_h, int64_t n);
int po_train_step(po_trainer* tr, const float* signal_h, int n, const int32_t* labels_h, const int32_t* label_len_h,
                  int merge_repeated, float lr, float beta1, float beta2, float eps, int update, float* loss_h,
                  float* grad_h, float* stage_ms_h);
int po_train_last(po_trainer* tr, int n, float* logits_h, float* dlogits_h);

/* Held-out validation on the trainer's resident parameters (train.validation_error's argmax path and edit distance,
 * DESIGN.md §11.1; the rules are poreover_amd/csrc/po_eval_rules.h).
 *   - po_train_eval takes n (1 .. max_batch) windows and their labels as po_train_step does, with the same checks,
 *     answered before any launch (PO_E_ARG naming the window).  On the trainer's stream it runs the forward pass; with
 *     loss_h given, the CTC lattice of merge_repeated, loss_h[n] = -log P(label | window), bit for bit what
 *     po_train_step(update = 0) writes; the path of every window (per frame np.argmax's class over the 5 probabilities:
 *     the first NaN, else the first maximum; classes 0..3 kept in frame order, class 4 dropped, repeats kept, whatever
 *     merge_repeated is); and the unit-cost edit distance of each path to its labels.  Writes edit_h[n], pred_len_h[n]
 *     (the paths' lengths), status_h[n] (0, or PO_E_CAP with edit -1 where both the path and the label are longer than
 *     PO_EDIT_MAX_SHORT = 4095: the other windows are still answered), pred_h (or NULL: n * T codes 0..3, window w's
 *     path at w * T, the rest of its T bytes unspecified).  No gradient, no Adam: parameters, m, v and the step count
 *     are untouched.  po_train_last afterwards describes this call's logits (its dlogits are an earlier step's).
 *   - stage_ms_h (or NULL): HOST float[3] set to device milliseconds by events: 0 forward, 1 CTC loss (0 without
 *     loss_h), 2 path and edit distance
 *   - po_eval_path_h: the path stage alone on host buffers: probs_h n * T * 5 f32, pred_h n * T codes, pred_len_h[n]
 *   - po_edit_distance_batch_h: the edit distance stage alone: pair i is a_h[a_off_h[i] .. a_off_h[i+1]) against
 *     b_h[b_off_h[i] .. b_off_h[i+1]) (bytes compared for equality; tables non-decreasing, their first entry need not
 *     be 0).  dist_h[n], status_h[n]: 0, or PO_E_CAP with dist -1 where min(la, lb) > 4095; the batch goes on.
 * All three are synchronous; the same inputs give the same bits at every batch position and on every run. */
int po_edit_distance_batch_h(const uint8_t* a_h, const int64_t* a_off_h, const uint8_t* b_h, const int64_t* b_off_h,
                             int n, int32_t* dist_h, int32_t* status_h);
int po_eval_path_h(const float* probs_h, int n, int T, uint8_t* pred_h, int32_t* pred_len_h);
int po_train_eval(po_trainer* tr, const float* signal_h, int n, const int32_t* labels_h, const int32_t* label_len_h,
                  int merge_repeated, float* loss_h, int32_t* edit_h, int32_t* pred_len_h, int32_t* status_h,
                  uint8_t* pred_h, float* stage_ms_h);

/* The precision of a trainer's GRU weight and input GEMMs: a property of the trainer, not of the process
 * (po_set_call_precision does not reach it, and it does not reach po_call_batch).
 *   PO_CALL_F32   (default) every product in f32
 *   PO_CALL_BF16  four products of every GRU layer take both operands rounded to bf16 (round to nearest even,
 *                 csrc/po_bf16_rules.h), with f32 products and sums on v_mfma_f32_16x16x32_bf16: the forward projection
 *                 P = x·W + b_in (po_call_batch's kernels under PO_CALL_BF16: the training logits are its bits), dW = X^T·dA,
 *                 dU = H_prev^T·dR and dX = sum_d dA_d·W_d^T.  Both recurrences (h·U, dR·U^T), the gates, the bias gradients
 *                 (sums of the unrounded dA and dR), Conv1D, Dense, CTC, Adam, the parameters, the gradient and Adam's m and v
 *                 stay f32.  No loss scaling: bf16 has f32's exponent range.  po_train_eval runs the trainer's forward pass
 *                 and so follows its mode.  The bf16 copies of a layer's W live in a workspace the trainer allocates when
 *                 the mode is first set.  A step stays the same bits on every run.
 * Every refusal leaves the trainer in the mode it was in and allocates nothing: another value is PO_E_ARG; a trainer whose
 * GRU layers are not 128 units is PO_E_UNSUPPORTED (the bf16 kernels are built for 128 units), naming bf16 and the width; a
 * null trainer is PO_E_ARG.  Switching keeps the parameters and Adam's state; back under PO_CALL_F32 a step is the f32
 * step's bits.  po_train_get_precision returns the mode. */
int po_train_set_precision(po_trainer* tr, int precision);
int po_train_get_precision(const po_trainer* tr);
/* The two GEMM stages alone for a 128-unit layer, on host buffers, by the kernels of `precision` (explicit: no selector is
 * read).  po_gru_wgrad_h: out_h[K][384] = sum_m a_h[m][k] · d_h[m][c] over M rows (a_h: rows lda >= K floats apart, d_h
 * [M][384]), split over M and combined as po_train_step does.  po_gru_dx_h: dX_h[M][cin] = sum_d dA_h[d][M][384] · w_h[d][cin][384]^T,
 * the directions in order.  M >= 0 (0: PO_OK, nothing written), K and cin >= 1, ndir 1 or 2; a null pointer, another value
 * or another precision is PO_E_ARG naming the argument, before any allocation. */
int po_gru_wgrad_h(const float* a_h, int64_t lda, int64_t M, int K, const float* d_h, int precision, float* out_h);
int po_gru_dx_h(const float* dA_h, int64_t M, int ndir, const float* w_h, int cin, int precision, float* dX_h);

/* The recipe around a step (the rules are poreover_amd/csrc/po_train_recipe_rules.h): gradient accumulation
 * over micro-batches, clipping by the global norm with a guard against non-finite gradients, AdamW, and Adam's state in and
 * out.  The accumulator (one more vector of the model's size, flat layout) is allocated at its first use; po_train_step and
 * po_train_eval never touch it.
 *   - po_train_accumulate runs po_train_step's checks (the same messages under its own name), forward pass, CTC and backward
 *     pass on n (1 .. max_batch) windows in the trainer's precision mode: update = 0's gradient g of the micro-batch's mean
 *     loss.  The accumulator becomes weight * g where it was empty (weight 1: g's bits), else fmaf(weight, g, accumulator).
 *     With weight n / N over micro-batches of N windows in all, the sum is the gradient of the mean loss over the N windows.
 *     loss_h[n] and stage_ms_h (float[5], slot 4: the accumulation) as in a step.  A weight that is not finite is PO_E_ARG.
 *   - po_train_accum_reset marks the accumulator empty: the next contribution overwrites.  po_train_get_accum copies it out
 *     (PO_E_ARG where it is empty); po_train_set_accum loads one and counts as one contribution.  n = the weight count.
 *   - po_train_apply: norm = the L2 norm of the whole accumulator, summed in f64 in a fixed partition (the same bits every
 *     run), written to *grad_norm_h (before clipping; NULL skips).  scale = clip_norm / norm where clip_norm > 0 and norm >
 *     clip_norm, else 1 (tf.clip_by_global_norm; clip_norm 0: no clipping).  Where the norm is finite: ge = scale * g, m and v
 *     as in a step, p -= lr_t m / (sqrt(v) + eps) + lr weight_decay p (decoupled decay at the rate lr, not the bias-corrected
 *     lr_t; weight_decay 0: none), Adam's t advances, *applied_h = 1 (NULL skips).  With scale 1 and no decay these are
 *     po_train_step(update = 1)'s bits.  Where it is NaN or infinite: *applied_h = 0 and p, m, v and t keep their bits.  Either
 *     way the accumulator is empty afterwards.  PO_E_ARG naming the argument, before any launch: a negative or non-finite
 *     clip_norm or weight_decay, an empty accumulator, a null trainer.
 *   - po_train_get_state / po_train_set_state: Adam's m and v (n = the weight count each) and its step count t (>= 0); with
 *     po_train_get_params / po_train_set_params (which resets Adam and empties the accumulator: call it first) a run continues
 *     in another trainer bit for bit.
 *   - po_grad_norm_h: the norm stage alone on a host buffer of n >= 0 floats (n = 0: 0).
 * All are synchronous. */
int po_train_accumulate(po_trainer* tr, const float* signal_h, int n, const int32_t* labels_h, const int32_t* label_len_h,
                        int merge_repeated, float weight, float* loss_h, float* stage_ms_h);
int po_train_accum_reset(po_trainer* tr);
int po_train_get_accum(po_trainer* tr, float* g_h, int64_t n);
int po_train_set_accum(po_trainer* tr, const float* g_h, int64_t n);
int po_train_apply(po_trainer* tr, float lr, float beta1, float beta2, float eps, float weight_decay, float clip_norm,
                   double* grad_norm_h, int* applied_h);
int po_train_get_state(po_trainer* tr, float* m_h, float* v_h, int64_t n, int64_t* step_h);
int po_train_set_state(po_trainer* tr, const float* m_h, const float* v_h, int64_t n, int64_t step);
int po_grad_norm_h(const float* g_h, int64_t n, double* norm_h);

/* Data-parallel training over several devices (the rules are poreover_amd/csrc/po_train_dp_rules.h).  A group
 * is n_replicas (1 .. 16) trainers, replica r on device devices_h[r]; a device may appear more than once.  One host thread per
 * replica, made at create and joined at destroy, binds its device once and runs that replica's work; the calling thread's
 * current device is never changed.  A replica's error comes back in po_last_error as "replica r (device d): <its message>".
 * Every argument error is answered before the first allocation or launch: a null pointer, a replica count outside 1 .. 16, a
 * device outside 0 .. po_device_count() - 1, a share outside 0 .. max_batch, no share at all, a weight that is not finite.
 *   - po_train_group_create: po_train_create's arguments and the devices; NULL on failure (po_last_error says why).
 *     po_train_group_size returns the replica count.
 *   - po_train_group_set_params / po_train_group_set_state: po_train_set_params / po_train_set_state on every replica (the
 *     same host bits to each).  po_train_group_get_params / po_train_group_get_state read replica 0;
 *     po_train_group_get_replica_params / po_train_group_get_replica_state read the named replica (the replicas hold the same
 *     bits after every call below; these are for checking that).  po_train_group_set_precision: po_train_set_precision on every
 *     replica, or on none where it is refused.
 *   - po_train_group_accumulate: n_h[r] (0: idle) windows for replica r.  The shares lie one after another, replica 0's first,
 *     in signal_h (T samples a window), label_len_h, labels_h and loss_h; weight_h[r] is replica r's weight; stage_ms_h (or
 *     NULL) float[n_replicas][5].  Every replica's share passes po_train_accumulate's checks (its messages) before any replica
 *     launches: a refused share refuses the call and no accumulator changes.  Then the replicas run po_train_accumulate on
 *     their shares at the same time.
 *   - po_train_group_reduce: the all-reduce alone.  Every replica's accumulator becomes ((ga_r0 + ga_r1) + ga_r2) + ... in
 *     plain f32 over the replicas whose accumulator is not empty, in ascending replica order (an empty one is skipped, not
 *     added as zero; all empty: PO_E_ARG), the same bits on every replica and in every run, and counts as one contribution.
 *     Replica r sums slice r (po_train_dp_rules.h) of every contributing accumulator into a staging vector on its device, and
 *     after a hand-off between launches every replica copies each slice from its owner.  *ms_h (or NULL): the milliseconds
 *     between events on replica 0's stream around its part.  A group of one has nothing to sum and launches nothing.
 *   - po_train_group_apply: the all-reduce, then po_train_apply on every replica's copy; *grad_norm_h and *applied_h are
 *     replica 0's (every replica's are the same bits).  The accumulators are empty afterwards.
 *   - po_train_group_get_accum / po_train_group_set_accum: po_train_get_accum / po_train_set_accum of one replica (before or
 *     after a reduce; set is how a test plants a value in one replica's share).
 *   - po_train_group_eval: po_train_eval with n_h[n_replicas] shares laid out as for po_train_group_accumulate (pred_h: T
 *     codes of room a window; stage_ms_h float[n_replicas][3]); the replicas evaluate their shares at the same time.
 *   - po_set_dp_route: how the slices travel, process-wide like po_set_chain_mode and read by every reduce.
 *     PO_DP_ROUTE_PEER: the kernels read the peers' device memory (peer access is enabled once at create; replicas on one
 *     device need none); where a pair of the group's devices has no peer access the reduce is PO_E_UNSUPPORTED naming the two
 *     devices, before any launch.  PO_DP_ROUTE_HOST: through pinned host buffers with hipMemcpyAsync, summed by the same
 *     kernel in the same order: the same bits.  PO_DP_ROUTE_AUTO (default): PEER where every pair can, else HOST.  Another
 *     value is PO_E_ARG and leaves the route as it was.
 *   - po_dp_allreduce_h: the reduce stage alone on host buffers: bufs_h[r] (n floats; may be NULL where present_h[r] is 0) is
 *     uploaded to a buffer on devices_h[r], the reduce runs on the current route, out_h[r] (n floats, every r) gets replica r's
 *     result.  n = 0 is PO_OK with nothing written; no replica present is PO_E_ARG.
 * All are synchronous. */
#define PO_DP_ROUTE_AUTO 0
#define PO_DP_ROUTE_PEER 1
#define PO_DP_ROUTE_HOST 2
typedef struct po_train_group po_train_group;
po_train_group* po_train_group_create(const po_call_layer* layers_h, int n_layers, int max_batch, int T, const int* devices_h,
                                      int n_replicas);
void po_train_group_destroy(po_train_group* g);
int po_train_group_size(po_train_group* g);
int po_train_group_set_params(po_train_group* g, const float* w_h, int64_t n);
int po_train_group_get_params(po_train_group* g, float* w_h, int64_t n);
int po_train_group_get_replica_params(po_train_group* g, int replica, float* w_h, int64_t n);
int po_train_group_set_state(po_train_group* g, const float* m_h, const float* v_h, int64_t n, int64_t step);
int po_train_group_get_state(po_train_group* g, float* m_h, float* v_h, int64_t n, int64_t* step_h);
int po_train_group_get_replica_state(po_train_group* g, int replica, float* m_h, float* v_h, int64_t n, int64_t* step_h);
int po_train_group_set_precision(po_train_group* g, int precision);
int po_train_group_accumulate(po_train_group* g, const float* signal_h, const int* n_h, const int32_t* labels_h,
                              const int32_t* label_len_h, int merge_repeated, const float* weight_h, float* loss_h,
                              float* stage_ms_h);
int po_train_group_get_accum(po_train_group* g, int replica, float* g_h, int64_t n);
int po_train_group_set_accum(po_train_group* g, int replica, const float* g_h, int64_t n);
int po_train_group_reduce(po_train_group* g, float* ms_h);
int po_train_group_apply(po_train_group* g, float lr, float beta1, float beta2, float eps, float weight_decay, float clip_norm,
                         double* grad_norm_h, int* applied_h);
int po_train_group_eval(po_train_group* g, const float* signal_h, const int* n_h, const int32_t* labels_h,
                        const int32_t* label_len_h, int merge_repeated, float* loss_h, int32_t* edit_h, int32_t* pred_len_h,
                        int32_t* status_h, uint8_t* pred_h, float* stage_ms_h);
int po_set_dp_route(int route);
int po_get_dp_route(void);
int po_dp_allreduce_h(const int* devices_h, int R, const float* const* bufs_h, const int* present_h, int64_t n,
                      float* const* out_h);

/* ---- read-to-genome mapping for `benchmark` (replaces mappy.Aligner as benchmark.py:16-20 uses it) ----
 * minimap2's map-ont seeds (k = 15, w = 10, its hash64) and scores reduced to a fixed integer specification: one
 * primary hit per read, a local affine alignment in a 512-column band around the best chain.  Sequences are upper-case
 * ASCII; any byte but A C G T is "not a base" (no k-mer covers it; it scores -1 against anything).  All calls are
 * synchronous and use the current device.
 *   - po_map_sketch_h: the minimizers of n sequences (seq_h back to back, off_h int64[n+1] from 0): hash_h (30-bit
 *     hashes), pos_h (k-mer start in its sequence), strand_h (0: the forward k-mer is the smaller code) in position
 *     order, sequence i's at moff_h[i] .. moff_h[i+1]; the three outputs hold off_h[n] entries at most
 *   - po_map_index_create: the contigs (ctg_h back to back, ctg_off_h int64[n_ctg+1], each < 2^31 bases) and their
 *     index: n_entries minimizers sorted by (hash, contig offset + pos), the hashes that occur more than max_occ times
 *     already left out, with pos_h[i] the position in its contig and ctg_strand_h[i] = contig << 1 | strand.  Returns
 *     NULL on failure (po_last_error says why).  The index keeps its batch workspace (grow-only) until destroyed.
 *   - po_map_batch_h: maps n reads (seq_h, off_h as above; each < 2^31 bases) in batches of at most budget_bytes of
 *     workspace (0: min(8 GB, device memory / 16)), longest first; a read larger than the budget goes alone.  hits_h[n]
 *     gets one po_map_hit per read; the alignment columns of read i (0 M, 1 X = mismatch or a non-ACGT pair, 2 I,
 *     3 D; forward along the contig and Q, the read reverse-complemented on the - strand) are ops_h[op_off ..
 *     op_off + n_ops).  *ops_len gets the number of op bytes; if it exceeds ops_cap the call returns PO_E_CAP (hits_h
 *     is still written).  dbg (or NULL): the sorted anchors, the best chains and the band starts of every read, laid out
 *     by the n_anchors / n_chain that a previous call with the same reads left in hits_h (and the reads' own offsets
 *     for band_lo).  stats_h (or NULL): double[6] = device ms of sketch, anchors + sort, chain, align + trace-back; the
 *     band cells computed; the number of batches.
 *   - po_map_workspace_bytes: the workspace one batch of n_reads reads of `bases` bases in all needs, anchors aside
 *     (they are sized once counted: 28 B each) */
typedef struct po_map_index po_map_index;
typedef struct po_map_hit {
    int32_t mapped;        /* 1: the fields below describe the primary hit; 0: unmapped */
    int32_t ctg;           /* contig index */
    int32_t strand;        /* +1 / -1 */
    int32_t score;         /* the best local alignment score (0 when no alignment ran) */
    int64_t r_st, r_en;    /* half-open contig interval */
    int32_t q_st, q_en;    /* half-open interval on the read as given */
    int32_t mlen, blen, nm; /* matches; alignment columns; mismatches + inserted + deleted bases */
    int32_t n_anchors;     /* the read's anchors */
    int32_t n_chain;       /* anchors in its best chain */
    int32_t chain_score;   /* that chain's score */
    int64_t op_off;        /* into ops_h */
    int32_t n_ops, pad;
} po_map_hit;
typedef struct po_map_debug {
    uint64_t* anchor_key;  /* HOST: (2 * contig + rev) << 32 | x per anchor, each read's in sort order */
    uint32_t* anchor_y;    /* HOST: y per anchor */
    int32_t* chain;        /* HOST: the best chain as indices into the read's sorted anchors, in y order */
    int32_t* band_lo;      /* HOST: the first band column (unclipped) of every row of Q, at the read's offset */
} po_map_debug;
int po_map_sketch_h(const char* seq_h, const int64_t* off_h, int n, uint32_t* hash_h, int32_t* pos_h, uint8_t* strand_h,
                    int64_t* moff_h);
po_map_index* po_map_index_create(const char* ctg_h, const int64_t* ctg_off_h, int n_ctg, const uint32_t* hash_h,
                                  const uint32_t* pos_h, const uint32_t* ctg_strand_h, int64_t n_entries);
void po_map_index_destroy(po_map_index* ix);
int po_map_batch_h(po_map_index* ix, const char* seq_h, const int64_t* off_h, int n, int64_t budget_bytes,
                   po_map_hit* hits_h, uint8_t* ops_h, int64_t ops_cap, int64_t* ops_len, po_map_debug* dbg,
                   double* stats_h);
size_t po_map_workspace_bytes(int64_t bases, int n_reads);

/* ---- pairwise mapping for `find-pairs`: every candidate against its OWN target ----
 *   - po_map_pairs_h: n_tgt target sequences (tgt_h back to back, tgt_off_h int64[n_tgt+1] from 0, each < 2^31 bases),
 *     n_qry query sequences (qry_h, qry_off_h likewise; the two sets may be the same arrays) and n_cand candidates,
 *     cand_h int32[n_cand][2] = (query index, target index).  hits_h[c] and its alignment columns are exactly what
 *     po_map_batch_h gives for that query against an index whose only contig is that target: the target's own
 *     minimizers in (hash, pos) order, max_occ from the target's own occurrence counts, anchors, chain, band, alignment
 *     and thresholds unchanged; ctg is the target's index (of every record, mapped or not).  Everything per target and
 *     per candidate runs on the device: the targets a batch names are sketched once each, their minimizers sorted
 *     inside per-target segments, and each query minimizer is looked up in its candidate's segment alone; candidates that
 *     share a target share its segment, and a sequence no candidate names is never touched.  Candidates go in batches
 *     of at most budget_bytes of workspace (0: min(8 GB, device memory / 16)), longest query first; one larger than the
 *     budget goes alone.  An empty, short or all-N sequence, the same read as query and target, n_cand = 0 are results
 *     (mostly mapped = 0), not errors; an index out of range is PO_E_ARG before any launch.  ops_h / ops_cap / ops_len
 *     and PO_E_CAP as in po_map_batch_h.  stats_h (or NULL): double[8] = device ms of sketch (targets and queries),
 *     anchors + sort, chain, align + trace-back; the band cells computed; the number of batches; device ms of the
 *     per-target index (segmented sort + max_occ); the number of target segments built. */
int po_map_pairs_h(const char* tgt_h, const int64_t* tgt_off_h, int n_tgt, const char* qry_h, const int64_t* qry_off_h,
                   int n_qry, const int32_t* cand_h, int n_cand, int64_t budget_bytes, po_map_hit* hits_h, uint8_t* ops_h,
                   int64_t ops_cap, int64_t* ops_len, double* stats_h);

/* ---- make_labeled_data: guided, banded CTC forced alignment (po_label.hip) ----
 * The frame of every base of a known sequence, over a whole read.  Plain `ctc` model (a non-blank frame emits one
 * base, blank = column A = C - 1); state k = number of label bases emitted.  Per read i: y float64 [T_i][C] (rows
 * y_off[i] .. y_off[i+1]), label characters [L_i] at label_off[i], guide int32 [T_i] at y_off[i] or guide == NULL
 * (c[t] = floor((t + 1) * L / T)); one band_size B per batch (<= 0: no band).  Row t admits
 * max(0, c[t] - B) <= k <= min(L, c[t] + B), every other cell is -inf;  S(-1, 0) = 0,
 * S(t, k) = max(S(t-1, k) + y[t][blank], S(t-1, k-1) + y[t][code(label[k-1])]), the emitting move only when
 * strictly greater.  score[i] = S(T-1, L); map int32[total_labels] at label_off[i]: map[k] = the frame at which
 * the best path moves k -> k + 1.  Float64 throughout, the additions of a path in frame order: a numpy restatement
 * gives the same bits.
 * status[i] (no batch abort): 0; PO_E_ENVELOPE when S(T-1, L) is -inf (the band admits no path from (-1, 0) to
 * (T-1, L), or L > T); PO_E_ARG for a label character outside the alphabet, or a guide that decreases or leaves
 * [0, L].  A read with a non-zero status gets score -inf and map -1.  L == 0 is valid (score = the sum of blanks).
 * Trace-back storage is one bit per admitted cell: po_label_align_workspace_bytes is at most
 * total_rows * (2 * ceil((2B + 1) / 64) * 8 + 16) + 32 * total_labels + 64 * n + 2^20 for B >= 1.
 * B <= 63 runs on the register kernels (one wave per read); wider bands and band_size <= 0 on the general kernel. */
size_t po_label_align_workspace_bytes(int n, int64_t total_rows, int64_t max_rows, int64_t total_labels, int band_size);
int po_label_align_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int band_size,
                         const char* labels, const int64_t* label_off, const int32_t* guide, int32_t* map,
                         double* score, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int po_label_align_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet,
                           int band_size, const char* labels_h, const int64_t* label_off_h, const int32_t* guide_h,
                           int32_t* map_h, double* score_h, int32_t* status_h);

/* ---- decode --fastq: per-base log-odds of a called sequence (po_qual.hip) ----
 * A guided, banded forward-backward lattice over a whole read.  F(x) = log P(x | y) under the model's tree recurrence
 * (what po_forward_batch computes); for a read with table y [T][C] and called sequence s [L]:
 *   odds[k][b] = F(s with s[k] replaced by alphabet[b]) - F(s), b < len(alphabet) (0 for s[k] itself, -inf for b >=
 *                len(alphabet));   odds[k][4] = F(s with s[k] deleted) - F(s).      Insertions are not among the alternatives.
 * model: PO_MODEL_CTC (a non-blank frame emits one base; state k = bases emitted) or PO_MODEL_MERGE (a run of equal
 * frames is one base, equal neighbours need a blank between them, and — as in the tree — the first base's run starts
 * at frame 0; every label position has a blank and a label state, which the band admits together).
 * PO_MODEL_FLIPFLOP returns PO_E_UNSUPPORTED.  C = len(alphabet) + 1, blank = column C - 1.
 * Per read i: y float64 rows y_off[i] .. y_off[i+1], label characters [L_i] at label_off[i], guide int32 [T_i] at
 * y_off[i] or guide == NULL (c[t] = floor((t + 1) * L / T)); one band_size B per batch (<= 0: no band); L_i < 2^26.  Rows are
 * counted u = 0 .. T, "after frame u - 1": row 0 admits position 0, row u >= 1 admits
 * max(0, c[u-1] - B) <= k <= min(L, c[u-1] + B); every other cell is -inf in the forward and in the backward lattice
 * alike, so every F above is the sum over the paths that stay inside the band in the coordinates of s (a substitution
 * at k is in state k before its first frame and k + 1 from then on; a deletion of k moves from k to k + 2 with the
 * frame that emits s[k+1], or ends the read in state L - 1 for k = L - 1).
 * odds float64 [total_labels][5] at label_off[i] * 5; logp[i] = F(s) in the band (the backward lattice's corner).
 * status[i] (no batch abort): 0; PO_E_ENVELOPE when F(s) is -inf in the band (or L > T); PO_E_ARG for a label
 * character outside the alphabet, or a guide that decreases or leaves [0, L].  A read with a non-zero status gets
 * odds 0 and logp -inf.  L == 0 is valid: no rows of odds, logp = the sum of the blanks.
 * Float64 and log-space (logaddexp) throughout, no atomics, one workgroup per read: two runs give the same bits and a
 * read's bits do not depend on the rest of the batch.  The backward lattice's rows are kept in the workspace:
 * po_qual_workspace_bytes is at most (total_rows + n) * (2B + 2) * 8 (* 2 for PO_MODEL_MERGE) +
 * 112 * (total_labels + n) + 32 * n + 2^10 for B >= 1, and (max_rows + 1) * (total_labels + n) * 8 (* 2) + the same
 * tail without a band; 0 for a model other than the two. */
size_t po_qual_workspace_bytes(int n, int64_t total_rows, int64_t max_rows, int64_t total_labels, int band_size, int model);
int po_qual_batch(const double* y, const int64_t* y_off, int n, int C, const char* alphabet, int model, const char* labels,
                  const int64_t* label_off, const int32_t* guide, int band_size, double* odds, double* logp,
                  int32_t* status, void* ws, size_t ws_bytes, void* stream);
int po_qual_batch_h(const double* y_h, const int64_t* y_off_h, int n, int C, const char* alphabet, int model,
                    const char* labels_h, const int64_t* label_off_h, const int32_t* guide_h, int band_size,
                    double* odds_h, double* logp_h, int32_t* status_h);

/* ---- timing aid for bench.py: HIP events on the stream the kernels run on ----------------- */
void* po_event_create(void);
int po_event_record(void* ev, void* stream);
int po_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
void po_event_destroy(void* ev);
/* accumulated device time (ms) and launch count of the named kernel family since the last
 * reset, measured with HIP events around each launch when profiling is enabled */
#define PO_K_VITERBI 0
#define PO_K_BEAM1D 1
#define PO_K_BEAM2D 2
#define PO_K_ALIGN 3
#define PO_K_ENVELOPE 4
#define PO_K_BEAM2D_MAIN 5 /* the pair beam search kernel alone (PO_K_BEAM2D = the stage: + pre-pass, walk, queue reset) */
#define PO_K_COUNT 6
void po_profile_enable(int on);
void po_profile_reset(void);
int po_profile_get(int kernel, double* total_ms, int64_t* launches);
/* Compute-side pricing of the pair beam search (its roofline is the f64 logaddexp stream, not HBM):
 * po_profile_update_counter - two device counters (uint64[2], or NULL to stop) the pair beam kernels add
 *   update_prob evaluations to (PrefixTree.h:478-704; ctc: one logaddexp each, merge-repeats two, flip-flop
 *   three or four): [0] those the reference's schedule makes for the same input (every element over its
 *   full windows in every step, every catch-up step), [1] those the kernels executed (they leave out the
 *   ones whose result is provably already stored);
 * po_lae_peak - measured peak rate of the engine's logaddexp on this device (micro-benchmark, all lanes
 *   busy, 4 independent chains per lane). */
int po_profile_update_counter(uint64_t* device_counter);
int po_lae_peak(int iters, double* lae_per_s, void* stream);

#ifdef __cplusplus
}
#endif
#endif
