// Entry points that one translation unit of the library defines and another calls, declared ONCE: the defining file and every
// calling file include this header, so a definition that drifts from its callers is a compile error (clang rejects conflicting
// declarations of a C-linkage function) instead of a call that links and passes garbage.  The public C-ABI is
// include/poreover_hip.h; what is here is internal.  (po_reg_*: po_beam2d_common.h, next to the argument block they take.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/poreover_hip.h"

extern "C" {
// po_capi.hip
void po_set_error(const char* msg);
void po_prof_stage(int kernel, hipStream_t s, int begin, void** tok);

// po_viterbi.hip
int po_launch_viterbi(const double* y, const int64_t* y_off, int n, int C, int A, uint32_t alphabet, int kind, int8_t* path,
                      char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* map, int32_t* status, int8_t* ff_ptr,
                      int8_t* ff_path, hipStream_t stream);
int po_launch_viterbi_strided(const double* y, const int64_t* y_off, int n, int C, int A, uint32_t alphabet, int kind,
                              int8_t* path, char* seq, const int64_t* seq_off, int so_base, int so_stride, int32_t* seq_len,
                              int32_t* map, int32_t* status, int8_t* ff_ptr, int8_t* ff_path, hipStream_t stream);

// po_beam1d.hip
int po_launch_beam1d(const double* y, const int64_t* y_off, int n, int C, int A, uint32_t alphabet, int W, int model,
                     int* arena_pl, int* arena_fc, char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status,
                     hipStream_t stream);
int64_t po_beam1d_arena_nodes(int n, int64_t total_rows, int W);

// po_beam2d.hip
int po_launch_lae_peak(int iters, double* lae_per_s, hipStream_t stream);

// po_beam2d_route.hip
size_t po_beam2d_ws_bytes_impl(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, int W, int model, int method);
int po_launch_beam2d(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, const int32_t* env,
                     int n, int C, int A, uint32_t alphabet, int W, int model, int method, char* seq, const int64_t* seq_off,
                     int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes, hipStream_t stream);
void po_b2_set_update_counter(unsigned long long* dev_counter);
void po_b2_set_mark(void (*f)(int, hipStream_t));
int po_launch_beam2d_geom(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, const int32_t* env,
                          int n, int C, int A, uint32_t alphabet, int W, int model, int method, int64_t tr1, int64_t tr2,
                          int64_t mr1, int64_t mr2, char* seq, const int64_t* seq_off, int32_t* seq_len, int32_t* status,
                          int use_pre_status, void* ws, size_t ws_bytes, hipStream_t stream);

// po_pair.hip
size_t po_pair_ws_bytes_impl(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, const po_pair_options* opt);
int po_launch_pair_decode_from_1d(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n,
                                  int C, const po_pair_options* opt, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2,
                                  const int32_t* map1, const int32_t* map2, char* seq1d, const int64_t* seq1d_off,
                                  int32_t* len1, int32_t* len2, double* identity, int32_t* env_out, char* seq,
                                  const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes,
                                  hipStream_t stream);
size_t po_align_ws_bytes(int n, int64_t max_len1, int64_t max_len2, int band);
int po_launch_align(const char* seqs, const int64_t* seq_off, int n, int band, int64_t max_len1, int64_t max_len2, char* aln1,
                    char* aln2, const int64_t* aln_off, int32_t* ncol, int32_t* status, void* ws, size_t ws_bytes,
                    hipStream_t stream);
int po_launch_nw_matrix(const char* seqs, const int64_t* seq_off, int n, int match, int mismatch, int gap, int32_t* dp,
                        const int64_t* dp_off, int32_t* status, hipStream_t stream);
int po_launch_align_scores(const char* seqs, const int64_t* seq_off, int n, int band, int match, int mismatch, int gap,
                           int64_t max_len1, int64_t max_len2, char* aln1, char* aln2, const int64_t* aln_off, int32_t* ncol,
                           int32_t* status, void* ws, size_t ws_bytes, hipStream_t stream);
size_t po_envelope_ws_bytes(int n, int64_t max_ncol);
int po_launch_envelope(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol, int n,
                       const int32_t* map1, const int64_t* map1_off, const int32_t* map2, const int64_t* map2_off,
                       const int32_t* U, const int32_t* V, int padding, int64_t max_ncol, int32_t* env, const int64_t* env_off,
                       int32_t* status, void* ws, size_t ws_bytes, hipStream_t stream);
int po_launch_pair_decode(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                          const po_pair_options* opt, char* seq1d, const int64_t* seq1d_off, int32_t* len1, int32_t* len2,
                          double* identity, int32_t* env_out, char* seq, const int64_t* seq_off, int32_t* seq_len,
                          int32_t* status, void* ws, size_t ws_bytes, hipStream_t stream);
int po_launch_pair_decode_geom(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                               const po_pair_options* opt, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2,
                               const int32_t* ext_map1, const int32_t* ext_map2, char* seq1d, const int64_t* seq1d_off,
                               int32_t* len1, int32_t* len2, double* identity, int32_t* env_out, char* seq,
                               const int64_t* seq_off, int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes,
                               hipStream_t stream);

int po_launch_pair_prep_hand(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                             const po_pair_options* opt, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, char* seq1d,
                             const int64_t* seq1d_off, int32_t* len1, int32_t* len2, double* identity, int32_t* env_out,
                             int32_t* status, char* aln1, char* aln2, const int64_t* aln_off, int32_t* ncol, const int32_t** map1,
                             const int32_t** map2, const int32_t** env, void* ws, size_t ws_bytes, hipStream_t stream);

// po_skip.hip (--skip_matches; the rules are po_skip_rules.h's).  matches / indels: skip_threshold / indel_threshold; tr / mr: total and
// largest rows of the two reads, as po_launch_pair_decode_geom takes them
size_t po_skip_plan_ws_bytes(int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, const po_pair_options* opt, int matches,
                             int indels);
int po_launch_skip_plan(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                        const po_pair_options* opt, int matches, int indels, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2,
                        char* seq1d, const int64_t* seq1d_off, int32_t* len1, int32_t* len2, double* identity, int32_t* status,
                        int32_t* n_anchors, int32_t* n_boxes, void* ws, size_t ws_bytes, po_skip_totals* totals, hipStream_t stream);
size_t po_skip_run_ws_bytes(int n, int C, const po_pair_options* opt, const po_skip_totals* totals);
int po_launch_skip_run(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, int n, int C,
                       const po_pair_options* opt, int matches, int indels, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2,
                       const po_skip_totals* totals, void* plan_ws, size_t plan_ws_bytes, char* seq, const int64_t* seq_off,
                       int32_t* seq_len, int32_t* status, void* ws, size_t ws_bytes, hipEvent_t* ev, hipStream_t stream);
int po_skip_plan_tables(void* plan_ws, int n, int64_t tr1, int64_t tr2, int64_t mr1, int64_t mr2, int C, const po_pair_options* opt,
                        int matches, int indels, const int32_t** anchors, const int32_t** boxes, const int32_t** env,
                        int64_t* tab_rows);
int po_launch_skip_boxes(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol, int n, const int32_t* map1,
                         const int64_t* map1_off, const int32_t* map2, const int64_t* map2_off, const int32_t* U, const int32_t* V,
                         const int32_t* env, const int64_t* env_off, int matches, int indels, int32_t* n_anchors, int32_t* n_boxes,
                         int32_t* anchors, int32_t* boxes, int32_t* status, long long* pinfo, hipStream_t stream);

// po_lattice.hip
size_t po_lattice_ws_bytes(int n, int64_t max_rows, int64_t max_label, int model, int acceptor);
int po_launch_forward(const double* y, const int64_t* y_off, int n, int C, int A, uint32_t alphabet, int model,
                      const char* labels, const int64_t* label_off, int64_t max_rows, double* out, int32_t* status, void* ws,
                      size_t ws_bytes, hipStream_t stream);
int po_launch_acceptor(const double* y, const int64_t* y_off, int n, int C, int A, uint32_t alphabet, int band,
                       const char* labels, const int64_t* label_off, int64_t max_rows, int64_t max_label, int32_t* path,
                       int32_t* status, void* ws, size_t ws_bytes, hipStream_t stream);

// po_prefix.hip
size_t po_prefix_ws_bytes(int n, int64_t max_rows);
size_t po_pair_prefix_ws_bytes(int n, int64_t max_rows);
int po_launch_forward_vec(const double* y, const int64_t* y_off, int n, int C, int s, int i, int flavor, const double* previous,
                          double* out, hipStream_t stream);
int po_launch_pair_prefix_search(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off,
                                 const double* gm, const int64_t* gm_off, int n, int C, int A, uint32_t alphabet, int flavor,
                                 int64_t max_rows, char* seq, const int64_t* seq_off, int32_t* seq_len, double* logp,
                                 int32_t* status, void* ws, size_t ws_bytes, hipStream_t stream);
int po_launch_prefix_search(const double* y, const int64_t* y_off, int n, int C, int A, uint32_t alphabet, int64_t max_rows,
                            char* seq, const int64_t* seq_off, int32_t* seq_len, double* logp, int32_t* status, void* ws,
                            size_t ws_bytes, hipStream_t stream);

// po_gamma.hip
size_t po_gamma_ws_bytes(int n, int64_t max_cells, int64_t max_rows1, int64_t max_rows2);
int po_launch_gamma(const double* y1, const int64_t* y1_off, const double* y2, const int64_t* y2_off, const int32_t* env,
                    const int64_t* env_off, int n, int C, int flavor, int64_t max_cells, int64_t max_rows1, int64_t max_rows2,
                    double* out, double* dense_out, const int64_t* dense_off, int32_t* status, void* ws, size_t ws_bytes,
                    hipStream_t stream);

// po_ingest.hip
int po_launch_ingest(const void* src, const int64_t* row_off, int n, int C, int mode, const int* perm, int reverse,
                     int64_t total_rows, double* out, hipStream_t stream);

// po_prep.hip (enqueue only; the rules are po_prep_rules.h's): device pointers throughout, raw 16-byte aligned, slab_off / slab_read
// a PoPrepPlan's tables, stats required (a and b travel through it), ws of po_prep_workspace_bytes
size_t po_prep_workspace_bytes(int n_reads, int64_t n_slabs, int bins);
int po_launch_signal_prep(const int16_t* raw, const int64_t* raw_off, int n_reads, int64_t total, const int64_t* slab_off,
                          const int32_t* slab_read, int64_t n_slabs, int scaling, int lo, int hi, const double* offset,
                          const double* alpha, float* signal, int64_t* sig_off, po_prep_stats* stats, void* ws, size_t ws_bytes,
                          hipStream_t stream);

// po_fastq.hip (enqueue only; the rules are po_fastq_rules.h's)
int po_launch_fastq_mode(const char* seq, const int32_t* len, const char* vseq, const int32_t* vlen, const int32_t* vstatus,
                         const int64_t* seq_off, int n, int32_t* mode, hipStream_t stream);
int po_launch_fastq_gather(const char* src0, const char* src1, const int64_t* src_off, const int32_t* item, int per,
                           const int64_t* dst_off, int n_strings, int64_t total, char* dst, hipStream_t stream);
int po_launch_fastq_consumed(const char* aln1, const char* aln2, const int64_t* aln_off, const int32_t* ncol,
                             const int32_t* aln_status, int n_pairs, const int32_t* pair_read, const int64_t* out_off,
                             const int32_t* called_len, const int32_t* label_len, int32_t* consumed, int32_t* mode,
                             hipStream_t stream);
int po_launch_fastq_guide(const int32_t* map, const int32_t* consumed, const int64_t* y_off, int n, int64_t rows,
                          const int32_t* called_len, const int32_t* label_len, const int32_t* mode, int32_t* guide,
                          hipStream_t stream);
int po_launch_fastq_phred(const double* odds, const char* labels, const int64_t* label_off, const int32_t* qstatus,
                          const int64_t* out_off, int n, int64_t total, const char* alphabet, char* qual, hipStream_t stream);
int po_launch_fastq_mode2(const char* seq, const int64_t* seq_off, const int32_t* len, const char* vseq, const int64_t* vseq_off,
                          const int32_t* vlen, const int32_t* vstatus, int n, int32_t* mode, hipStream_t stream);
int po_launch_fastq_gather2(const char* src0, const int64_t* off0, const char* src1, const int64_t* off1, const int32_t* item,
                            const int64_t* dst_off, int n_strings, int64_t base, int64_t total, char* dst, hipStream_t stream);
int po_launch_fastq_pair_phred(const double* odds1, const int64_t* pos1, const int32_t* sel1, const int32_t* qst1,
                               const double* odds2, const int64_t* pos2, const int32_t* sel2, const int32_t* qst2, const char* seq,
                               const int64_t* seq_off, const int64_t* dense_off, int n, int64_t total, const char* alphabet,
                               char* qual, hipStream_t stream);

// po_qual.hip: what the entries on resident tables pass to po_qual_batch_route (include/poreover_hip.h): PO_QUAL_ROUTE_AUTO
// unless po_set_qual_route forced the other
int po_qual_entry_route();

// po_eval.hip (enqueue only; the rules are po_eval_rules.h's).  Pair i of po_launch_edit_distance is a[a_off[i] ..] of
// a_len[i] symbols (a_len NULL: a_off[i + 1] - a_off[i]) against b[b_off[i] .. b_off[i + 1])
int po_launch_eval_path(const float* probs, int n, int T, uint8_t* pred, int32_t* pred_len, hipStream_t stream);
int po_launch_edit_distance(const uint8_t* a, const int64_t* a_off, const int32_t* a_len, const uint8_t* b,
                            const int64_t* b_off, int n, int32_t* dist, int32_t* status, hipStream_t stream);

// po_train.hip, for po_train_group.hip: what a group needs of a member trainer.  po_trainer_accum_view gives the accumulator (made
// at first use, n floats, a whole allocation), the count of contributions since it was last emptied (0: empty; the group sets
// it after an all-reduce) and the trainer's stream; po_trainer_check_batch runs po_train_accumulate's checks of a batch under
// the name `me` and launches nothing
struct po_trainer_accum {
    float* ga;
    int64_t n;
    int64_t* count;
    hipStream_t stream;
};
int po_trainer_accum_view(po_trainer* tr, po_trainer_accum* out);
int po_trainer_check_batch(const po_trainer* tr, const char* me, int n, const int32_t* labels_h, const int32_t* label_len_h,
                           int merge_repeated);
}  // extern "C"

// ---- The pair-beam launch layer: po_beam2d_route.hip owns every process-wide setting and chooses the kernel family; po_beam2d.hip and
// po_beam2d_grid.hip plan the workspace of their kernel and launch it, with what they need of the settings in a PoB2Call.  C++
// linkage and hidden: no part of the library's symbol table.
#define PO_HIDDEN __attribute__((visibility("hidden")))
struct PoB2Call {   // po_launch_beam2d_geom's arguments ...
    const double* y1; const int64_t* y1_off; const double* y2; const int64_t* y2_off; const int32_t* env;
    int n, C, A; uint32_t alphabet; int W, model, method;
    int64_t mr1, mr2;
    char* seq; const int64_t* seq_off; int32_t* seq_len; int32_t* status; int use_pre_status;
    hipStream_t stream;
    // ... and the route's settings.  order: writes the queue's order (longest pair first), or NULL: input order
    void (*order)(const int64_t* y1_off, const int64_t* y2_off, int n, int* order, hipStream_t stream);
    unsigned long long* upd_count;                  // profiling: device counter of update_prob evaluations, or NULL
    void (*mark)(int begin, hipStream_t stream);    // profiling: brackets the main pair beam kernel, or NULL
};
// beam2d_kernel.  max_blocks > 0: the small pass (that many workgroups at most, the larger store) over the pairs another kernel handed on
PO_HIDDEN size_t po_b2_legacy_ws_bytes(int n, int64_t mr1, int64_t mr2, int W, int model, int method, int max_blocks);
PO_HIDDEN int po_b2_launch_legacy(const PoB2Call& c, void* ws, size_t ws_bytes, int max_blocks, const int2* only_meta, int retry = 0,
                                  const int* retry_flag = nullptr);
// beam2d_grid_kernel
PO_HIDDEN size_t po_b2_grid_ws_bytes(int n, int64_t mr1, int64_t mr2, int W, int model, bool has_env);
PO_HIDDEN int po_b2_launch_grid(const PoB2Call& c, void* ws, size_t ws_bytes);
