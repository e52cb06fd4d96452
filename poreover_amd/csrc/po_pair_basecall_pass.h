// The body of po_pair_basecall_batch_h / po_pair_basecall_fastq_batch_h / po_pair_basecall_skip_batch_h
// (po_pair_basecall.hip) on a state that may outlive the call, as po_basecall_pass.h has it for `basecall`.  The entries run
// it on a fresh state and the null stream; a po_pair_basecaller worker (po_pair_basecall_stream.hip) keeps one state per
// worker - weights uploaded once, every buffer grow-only - and gives its own stream.  Host only, hidden: nothing here is
// part of the library's symbol table.
#pragma once
#include "po_basecall_pass.h"

#pragma GCC visibility push(hidden)

// what po_pair_basecall_fastq_batch_h adds to po_pair_basecall_batch_h's arguments
struct PoPairBasecallFastq {
    int band_size; const int32_t* unbanded_h;
    char* qual1d_h; char* qual_h; int32_t* qual_status_h; double* odds1d_h; double* odds_cons_h; int32_t* guide_h;
};

// everything a call keeps on the device: the network's passes with the weights, the two pair tables, the strings, lengths
// and identities, the pair chain's workspace and the quality stages' buffers
struct PoPairBasecallResident;
PoPairBasecallResident* po_pair_basecall_resident_new();
void po_pair_basecall_resident_free(PoPairBasecallResident* st);
PoBasecallPasses& po_pair_basecall_resident_net(PoPairBasecallResident* st);
// signal_resident: signal_h is not read, the signal lies in the state's buffer, sig_off_h[n_reads] values from 0.
// skip (or NULL): {skip_threshold, indel_threshold} of --skip_matches (its run workspace depends on the data and lives for
// the call: not part of the state)
int po_pair_basecall_body(PoPairBasecallResident* st, hipStream_t stream, bool signal_resident, const char* name,
                          const float* signal_h, const int64_t* sig_off_h, int n_reads, int window, int overlap,
                          const po_call_layer* layers_h, int n_layers, const float* weights_h, int64_t n_weights,
                          int max_windows_per_pass, const int32_t* pair_idx_h, int n_pairs, int reverse_complement,
                          const po_pair_options* opt, char* seq1d_h, const int64_t* seq1d_off_h, int32_t* len1_h, int32_t* len2_h,
                          double* identity_h, char* seq_h, const int64_t* seq_off_h, int32_t* seq_len_h, int32_t* status_h,
                          float* logits_h, float* stage_ms_h, const PoPairBasecallFastq* fq, const int* skip);

#pragma GCC visibility pop
