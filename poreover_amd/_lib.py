"""ctypes binding of libporeover_hip.so (include/poreover_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is visible,
calls raise EngineUnavailable.  (The CPU restatement under oracle/ is test infrastructure and
is never imported from here.)
"""
import contextlib
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# POREOVER_HIP_LIB selects an alternative build of the same library (A/B timing builds)
LIB_PATH = os.environ.get("POREOVER_HIP_LIB") or os.path.join(HERE, "libporeover_hip.so")

OK = 0
E_CAP, E_ARG, E_ENVELOPE, E_NOMEM, E_DIVERGE, E_UNSUPPORTED, E_HIP = -1, -2, -3, -4, -5, -6, -7
SKIP_LENGTH, SKIP_IDENTITY = -10, -11
E_NO_ANCHOR, E_BOX = -12, -13      # --skip_matches: the reference's assert / IndexError (csrc/po_skip_rules.h)
MODELS = {"ctc": 0, "ctc_merge_repeats": 1, "ctc_flipflop": 2}
METHODS = {"row": 0, "row_col": 1, "grid": 2}
KINDS = {"poreover": 0, "bonito": 1, "flipflop": 2}
MODEL_OF_KIND = {"poreover": "ctc", "bonito": "ctc_merge_repeats", "flipflop": "ctc_flipflop"}   # the tree model that decodes a basecaller kind
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2, "float64": 3}   # PO_DTYPE_* of po_ingest_strided
INGEST_TILED, INGEST_PER_FRAME = 0x100, 0x200
QUAL_ROUTE_GENERAL, QUAL_ROUTE_AUTO, QUAL_ROUTE_REG = 0, 1, 2          # PO_QUAL_ROUTE_* of po_qual_batch_route
K_VITERBI, K_BEAM1D, K_BEAM2D, K_ALIGN, K_ENVELOPE, K_BEAM2D_MAIN = range(6)
_CODE_NAMES = {E_CAP: "PO_E_CAP (buffer too small)", E_ARG: "PO_E_ARG (bad argument)",
               E_ENVELOPE: "PO_E_ENVELOPE (envelope undefined for the reference)",
               E_NOMEM: "PO_E_NOMEM (node arena / band capacity exceeded)",
               E_DIVERGE: "PO_E_DIVERGE (the reference never terminates on this input)",
               E_UNSUPPORTED: "PO_E_UNSUPPORTED", E_HIP: "PO_E_HIP",
               E_NO_ANCHOR: "PO_E_NO_ANCHOR (no run of matches / indels long enough)",
               E_BOX: "PO_E_BOX (a box that is empty or lies past a basecall's end)"}


class EngineUnavailable(RuntimeError):
    pass


class EngineError(RuntimeError):
    def __init__(self, code, what, detail=""):
        super().__init__("%s: %s%s" % (what, _CODE_NAMES.get(code, "code %d" % code),
                                       (" — " + detail) if detail else ""))
        self.code = code


class PairOptions(C.Structure):
    _fields_ = [("beam_width", C.c_int), ("model", C.c_int), ("method", C.c_int), ("padding", C.c_int),
                ("full_alignment", C.c_int), ("diagonal_envelope", C.c_int), ("diagonal_width", C.c_int)]


class SkipTotals(C.Structure):
    _fields_ = [("n_boxes", C.c_int64), ("total_rows1", C.c_int64), ("total_rows2", C.c_int64), ("max_rows1", C.c_int64),
                ("max_rows2", C.c_int64)]


class CallLayer(C.Structure):
    _fields_ = [("kind", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("kernel", C.c_int)]


class BasecallerOptions(C.Structure):
    _fields_ = [("window", C.c_int), ("overlap", C.c_int), ("kind", C.c_int), ("beam_width", C.c_int), ("model", C.c_int),
                ("max_windows_per_pass", C.c_int), ("fastq", C.c_int), ("band_size", C.c_int), ("scaling", C.c_int),
                ("lo", C.c_int), ("hi", C.c_int), ("resident_bytes", C.c_int64)]


class PairBasecallerOptions(C.Structure):
    _fields_ = [("window", C.c_int), ("overlap", C.c_int), ("max_windows_per_pass", C.c_int), ("reverse_complement", C.c_int),
                ("pair", PairOptions), ("fastq", C.c_int), ("band_size", C.c_int), ("scaling", C.c_int), ("lo", C.c_int),
                ("hi", C.c_int), ("resident_bytes", C.c_int64)]


CALL_KINDS = {"conv": 0, "bigru": 1, "gru": 2, "gru_back": 3, "dense": 4}
CALL_STAGES = ("conv", "gru_proj", "gru_recur", "dense_softmax")
BASECALL_STAGES = CALL_STAGES + ("stitch_ingest", "decode")
BASECALL_FASTQ_STAGES = BASECALL_STAGES + ("guides", "lattice_phred")
PAIR_BASECALL_STAGES = CALL_STAGES + ("stitch_tables", "pair_decode")
PAIR_BASECALL_FASTQ_STAGES = PAIR_BASECALL_STAGES + ("guides", "lattice_phred")
TRAIN_STAGES = ("forward", "ctc", "back_recur", "gemm", "adam")
EVAL_STAGES = ("forward", "ctc", "path_edit")
EDIT_STATS_MAX_LONG = 262142   # po_edit_stats: the longer string of a pair (PO_EDIT_STATS_MAX_LONG; beyond it: E_CAP, distance and matches -1)
EDIT_MAX_SHORT = 4095    # po_edit_distance_batch_h / po_train_eval: the shorter string of a pair (beyond it: E_CAP, distance -1)

_vp, _i64p, _i32p, _dp, _cp = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
# every symbol include/poreover_hip.h declares: (restype, argtypes)
PROTOTYPES = {
    "po_version": (C.c_int, []),
    "po_device_count": (C.c_int, []),
    "po_set_device": (C.c_int, [C.c_int]),
    "po_last_error": (C.c_char_p, []),
    "po_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_size_t)]),
    "po_set_pair_route": (C.c_int, [C.c_int, C.c_int]),
    "po_set_chain_mode": (C.c_int, [C.c_int]),
    "po_get_chain_mode": (C.c_int, []),
    "po_set_reg_fixed_shape": (C.c_int, [C.c_int]),
    "po_get_reg_fixed_shape": (C.c_int, []),
    "po_reg_pool_prewarm": (C.c_int, [C.c_int, C.c_int]),
    "po_reg_pool_release": (C.c_int, []),
    "po_debug_deferred_pairs": (C.c_longlong, [C.c_int]),
    "po_set_align_route": (C.c_int, [C.c_int]),
    "po_set_qual_route": (C.c_int, [C.c_int]),
    "po_debug_qual_reg_reads": (C.c_longlong, [C.c_int]),
    "po_ingest_batch": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dp, _vp]),
    "po_ingest_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _dp]),
    "po_ingest_strided": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int64, _dp, _vp]),
    "po_ingest_strided_h": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _i64p, _i64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_int), C.c_int, _dp]),
    "po_pack_strings_workspace_bytes": (C.c_size_t, [C.c_int]),
    "po_pack_strings": (C.c_int, [_cp, _i64p, _i32p, _i32p, C.c_int, _cp, _i64p, _vp, C.c_size_t, _vp]),
    "po_pack_strings_h": (C.c_int, [_cp, _i64p, _i32p, _i32p, C.c_int, _cp, _i64p]),
    "po_ctc_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "po_ctc_loss": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _i32p, _i64p, C.c_int, C.c_int64,
                              C.c_int64, C.c_int, _vp, _i32p, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "po_ctc_loss_h": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _i64p, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                _i32p, _i64p, C.c_int, _vp, _i32p, _vp, C.c_int]),
    "po_forced_align_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "po_forced_align": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _i32p, _i64p, C.c_int,
                                  C.c_int64, C.c_int64, C.c_int, _dp, _i32p, C.c_int64, _i32p, _i32p, _i32p, _vp, C.c_size_t, _vp]),
    "po_forced_align_h": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _i64p, _i64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_int), _i32p, _i64p, C.c_int, _dp, _i32p, C.c_int64, _i32p, _i32p, _i32p]),
    "po_logits_path": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _cp, C.c_int64, _i32p, _vp]),
    "po_logits_path_h": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _i64p, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                   _cp, C.c_int64, _i32p]),
    "po_edit_stats": (C.c_int, [_cp, _i64p, _i32p, _cp, _i64p, _i32p, C.c_int, _i32p, _i32p, _i32p, _vp]),
    "po_edit_stats_h": (C.c_int, [_cp, _i64p, _i32p, _cp, _i64p, _i32p, C.c_int, _i32p, _i32p, _i32p]),
    "po_edit_align_trace_words": (C.c_size_t, [C.c_int64, C.c_int64]),
    "po_edit_align": (C.c_int, [_cp, _i64p, _i32p, _cp, _i64p, _i32p, C.c_int, _vp, _i64p, _cp, C.c_int64, _i32p, _i32p, _i32p, _i32p,
                                _i32p, _vp]),
    "po_edit_align_h": (C.c_int, [_cp, _i64p, _i32p, _cp, _i64p, _i32p, C.c_int, _cp, C.c_int64, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "po_viterbi_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_int]),
    "po_viterbi_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _vp, _cp, _i64p, _i32p,
                                   _i32p, _i32p, _vp, C.c_size_t, _vp]),
    "po_beam1d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "po_beam1d_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, _cp, _i64p, _i32p,
                                  _i32p, _vp, C.c_size_t, _vp]),
    "po_beam2d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                               C.c_int, C.c_int, C.c_int]),
    "po_beam2d_batch": (C.c_int, [_dp, _i64p, _dp, _i64p, _i32p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                  C.c_int, _cp, _i64p, _i32p, _i32p, _vp, C.c_size_t, _vp]),
    "po_forward_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "po_forward_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _dp, _i32p, _vp,
                                   C.c_size_t, _vp]),
    "po_viterbi_acceptor_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64]),
    "po_viterbi_acceptor_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p,
                                            _i32p, _vp, C.c_size_t, _vp]),
    "po_forward_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _dp, _i32p]),
    "po_viterbi_acceptor_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p,
                                              _i32p]),
    "po_prefix_search_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "po_prefix_search_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, _cp, _i64p, _i32p, _dp, _i32p, _vp,
                                         C.c_size_t, _vp]),
    "po_prefix_search_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, _cp, _i64p, _i32p, _dp, _i32p]),
    "po_align_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int]),
    "po_align_batch": (C.c_int, [_cp, _i64p, C.c_int, C.c_int, _cp, _cp, _i64p, _i32p, _i32p, _vp, C.c_size_t, _vp]),
    "po_align_batch_h": (C.c_int, [_cp, _i64p, C.c_int, C.c_int, _cp, _cp, _i64p, _i32p, _i32p]),
    "po_align_scores_batch_h": (C.c_int, [_cp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _cp, _cp, _i64p, _i32p, _i32p]),
    "po_nw_matrix_batch": (C.c_int, [_cp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i64p, _i32p, _vp]),
    "po_nw_matrix_batch_h": (C.c_int, [_cp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i64p, _i32p]),
    "po_envelope_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "po_envelope_batch": (C.c_int, [_cp, _cp, _i64p, _i32p, C.c_int, _i32p, _i64p, _i32p, _i64p, _i32p, _i32p, C.c_int,
                                    _i32p, _i64p, _i32p, _vp, C.c_size_t, _vp]),
    "po_envelope_batch_h": (C.c_int, [_cp, _cp, _i64p, _i32p, C.c_int, _i32p, _i64p, _i32p, _i64p, _i32p, _i32p, C.c_int,
                                      _i32p, _i64p, _i32p]),
    "po_pair_gamma_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64]),
    "po_pair_gamma_batch": (C.c_int, [_dp, _i64p, _dp, _i64p, _i32p, _i64p, C.c_int, C.c_int, C.c_int, C.c_int64, _dp, _dp,
                                      _i64p, _i32p, _vp, C.c_size_t, _vp]),
    "po_pair_gamma_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, _i32p, _i64p, C.c_int, C.c_int, C.c_int, _dp, _dp, _i64p,
                                        _i32p]),
    "po_pair_decode_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                                    C.POINTER(PairOptions)]),
    "po_pair_decode_batch": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.POINTER(PairOptions), _cp,
                                       _i64p, _i32p, _i32p, _dp, _i32p, _cp, _i64p, _i32p, _i32p, _vp,
                                       C.c_size_t, _vp]),
    "po_decode_1d_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int,
                                       C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p]),
    "po_viterbi_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _vp, _cp, _i64p, _i32p,
                                     _i32p, _i32p]),
    "po_beam1d_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, _cp, _i64p,
                                    _i32p, _i32p]),
    "po_beam2d_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, _i32p, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                    C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p]),
    "po_pair_decode_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.POINTER(PairOptions), _cp,
                                         _i64p, _i32p, _i32p, _dp, _i32p, _cp, _i64p, _i32p, _i32p]),
    "po_pair_decode_from_1d_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.POINTER(PairOptions), _cp,
                                                 _i64p, _i32p, _i32p, _i32p, _i32p, _dp, _i32p, _cp, _i64p, _i32p, _i32p]),
    "po_pair_skip_plan_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                                       C.POINTER(PairOptions), C.c_int, C.c_int]),
    "po_pair_skip_plan": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.POINTER(PairOptions), C.c_int, C.c_int, _cp, _i64p,
                                    _i32p, _i32p, _dp, _i32p, _i32p, _i32p, _vp, C.c_size_t, C.POINTER(SkipTotals), _vp]),
    "po_pair_skip_run_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.POINTER(PairOptions), C.POINTER(SkipTotals)]),
    "po_pair_skip_run": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.POINTER(PairOptions), C.c_int, C.c_int,
                                   C.POINTER(SkipTotals), _vp, C.c_size_t, _cp, _i64p, _i32p, _i32p, _vp, C.c_size_t, _vp]),
    "po_pair_skip_decode_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.POINTER(PairOptions), C.c_int, C.c_int,
                                              _cp, _i64p, _i32p, _i32p, _dp, _i32p, _cp, _i64p, _i32p, _i32p, _i32p, _i32p, _i64p,
                                              _i32p, _i32p, C.POINTER(SkipTotals), C.POINTER(C.c_float)]),
    "po_skip_boxes_batch_h": (C.c_int, [_cp, _cp, _i64p, _i32p, C.c_int, _i32p, _i64p, _i32p, _i64p, _i32p, _i32p, _i32p, _i64p,
                                        C.c_int, C.c_int, _i32p, _i32p, _i64p, _i32p, _i32p, _i32p]),
    "po_profile_update_counter": (C.c_int, [C.c_void_p]),
    "po_lae_peak": (C.c_int, [C.c_int, _dp, C.c_void_p]),
    "po_pair_prefix_search_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p,
                                                _dp, _i32p]),
    "po_pair_prefix_search_env_batch_h": (C.c_int, [_dp, _i64p, _dp, _i64p, _i32p, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp,
                                                    _i64p, _i32p, _dp, _i32p]),
    "po_forward_vec_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "po_viterbi_acceptor_cy_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p,
                                              _i32p]),
    "po_pipeline_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int64, C.c_int]),
    "po_pipeline_destroy": (None, [C.c_void_p]),
    "po_pipeline_pair_decode": (C.c_int, [C.c_void_p, _vp, _i64p, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.c_int, C.POINTER(PairOptions), _cp, _i64p, _i32p, _i32p, _dp,
                                          _i32p, _cp, _i64p, _i32p, _i32p]),
    "po_multi_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int64, C.c_int]),
    "po_multi_destroy": (None, [C.c_void_p]),
    "po_multi_devices": (C.c_int, [C.c_void_p]),
    "po_multi_pair_decode": (C.c_int, [C.c_void_p, _vp, _i64p, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.c_int, C.POINTER(PairOptions), _cp, _i64p, _i32p, _i32p, _dp,
                                       _i32p, _cp, _i64p, _i32p, _i32p]),
    "po_wave_plan": (C.c_int, [_i64p, _i64p, C.c_int, C.c_int, C.c_int64, C.c_int, _i32p, _i32p, C.c_int]),
    "po_multi_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "po_pipeline_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_int)]),
    "po_call_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int]),
    "po_call_batch": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64, _vp, _vp, _vp,
                                C.c_size_t, _vp, C.POINTER(C.c_float)]),
    "po_call_batch_h": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64, _vp, _vp,
                                  C.POINTER(C.c_float)]),
    "po_set_call_precision": (C.c_int, [C.c_int]),
    "po_get_call_precision": (C.c_int, []),
    "po_gru_proj_h": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]),
    "po_set_recur_precision": (C.c_int, [C.c_int]),
    "po_get_recur_precision": (C.c_int, []),
    "po_gru_recur_h": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "po_signal_prep_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _vp, _i64p, _vp,
                                   C.POINTER(C.c_float)]),
    "po_basecall_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64,
                                      C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p, _vp,
                                      C.POINTER(C.c_float)]),
    "po_basecall_fastq_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64,
                                            C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p, _vp,
                                            C.c_int, _cp, _i32p, _dp, _i32p, C.POINTER(C.c_float)]),
    "po_basecaller_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64, C.c_char_p,
                                          C.POINTER(BasecallerOptions)]),
    "po_basecaller_destroy": (None, [C.c_void_p]),
    "po_basecaller_run_f32": (C.c_int, [C.c_void_p, _vp, _i64p, C.c_int, _cp, _i64p, _i32p, _i32p, _vp, _cp, _i32p]),
    "po_basecaller_run_raw": (C.c_int, [C.c_void_p, _vp, _i64p, C.c_int, _dp, _dp, _cp, _i64p, _i32p, _i32p, _vp, _cp, _i32p,
                                        _i64p]),
    "po_basecaller_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                      C.POINTER(C.c_double)]),
    "po_basecall_group_plan": (C.c_int, [_i64p, C.c_int, C.c_int64, C.c_int, _i32p, _i32p, C.c_int]),
    "po_basecall_group_samples": (C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    "po_fastq_guide_h": (C.c_int, [_i32p, _i32p, _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p]),
    "po_fastq_consumed_h": (C.c_int, [_cp, _cp, _i64p, _i32p, C.c_int, _i32p, _i32p, _i64p, _i32p, _i32p]),
    "po_fastq_phred_h": (C.c_int, [_dp, _cp, _i64p, C.c_int, C.c_char_p, _i32p, _cp]),
    "po_pair_basecall_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64,
                                           C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(PairOptions), _cp, _i64p, _i32p, _i32p, _dp,
                                           _cp, _i64p, _i32p, _i32p, _vp, C.POINTER(C.c_float)]),
    "po_pair_basecall_skip_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64,
                                                C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(PairOptions), _cp, _i64p, _i32p, _i32p, _dp,
                                                _cp, _i64p, _i32p, _i32p, _vp, C.POINTER(C.c_float), C.c_int, C.c_int]),
    "po_pair_basecall_fastq_batch_h": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64,
                                                 C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(PairOptions), _cp, _i64p, _i32p, _i32p,
                                                 _dp, _cp, _i64p, _i32p, _i32p, _vp, C.c_int, _i32p, _cp, _cp, _i32p, _dp, _dp, _i32p,
                                                 C.POINTER(C.c_float)]),
    "po_pair_qual_h": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p, _cp, _i64p, _i32p, _i32p,
                                 C.c_int, _i32p, _cp, _cp, _i32p, _dp, _dp, _i32p]),
    "po_pair_qual": (C.c_int, [_dp, _i64p, _dp, _i64p, C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p, _cp, _i64p, _i32p, _i32p,
                               C.c_int, _i32p, _cp, _cp, _i32p, _dp, _dp, _i32p, _vp]),
    "po_fastq_tables": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, _cp, _i64p, _i32p, _i32p, _i32p, C.c_int, C.c_int,
                                  _i32p, _cp, _i32p, _dp, _i32p, _vp]),
    "po_fastq_pair_phred_h": (C.c_int, [_dp, _dp, _cp, _i64p, C.c_int, C.c_char_p, _i32p, _i32p, _cp]),
    "po_pair_basecaller_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int, C.POINTER(CallLayer), C.c_int, _vp, C.c_int64,
                                               C.POINTER(PairBasecallerOptions)]),
    "po_pair_basecaller_destroy": (None, [C.c_void_p]),
    "po_pair_basecaller_run_f32": (C.c_int, [C.c_void_p, _vp, _i64p, C.c_int, _i32p, C.c_int, _cp, _i64p, _i32p, _i32p, _dp, _cp, _i64p,
                                             _i32p, _i32p, _vp, _i32p, _cp, _cp, _i32p]),
    "po_pair_basecaller_run_raw": (C.c_int, [C.c_void_p, _vp, _i64p, C.c_int, _dp, _dp, _i32p, C.c_int, _cp, _i64p, _i32p, _i32p, _dp,
                                             _cp, _i64p, _i32p, _i32p, _vp, _i32p, _cp, _cp, _i32p, _i64p]),
    "po_pair_basecaller_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "po_pair_basecall_group_plan": (C.c_int, [_i64p, C.c_int, _i32p, C.c_int, C.POINTER(PairOptions), C.c_int, C.c_int, C.c_int64,
                                              C.c_int, _i32p, _i32p, C.c_int]),
    "po_pair_tables_h": (C.c_int, [_vp, _i64p, C.c_int, _i32p, C.c_int, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "po_train_create": (C.c_void_p, [C.POINTER(CallLayer), C.c_int, C.c_int, C.c_int]),
    "po_train_destroy": (None, [C.c_void_p]),
    "po_train_set_params": (C.c_int, [C.c_void_p, _vp, C.c_int64]),
    "po_train_get_params": (C.c_int, [C.c_void_p, _vp, C.c_int64]),
    "po_train_step": (C.c_int, [C.c_void_p, _vp, C.c_int, _i32p, _i32p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_int, _vp, _vp, C.POINTER(C.c_float)]),
    "po_train_last": (C.c_int, [C.c_void_p, C.c_int, _vp, _vp]),
    "po_train_eval": (C.c_int, [C.c_void_p, _vp, C.c_int, _i32p, _i32p, C.c_int, _vp, _i32p, _i32p, _i32p, _cp,
                                C.POINTER(C.c_float)]),
    "po_train_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "po_train_get_precision": (C.c_int, [C.c_void_p]),
    "po_gru_wgrad_h": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int, _vp, C.c_int, _vp]),
    "po_gru_dx_h": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    "po_train_accumulate": (C.c_int, [C.c_void_p, _vp, C.c_int, _i32p, _i32p, C.c_int, C.c_float, _vp, C.POINTER(C.c_float)]),
    "po_train_accum_reset": (C.c_int, [C.c_void_p]),
    "po_train_get_accum": (C.c_int, [C.c_void_p, _vp, C.c_int64]),
    "po_train_set_accum": (C.c_int, [C.c_void_p, _vp, C.c_int64]),
    "po_train_apply": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "po_train_get_state": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "po_train_set_state": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.c_int64]),
    "po_grad_norm_h": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_double)]),
    "po_train_group_create": (C.c_void_p, [C.POINTER(CallLayer), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "po_train_group_destroy": (None, [C.c_void_p]),
    "po_train_group_size": (C.c_int, [C.c_void_p]),
    "po_train_group_set_params": (C.c_int, [C.c_void_p, _vp, C.c_int64]),
    "po_train_group_get_params": (C.c_int, [C.c_void_p, _vp, C.c_int64]),
    "po_train_group_get_replica_params": (C.c_int, [C.c_void_p, C.c_int, _vp, C.c_int64]),
    "po_train_group_set_state": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.c_int64]),
    "po_train_group_get_state": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "po_train_group_get_replica_state": (C.c_int, [C.c_void_p, C.c_int, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "po_train_group_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "po_train_group_accumulate": (C.c_int, [C.c_void_p, _vp, _i32p, _i32p, _i32p, C.c_int, _vp, _vp, _vp]),
    "po_train_group_get_accum": (C.c_int, [C.c_void_p, C.c_int, _vp, C.c_int64]),
    "po_train_group_set_accum": (C.c_int, [C.c_void_p, C.c_int, _vp, C.c_int64]),
    "po_train_group_reduce": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "po_train_group_apply": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "po_train_group_eval": (C.c_int, [C.c_void_p, _vp, _i32p, _i32p, _i32p, C.c_int, _vp, _i32p, _i32p, _i32p, _cp, _vp]),
    "po_set_dp_route": (C.c_int, [C.c_int]),
    "po_get_dp_route": (C.c_int, []),
    "po_dp_allreduce_h": (C.c_int, [_i32p, C.c_int, _vp, _i32p, C.c_int64, _vp]),
    "po_eval_path_h": (C.c_int, [_vp, C.c_int, C.c_int, _cp, _i32p]),
    "po_edit_distance_batch_h": (C.c_int, [_cp, _i64p, _cp, _i64p, C.c_int, _i32p, _i32p]),
    "po_map_sketch_h": (C.c_int, [_cp, _i64p, C.c_int, _vp, _vp, _vp, _i64p]),
    "po_map_index_create": (C.c_void_p, [_cp, _i64p, C.c_int, _vp, _vp, _vp, C.c_int64]),
    "po_map_index_destroy": (None, [C.c_void_p]),
    "po_map_batch_h": (C.c_int, [C.c_void_p, _cp, _i64p, C.c_int, C.c_int64, C.c_void_p, _vp, C.c_int64,
                                 C.POINTER(C.c_int64), C.c_void_p, _dp]),
    "po_map_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "po_map_pairs_h": (C.c_int, [_cp, _i64p, C.c_int, _cp, _i64p, C.c_int, _i32p, C.c_int, C.c_int64, C.c_void_p, _vp,
                                 C.c_int64, C.POINTER(C.c_int64), _dp]),
    "po_label_align_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int]),
    "po_label_align_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p, _i32p, _dp, _i32p,
                                       _vp, C.c_size_t, _vp]),
    "po_label_align_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p, _i32p, _dp,
                                         _i32p]),
    "po_qual_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "po_qual_batch": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p, C.c_int, _dp, _dp, _i32p,
                                _vp, C.c_size_t, _vp]),
    "po_qual_batch_route": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p, C.c_int, _dp, _dp, _i32p,
                                      _vp, C.c_size_t, _vp, C.c_int]),
    "po_qual_batch_h": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, C.c_char_p, C.c_int, _cp, _i64p, _i32p, C.c_int, _dp, _dp,
                                  _i32p]),
    "po_event_create": (C.c_void_p, []),
    "po_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "po_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "po_event_destroy": (None, [C.c_void_p]),
    "po_profile_enable": (None, [C.c_int]),
    "po_profile_reset": (None, []),
    "po_profile_get": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}

_lib = None


def load(require_gpu=True):
    """Load the HIP library (once).  Raises EngineUnavailable instead of falling back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineUnavailable(
                "libporeover_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError here means the .so is stale vs the header
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    if require_gpu and _lib.po_device_count() < 1:
        raise EngineUnavailable("no HIP device visible: the decoding engine needs an MI355X (gfx950) GPU; "
                                "there is no CPU fallback")
    return _lib


_CURRENT_DEVICE = [None]


def set_device(device):
    """Bind this process (its calling thread, as HIP does) to `device` for every later engine call, and remember it:
    the cached pipelines of stream.pair_decode_stream are per device and ask current_device()."""
    check(load().po_set_device(int(device)), "po_set_device(%d)" % int(device))
    _CURRENT_DEVICE[0] = int(device)


def current_device():
    """The device set_device() chose, else POREOVER_DEVICE (what dist.run_sharded gives its workers), else 0."""
    if _CURRENT_DEVICE[0] is not None:
        return _CURRENT_DEVICE[0]
    return int(os.environ.get("POREOVER_DEVICE", "0") or 0)


ROUTES = {"auto": 0, "legacy": 2, "reg": 4}


def set_pair_route(route="auto", defer_odd=False, starve=0):
    """test / tuning hook (po_set_pair_route): which kernel serves the pair beam search; defer_odd: every odd pair is handed
    to beam2d_kernel; starve: 1 = the register-state kernel runs with a dozen row groups, 2 = with a tiny tree arena (pairs run
    out of them and are handed on)"""
    check(load(False).po_set_pair_route(ROUTES[route], (1 if defer_odd else 0) | ((int(starve) & 3) << 1)), "po_set_pair_route")


CHAIN_MODES = {"serial": 0, "closed_form": 1, "closed_guard3": 2}


def set_chain_mode(mode="serial"):
    """po_set_chain_mode: how the register-state pair kernel computes a new element's window — "serial" (default): the
    reference's logaddexp chain; "closed_form": one exp, a prefix sum, one log per time (values within ~1e-12 of the
    reference's, strings inside its edit tolerance; measured slower, opt-in); "closed_guard3": the tests' way to its hand-over"""
    check(load(False).po_set_chain_mode(CHAIN_MODES[mode]), "po_set_chain_mode")


def get_chain_mode():
    return {v: k for k, v in CHAIN_MODES.items()}[int(load(False).po_get_chain_mode())]


CALL_PRECISIONS = {"f32": 0, "bf16": 1}
TRAIN_PRECISIONS = CALL_PRECISIONS     # po_train_set_precision takes the same codes (a trainer's own mode)


DP_ROUTES = {"auto": 0, "peer": 1, "host": 2}


def set_dp_route(route="auto"):
    """po_set_dp_route: how the gradient slices of a TrainerGroup's all-reduce travel between replicas — "peer": the kernels
    read the peers' device memory; "host": through pinned host buffers; "auto" (default): peer where every pair of the group's
    devices can, else host.  The same bits either way; process-wide, read by every reduce"""
    if route not in DP_ROUTES:
        raise ValueError("dp route %r (one of %s)" % (route, ", ".join(DP_ROUTES)))
    check(load(False).po_set_dp_route(DP_ROUTES[route]), "po_set_dp_route")


def get_dp_route():
    return {v: k for k, v in DP_ROUTES.items()}[int(load(False).po_get_dp_route())]


@contextlib.contextmanager
def dp_route(route):
    """the reduces of the block run under `route`; the previous one is back afterwards, whatever happens"""
    before = get_dp_route()
    set_dp_route(route)
    try:
        yield
    finally:
        set_dp_route(before)


def dp_allreduce(bufs, devices, present=None):
    """po_dp_allreduce_h: the all-reduce stage of a TrainerGroup alone.  bufs: R float32 vectors of one length (None where
    not present), replica r on devices[r]; returns the R results (each replica's copy of the sum in replica order)"""
    import numpy as np
    R = len(devices)
    present = [b is not None for b in bufs] if present is None else [bool(x) for x in present]
    arrs = [np.ascontiguousarray(b, dtype=np.float32) if b is not None else None for b in bufs]
    n = next((a.size for a in arrs if a is not None), 0)
    outs = [np.zeros(n, dtype=np.float32) for _ in range(R)]
    dev = (C.c_int * R)(*[int(d) for d in devices])
    pres = (C.c_int * R)(*[1 if p else 0 for p in present])
    inp = (C.c_void_p * R)(*[a.ctypes.data if a is not None else None for a in arrs])
    outp = (C.c_void_p * R)(*[o.ctypes.data for o in outs])
    check(load().po_dp_allreduce_h(dev, R, inp, pres, n, outp), "po_dp_allreduce_h")
    return outs


def _precision_code(name):
    if name not in CALL_PRECISIONS:
        raise ValueError("call precision %r (one of %s)" % (name, ", ".join(CALL_PRECISIONS)))
    return CALL_PRECISIONS[name]


def set_call_precision(name="f32"):
    """po_set_call_precision: the operands of the network's GRU input projections — "f32" (default) or "bf16" (rounded to
    bf16, products and sums in f32; about one called base in a thousand differs).  Process-wide: prefer
    call_precision() or the precision= keyword of forward / basecall_signals / pair_basecall_signals, which restore it."""
    code = _precision_code(name)
    check(load(False).po_set_call_precision(code), "po_set_call_precision")


def get_call_precision():
    return {v: k for k, v in CALL_PRECISIONS.items()}[int(load(False).po_get_call_precision())]


@contextlib.contextmanager
def call_precision(name):
    """the engine calls of the block run under call precision `name`; the previous one is back afterwards, whatever happens"""
    code = _precision_code(name)
    lib = load(False)
    before = int(lib.po_get_call_precision())
    check(lib.po_set_call_precision(code), "po_set_call_precision")
    try:
        yield
    finally:
        lib.po_set_call_precision(before)


RECUR_PRECISIONS = {"f32": 0, "bf16x3": 1}


def _recur_code(name):
    if name not in RECUR_PRECISIONS:
        raise ValueError("recurrence precision %r (one of %s)" % (name, ", ".join(RECUR_PRECISIONS)))
    return RECUR_PRECISIONS[name]


def set_recur_precision(name="f32"):
    """po_set_recur_precision: the product h·U of the network's GRU recurrence — "f32" (default) or "bf16x3" (h and U each
    split in two bf16 values, three bf16 products with f32 sums; logits stay within the f32 path's bound).
    Independent of set_call_precision.  Process-wide: prefer recur_precision() or the recurrence= keyword of forward /
    basecall_signals / pair_basecall_signals, which restore it."""
    code = _recur_code(name)
    check(load(False).po_set_recur_precision(code), "po_set_recur_precision")


def get_recur_precision():
    return {v: k for k, v in RECUR_PRECISIONS.items()}[int(load(False).po_get_recur_precision())]


@contextlib.contextmanager
def recur_precision(name):
    """the engine calls of the block run under recurrence precision `name`; the previous one is back afterwards, whatever
    happens"""
    code = _recur_code(name)
    lib = load(False)
    before = int(lib.po_get_recur_precision())
    check(lib.po_set_recur_precision(code), "po_set_recur_precision")
    try:
        yield
    finally:
        lib.po_set_recur_precision(before)


def set_reg_fixed_shape(on=True):
    """po_set_reg_fixed_shape: whether pair launches of the default shape (ctc, beam_width 5, four bases) take the register-state
    kernel's instantiation compiled for that shape (default) or the run-time kernel of every other shape; results are identical"""
    check(load(False).po_set_reg_fixed_shape(1 if on else 0), "po_set_reg_fixed_shape")


def get_reg_fixed_shape():
    return bool(load(False).po_get_reg_fixed_shape())


def reg_pool_prewarm(model="ctc", beam_width=5):
    """po_reg_pool_prewarm: make the register-state pair kernel's slice pool for (model, beam_width) on the current device now"""
    check(load().po_reg_pool_prewarm(MODELS[model], int(beam_width)), "po_reg_pool_prewarm")


def reg_pool_release():
    """po_reg_pool_release: wait for the device and free every slice pool of the current device"""
    check(load().po_reg_pool_release(), "po_reg_pool_release")


def deferred_pairs(reset=False):
    """test hook (po_debug_deferred_pairs): pairs handed from the register-state kernel to beam2d_kernel since the last reset"""
    return int(load(False).po_debug_deferred_pairs(1 if reset else 0))


def set_align_route(legacy=False):
    """test / tuning hook (po_set_align_route): the banded aligner on its row-at-a-time kernel (True) or the skewed wavefront"""
    check(load(False).po_set_align_route(1 if legacy else 0), "po_set_align_route")


def set_qual_route(route):
    """test hook (po_set_qual_route): the route that the quality entries on resident tables pass to the lattice from now on,
    QUAL_ROUTE_AUTO (the default), QUAL_ROUTE_GENERAL or QUAL_ROUTE_REG (rings of at most 64 indices on qual_reg_kernel)"""
    check(load(False).po_set_qual_route(int(route)), "po_set_qual_route")


def qual_reg_reads(reset=False):
    """test hook (po_debug_qual_reg_reads): the reads launched on qual_reg_kernel since the last reset"""
    return int(load(False).po_debug_qual_reg_reads(1 if reset else 0))


def check(rc, what):
    if rc != OK:
        detail = load(False).po_last_error()
        raise EngineError(rc, what, detail.decode() if detail else "")
