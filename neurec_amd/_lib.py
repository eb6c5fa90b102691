"""ctypes binding of libneurec_hip.so (the C ABI declared in include/neurec_hip.h).

There is no CPU fallback: if the shared library is missing or fails to load,
importing this module raises.  Build it with ``python -m neurec_amd.build``.
"""
import ctypes as C
import os

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libneurec_hip.so")

ERR_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_WORKSPACE = 1, 2, 3, 4


class NeuRecHipError(RuntimeError):
    """A HIP runtime failure or workspace error reported by the native library."""


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "libneurec_hip.so is not built (expected at %s). Run `python -m neurec_amd.build` "
            "(needs hipcc; the engine has no CPU fallback)." % LIB_PATH)
    if os.path.isfile(_build.STAMP) and not _build.is_current() and not os.environ.get("NEUREC_ALLOW_STALE_LIB"):
        raise ImportError(
            "libneurec_hip.so was built from other sources than neurec_amd/csrc now holds (digest in %s differs). "
            "Run `python -m neurec_amd.build`; NEUREC_ALLOW_STALE_LIB=1 loads it anyway." % _build.STAMP)
    try:
        return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the box
        raise ImportError("cannot load %s: %s" % (LIB_PATH, e))


lib = _load()

p = C.c_void_p
i32, i64, u64, f32 = C.c_int, C.c_int64, C.c_uint64, C.c_float
sz = C.c_size_t
psz = C.POINTER(C.c_size_t)



class LightGCNBuffers(C.Structure):
    """nrhip_lightgcn_buffers (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "plan", "plan_t", "indptr", "indices", "vals", "indptr_t", "indices_t", "vals_t",
        "E0", "m", "v", "Ea", "Eb", "Esum", "Esum_rows", "Gstar", "Greg", "H", "Ga", "Gb",
        "batch_rows", "row_flag", "terms", "spmm_ws")] + [
        ("spmm_ws_bytes", C.c_size_t), ("n_users", C.c_int), ("n_nodes", C.c_int), ("d", C.c_int),
        ("n_layers", C.c_int), ("max_batch", C.c_int), ("reg", C.c_float)]


class MFBuffers(C.Structure):
    """nrhip_mf_buffers (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("P", "Q", "mP", "vP", "mQ", "vQ", "GP", "GQ", "terms")] + [
        ("n_users", C.c_int), ("n_items", C.c_int), ("d", C.c_int), ("max_batch", C.c_int),
        ("reg", C.c_float), ("last", C.c_void_p), ("stamp", C.c_void_p), ("alpha_tab", C.c_void_p),
        ("alpha_len", C.c_int),
        ("lazy_period", C.c_int), ("tw", C.c_void_p), ("inb", C.c_void_p)]


NGCF_MAX_LAYERS = 4


class NGCFBuffers(C.Structure):
    """nrhip_ngcf_buffers (include/neurec_hip.h)"""
    _L = NGCF_MAX_LAYERS
    _fields_ = [(n, C.c_void_p) for n in ("plan", "plan_t", "indptr", "indices", "vals", "indptr_t", "indices_t",
                                          "vals_t", "spmm_ws")] + [("spmm_ws_bytes", C.c_size_t)] + \
        [(n, C.c_void_p) for n in ("E0", "mE", "vE", "gE0", "Out", "dOut")] + \
        [("S", C.c_void_p * _L), ("ego", C.c_void_p * (_L + 1)), ("mask", C.c_void_p * _L),
         ("W", (C.c_void_p * 4) * _L), ("gW", (C.c_void_p * 4) * _L), ("mW", (C.c_void_p * 4) * _L),
         ("vW", (C.c_void_p * 4) * _L)] + \
        [(n, C.c_void_p) for n in ("dS", "dEd", "dT1", "dT2")] + [("dEgo", C.c_void_p * 2)] + \
        [("terms", C.c_void_p), ("rows", C.c_void_p), ("flag", C.c_void_p), ("ws", C.c_void_p),
         ("ws_bytes", C.c_size_t), ("n_users", C.c_int), ("n_nodes", C.c_int), ("d", C.c_int),
         ("n_layers", C.c_int), ("max_batch", C.c_int), ("reg", C.c_float), ("keep", C.c_float)]


NGCF_WIDE_MAX_LAYERS = 8


class NGCFWideBuffers(C.Structure):
    """nrhip_ngcf_wide_buffers (include/neurec_hip.h)"""
    _L = NGCF_WIDE_MAX_LAYERS
    _fields_ = [(n, C.c_void_p) for n in ("plan", "indptr", "indices", "vals", "plan_t", "indptr_t", "indices_t",
                                          "vals_t")] + \
        [("ws_fwd", C.c_void_p * _L), ("ws_fwd_bytes", C.c_size_t * _L), ("ws_bwd", C.c_void_p * _L),
         ("ws_bwd_bytes", C.c_size_t * _L)] + \
        [(n, C.c_int) for n in ("n_users", "n_nodes", "n_layers", "max_batch", "dsum", "splits")] + \
        [("w", C.c_int * (_L + 1)), ("wp", C.c_int * (_L + 1)), ("off", C.c_int * (_L + 2))] + \
        [(n, C.c_void_p) for n in ("E0p", "mE", "vE", "gE0", "Out", "dOut")] + \
        [("ego", C.c_void_p * (_L + 1)), ("S", C.c_void_p * _L), ("X2", C.c_void_p * _L), ("T1", C.c_void_p * _L),
         ("T2", C.c_void_p * _L), ("mask", C.c_void_p * _L),
         ("W", (C.c_void_p * 4) * _L), ("gW", (C.c_void_p * 4) * _L), ("mW", (C.c_void_p * 4) * _L),
         ("vW", (C.c_void_p * 4) * _L),
         ("dS", C.c_void_p * _L), ("dEd", C.c_void_p * _L), ("dEgo", C.c_void_p * _L)] + \
        [(n, C.c_void_p) for n in ("dT1", "dT2", "Y1", "Y2", "terms", "cs_ws")] + \
        [("cs_ws_bytes", C.c_size_t), ("rows", C.c_void_p), ("flag", C.c_void_p), ("gemm_ws", C.c_void_p),
         ("gemm_ws_bytes", C.c_size_t), ("reg", C.c_float), ("keep", C.c_float)]


class VaeStepArgs(C.Structure):
    """nrhip_vae_step_args (include/neurec_hip.h)"""
    _fields_ = [("indptr", C.c_void_p), ("indices", C.c_void_p), ("n_items", C.c_int), ("h", C.c_int), ("z", C.c_int),
                ("act", C.c_int), ("P", C.c_void_p * 8), ("G", C.c_void_p * 8), ("M", C.c_void_p * 8),
                ("V", C.c_void_p * 8), ("sizes", C.c_int64 * 8)] + \
        [(n, C.c_void_p) for n in ("H1", "MU", "LOGVAR", "EPSSTD", "ZS", "G1", "KLb", "h0val", "nll", "dG1", "DA3",
                                   "DH2", "DA1", "stats", "regsum", "ws")] + \
        [("ws_bytes", C.c_size_t), ("drop_given", C.c_void_p), ("eps_given", C.c_void_p), ("reg", C.c_float),
         ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float), ("seed", C.c_uint64)]


class EvalPrunedArgs(C.Structure):
    """nrhip_eval_pruned_args (include/neurec_hip.h)"""
    _fields_ = [("P", C.c_void_p), ("ldp", C.c_int64), ("Q", C.c_void_p), ("ldq", C.c_int64), ("d", C.c_int),
                ("cols", C.c_int), ("users", C.c_void_p), ("n_users", C.c_int), ("batch_rows", C.c_int),
                ("tr_indptr", C.c_void_p), ("tr_indices", C.c_void_p), ("truth_indptr", C.c_void_p),
                ("truth_indices", C.c_void_p), ("chunk_tile", C.c_void_p), ("chunk_begin", C.c_void_p),
                ("n_chunks", C.c_int), ("tile_ptr", C.c_void_p), ("plan_user", C.c_void_p), ("plan_mask", C.c_void_p),
                ("row_of", C.c_void_p), ("metric_ids", C.POINTER(C.c_int)), ("n_metric", C.c_int), ("top_k", C.c_int),
                ("n_keep", C.c_int), ("use_filter", C.c_int), ("prepare_items", C.c_int),
                ("gemm_ws", C.c_void_p), ("gemm_ws_bytes", C.c_size_t), ("filter_ws", C.c_void_p),
                ("filter_ws_bytes", C.c_size_t), ("tiles_ws", C.c_void_p), ("tiles_ws_bytes", C.c_size_t),
                ("M", C.c_void_p), ("mld", C.c_int64), ("eps", C.c_void_p), ("out", C.c_void_p), ("flags", C.c_void_p),
                ("sums", C.c_void_p), ("colsum_ws", C.c_void_p), ("colsum_ws_bytes", C.c_size_t)]


class EvalRedoArgs(C.Structure):
    """nrhip_eval_redo_args (include/neurec_hip.h)"""
    _fields_ = [("ev", C.POINTER(EvalPrunedArgs)), ("n_flagged", C.c_int), ("reload_items", C.c_int),
                ("scores", C.c_void_p), ("lds", C.c_int64), ("slab_rows", C.c_int), ("rows", C.c_void_p),
                ("row_users", C.c_void_p), ("count", C.c_void_p), ("fixed", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_size_t)]


class FismStepArgs(C.Structure):
    """nrhip_fism_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "indptr", "indices", "t_indptr", "t_users", "c1", "Q", "bias", "G_c1", "G_Q", "G_bias", "flag_Q", "flag_bias",
        "flag_c1", "users", "items", "third", "keys", "inst", "n", "p", "g", "scal", "slot", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "batch", "pairwise", "loss_kind", "step")] + \
        [(n, C.c_float) for n in ("alpha", "reg_p", "reg_q")]


class NaisStepArgs(C.Structure):
    """nrhip_nais_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "indptr", "indices", "t_indptr", "t_users", "c1", "Q", "bias", "W", "b", "h", "G_c1", "G_Q", "G_bias", "G_W",
        "G_b", "G_h", "flag_Q", "flag_bias", "flag_c1", "users", "items", "third", "keys", "inst", "n", "p", "scal",
        "slot", "off", "need", "pkeys", "rows", "dWp", "dbp", "dhp", "dqp", "loss2")] + [("row_cap", C.c_int64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "w", "batch", "pairwise", "loss_kind", "step", "algorithm",
                                "activation", "reference_mask", "c1_sort")] + \
        [(n, C.c_float) for n in ("alpha", "beta", "reg_p", "reg_q")]


class NaisScoresArgs(C.Structure):
    """nrhip_nais_scores_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "indptr", "indices", "c1", "Q", "bias", "W", "b", "h", "users", "out", "map", "hs", "cnt", "E", "F", "cW",
        "qW")] + [("ld", C.c_int64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "w", "algorithm", "activation", "batch", "h_cap", "tile",
                                "project", "mfma")] + \
        [(n, C.c_float) for n in ("alpha", "beta")]


class FpmcStepArgs(C.Structure):
    """nrhip_fpmc_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "UI", "IU", "IL", "LI", "G_UI", "G_IU", "G_IL", "G_LI", "flag_UI", "flag_IU", "flag_IL", "flag_LI", "users",
        "recent", "items", "third", "keys", "scal", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "batch", "pairwise", "loss_kind")] + [("reg", C.c_float)]


class FossilStepArgs(C.Structure):
    """nrhip_fossil_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "indptr", "indices", "t_indptr", "t_users", "c1", "Q", "bias", "eta", "eta_bias", "G_c1", "G_Q", "G_bias",
        "G_eta", "G_eta_bias", "flag_Q", "flag_bias", "flag_c1", "flag_eta", "users", "recents", "items", "third",
        "keys", "inst", "n", "p", "x", "g", "dots", "scal", "slot", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "L", "batch", "pairwise", "loss_kind", "step")] + \
        [(n, C.c_float) for n in ("alpha", "reg_p", "reg_q", "reg_eta")]


class HrmStepArgs(C.Structure):
    """nrhip_hrm_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "P", "V", "G_P", "G_V", "flag_P", "flag_V", "users", "recents", "items", "labels", "keys", "scal", "s", "ds",
        "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "L", "batch", "pre_max", "session_max", "loss_kind")] + \
        [("reg", C.c_float)]


class NpeStepArgs(C.Structure):
    """nrhip_npe_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "P", "V", "W", "G_P", "G_V", "G_W", "flag_P", "flag_V", "flag_W", "users", "recents", "items", "labels",
        "keys", "scal", "s", "ds", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "L", "batch", "loss_kind")] + [("reg", C.c_float)]


class FpmcplusStepArgs(C.Structure):
    """nrhip_fpmcplus_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "UI", "IU", "IL", "LI", "W", "b", "h", "G_UI", "G_IU", "G_IL", "G_LI", "G_W", "G_b", "G_h", "flag_UI",
        "flag_IU", "flag_IL", "flag_LI", "users", "recents", "items", "third", "keys", "contrib", "scal", "delta",
        "partial", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "w", "L", "batch", "pairwise", "loss_kind")] + \
        [("reg_mf", C.c_float), ("reg_w", C.c_float)]


class FpmcplusScoresArgs(C.Structure):
    """nrhip_fpmcplus_scores_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "UI", "IU", "IL", "LI", "W", "b", "h", "last", "users", "c", "p", "out")] + [("ld", C.c_int64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "w", "L", "batch")]


class TransrecStepArgs(C.Structure):
    """nrhip_transrec_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "P", "Q", "b", "T", "G_P", "G_Q", "G_b", "G_T", "flag_P", "flag_Q", "flag_b", "users", "recent", "items",
        "third", "keys", "scal", "partial", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "batch", "pairwise", "loss_kind")] + [("reg", C.c_float)]


class SbprSetsArgs(C.Structure):
    """nrhip_sbpr_sets_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "tr_indptr", "tr_indices", "s_indptr", "s_indices", "pair_off", "keys", "cnt", "pos", "chunk", "items_out",
        "counts_out", "indptr_out", "total", "seg_len", "big_off", "big_len")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "u0", "u1")] + [("n_pairs", C.c_int64)] + \
        [(n, C.c_int) for n in ("max_seg_len", "n_big")]


class SbprStreamArgs(C.Structure):
    """nrhip_sbpr_stream_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "tr_indptr", "tr_indices", "c_indptr", "c_items", "c_counts", "slot_ptr", "slot_row", "elig", "users_out",
        "items_out", "social_out", "neg_out", "suk_out")] + \
        [(n, C.c_int64) for n in ("n_slots", "out_begin", "out_count")] + \
        [(n, C.c_uint64) for n in ("seed", "epoch")] + \
        [(n, C.c_int) for n in ("n_elig", "n_users", "n_items", "shuffle")]


class SbprStepArgs(C.Structure):
    """nrhip_sbpr_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "P", "Q", "b", "G_P", "G_Q", "G_b", "flag_P", "flag_Q", "flag_b", "users", "items", "social", "neg", "suk",
        "keys", "scal", "loss2")] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "batch", "loss_kind")] + [("reg", C.c_float)]


class JcaArgs(C.Structure):
    """nrhip_jca_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "W", "M", "V", "G", "flag", "indptr", "indices", "t_indptr", "t_users", "rowslot", "colslot", "wsf", "wsi",
        "wsd", "rows", "cols", "pairs", "total", "loss2")] + \
        [("n_pairs", C.c_int64), ("stamp", C.c_int64), ("seed", C.c_uint64), ("epoch", C.c_uint64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "H", "batch_size", "num_neg", "n_rows", "n_cols", "f_act",
                                "g_act", "block_i", "block_j")] + [("margin", C.c_float), ("reg", C.c_float)]


class AprStepArgs(C.Structure):
    """nrhip_apr_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "P", "Q", "G_P", "G_Q", "flag_P", "flag_Q", "users", "pos", "neg", "delta_given", "keys", "scal", "where",
        "gamma", "delta", "part", "loss2")] + [("seed", C.c_uint64), ("step", C.c_uint64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "batch", "adversarial", "adv_random", "with_reg")] + \
        [(n, C.c_float) for n in ("reg", "reg_adv", "eps")]


GRU4REC_MAX_LAYERS = 3


class Gru4recWeights(C.Structure):
    """nrhip_gru4rec_weights (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p * GRU4REC_MAX_LAYERS) for n in ("Wg", "bg", "Wc", "bc")] + [("width", C.c_int * GRU4REC_MAX_LAYERS),
                                                                          ("n_layers", C.c_int), ("hidden_act", C.c_int)]


class Gru4recStepArgs(C.Structure):
    """nrhip_gru4rec_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("Ein", "Q", "b")] + [("w", Gru4recWeights)] + \
        [(n, C.c_void_p) for n in ("G_Ein", "G_Q", "G_b")] + \
        [(n, C.c_void_p * GRU4REC_MAX_LAYERS) for n in ("G_Wg", "G_bg", "G_Wc", "G_bc", "state", "h_new")] + \
        [(n, C.c_void_p) for n in ("X", "Y", "keys", "ws", "loss2")] + \
        [(n, C.c_int) for n in ("n_items", "batch", "final_act", "loss_kind")] + [("reg", C.c_float)]


class Gru4recplusStepArgs(C.Structure):
    """nrhip_gru4recplus_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("Ein", "Q", "b")] + [("w", Gru4recWeights)] + \
        [(n, C.c_void_p) for n in ("G_Ein", "G_Q", "G_b")] + \
        [(n, C.c_void_p * GRU4REC_MAX_LAYERS) for n in ("G_Wg", "G_bg", "G_Wc", "G_bc", "state", "h_new")] + \
        [(n, C.c_void_p) for n in ("X", "Y", "keys", "ws", "loss2")] + \
        [(n, C.c_int) for n in ("n_items", "batch", "n_sample", "final_act", "loss_kind")] + \
        [("reg", C.c_float), ("bpr_reg", C.c_float)]


SASREC_MAX_BLOCKS, SASREC_BLOCK_VARS = 4, 14
SASREC_MAX_SITES = 1 + 3 * SASREC_MAX_BLOCKS


class SasrecWeights(C.Structure):
    """nrhip_sasrec_weights (include/neurec_hip.h)"""
    _fields_ = [("item", C.c_void_p), ("pos", C.c_void_p), ("blk", (C.c_void_p * SASREC_BLOCK_VARS) * SASREC_MAX_BLOCKS),
                ("lnf_beta", C.c_void_p), ("lnf_gamma", C.c_void_p)] + \
        [(n, C.c_int) for n in ("n_items", "d", "L", "n_blocks", "n_heads")]


class SasrecStepArgs(C.Structure):
    """nrhip_sasrec_step_args (include/neurec_hip.h)"""
    _fields_ = [("w", SasrecWeights), ("G_item", C.c_void_p), ("G_pos", C.c_void_p),
                ("G_blk", (C.c_void_p * SASREC_BLOCK_VARS) * SASREC_MAX_BLOCKS), ("G_lnf_beta", C.c_void_p),
                ("G_lnf_gamma", C.c_void_p), ("seq", C.c_void_p), ("pos_ids", C.c_void_p), ("neg_ids", C.c_void_p),
                ("mask", C.c_void_p * SASREC_MAX_SITES), ("keys", C.c_void_p), ("ws", C.c_void_p), ("loss2", C.c_void_p),
                ("seed", C.c_uint64), ("batch", C.c_int), ("step", C.c_int), ("rate", C.c_float), ("l2_emb", C.c_float)]


CASER_MAX_LEN = 10


class CaserWeights(C.Structure):
    """nrhip_caser_weights (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("user", "seq_item", "item", "item_bias", "conv_v", "conv_v_bias")] + \
        [("conv_h", C.c_void_p * CASER_MAX_LEN), ("conv_h_bias", C.c_void_p * CASER_MAX_LEN), ("fc", C.c_void_p),
         ("fc_bias", C.c_void_p)] + [(n, C.c_int) for n in ("n_users", "n_items", "d", "L", "nv", "nh")]


class CaserStepArgs(C.Structure):
    """nrhip_caser_step_args (include/neurec_hip.h)"""
    _fields_ = [("w", CaserWeights)] + \
        [(n, C.c_void_p) for n in ("G_user", "G_seq_item", "G_item", "G_item_bias", "G_conv_v", "G_conv_v_bias")] + \
        [("G_conv_h", C.c_void_p * CASER_MAX_LEN), ("G_conv_h_bias", C.c_void_p * CASER_MAX_LEN), ("G_fc", C.c_void_p),
         ("G_fc_bias", C.c_void_p)] + \
        [(n, C.c_void_p) for n in ("users", "seq", "pos", "neg", "mask", "keys", "ws", "loss2")] + \
        [("seed", C.c_uint64), ("batch", C.c_int), ("T", C.c_int), ("N", C.c_int), ("step", C.c_int),
         ("rate", C.c_float), ("l2_reg", C.c_float)]


SRGNN_VARS = ("nasr_w1", "nasr_w2", "nasrv", "nasr_b", "embedding", "W_in", "b_in", "W_out", "b_out", "B", "gates_kernel",
              "gates_bias", "candidate_kernel", "candidate_bias")


class SrgnnWeights(C.Structure):
    """nrhip_srgnn_weights (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in SRGNN_VARS] + \
        [(n, C.c_int) for n in ("n_items", "d", "L", "step", "nonhybrid")]


class SrgnnFeed(C.Structure):
    """nrhip_srgnn_feed (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("seq", "target", "users", "ends", "seq_ptr", "seq_flat")] + \
        [("n_users", C.c_int)]


class SrgnnStepArgs(C.Structure):
    """nrhip_srgnn_step_args (include/neurec_hip.h)"""
    _fields_ = [("w", SrgnnWeights), ("f", SrgnnFeed)] + [("G_" + n, C.c_void_p) for n in SRGNN_VARS] + \
        [(n, C.c_void_p) for n in ("keys", "ws", "loss2")] + [("batch", C.c_int), ("l2", C.c_float)]


NEUMF_MAX_LAYERS = 4


class NeumfWeights(C.Structure):
    """nrhip_neumf_weights (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("mf_user", "mf_item", "mlp_user", "mlp_item")] + \
        [("kernel", C.c_void_p * NEUMF_MAX_LAYERS), ("bias", C.c_void_p * NEUMF_MAX_LAYERS)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "n_layers")] + [("width", C.c_int * NEUMF_MAX_LAYERS)]


class NeumfStepArgs(C.Structure):
    """nrhip_neumf_step_args (include/neurec_hip.h)"""
    _fields_ = [("w", NeumfWeights)] + \
        [(n, C.c_void_p) for n in ("G_mf_user", "G_mf_item", "G_mlp_user", "G_mlp_item")] + \
        [("G_kernel", C.c_void_p * NEUMF_MAX_LAYERS), ("G_bias", C.c_void_p * NEUMF_MAX_LAYERS)] + \
        [(n, C.c_void_p) for n in ("flag_mf_user", "flag_mf_item", "flag_mlp_user", "flag_mlp_item", "users", "items",
                                   "labels", "keys", "ws", "loss2")] + \
        [("batch", C.c_int), ("loss_kind", C.c_int), ("reg_mf", C.c_float), ("reg_mlp", C.c_float)]


class CdaeBatchArgs(C.Structure):
    """nrhip_cdae_batch_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "indptr", "indices", "users", "pos_ptr", "seg_off", "seg_len", "keys", "entry_ptr", "items", "labels", "slot",
        "in_items", "in_pos")] + [("n_draws", C.c_int64), ("seed", C.c_uint64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "batch", "num_neg", "max_draws")]


class CdaeStepArgs(C.Structure):
    """nrhip_cdae_step_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in (
        "user", "en", "offset", "de", "bias", "G_user", "G_en", "G_offset", "G_de", "G_bias", "flag_user", "flag_en",
        "flag_de", "flag_bias", "users", "entry_ptr", "items", "labels", "slot", "in_items", "in_pos", "keep", "keys",
        "g", "hidden", "dz", "scal", "l2", "loss2")] + [("seed", C.c_uint64), ("step", C.c_uint64)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "batch", "entry_cap", "act", "loss_kind", "keep_given")] + \
        [("keep_prob", C.c_float), ("reg", C.c_float)]


CONVNCF_MAX_LAYERS = 6


class ConvncfWeights(C.Structure):
    """nrhip_convncf_weights (include/neurec_hip.h)"""
    _fields_ = [("P", C.c_void_p), ("Q", C.c_void_p)] + \
        [("kernel", C.c_void_p * CONVNCF_MAX_LAYERS), ("bias", C.c_void_p * CONVNCF_MAX_LAYERS)] + \
        [("W", C.c_void_p), ("b", C.c_void_p)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "n_layers")] + [("channel", C.c_int * CONVNCF_MAX_LAYERS)]


class ConvncfStepArgs(C.Structure):
    """nrhip_convncf_step_args (include/neurec_hip.h)"""
    _fields_ = [("w", ConvncfWeights), ("G_P", C.c_void_p), ("G_Q", C.c_void_p)] + \
        [("G_kernel", C.c_void_p * CONVNCF_MAX_LAYERS), ("G_bias", C.c_void_p * CONVNCF_MAX_LAYERS)] + \
        [(n, C.c_void_p) for n in ("G_W", "G_b", "flag_P", "flag_Q", "users", "pos", "neg", "keys", "ws", "loss2")] + \
        [("batch", C.c_int), ("loss_kind", C.c_int), ("reg_embed", C.c_float), ("reg_head", C.c_float),
         ("reg_net", C.c_float)]


CFGAN_MAX_HIDDEN = 3


class CfganNet(C.Structure):
    """nrhip_cfgan_net (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p * (CFGAN_MAX_HIDDEN + 1)) for n in ("W", "b", "G_W", "G_b", "m_W", "m_b", "v_W", "v_b")] + \
        [("n_hidden", C.c_int), ("width", C.c_int * CFGAN_MAX_HIDDEN)]


class CfganStepArgs(C.Structure):
    """nrhip_cfgan_step_args (include/neurec_hip.h)"""
    _fields_ = [("gen", CfganNet), ("dis", CfganNet)] + \
        [(n, C.c_void_p) for n in ("indptr", "indices", "rows", "ent_ptr", "zr", "pm", "keys", "ws", "gemm_ws")] + \
        [("gemm_ws_bytes", C.c_size_t), ("loss3", C.c_void_p)] + \
        [(n, C.c_int) for n in ("n_rows", "n_cols", "batch", "n_ent", "max_batch")] + [("zr_coef", C.c_float)]


class IrganArgs(C.Structure):
    """nrhip_irgan_args (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("Pg", "Qg", "bg", "Pd", "Qd", "bd", "indptr", "indices", "z", "w", "draw_items",
                                          "draw_r", "hdr", "ws")] + [("ws_floats", C.c_size_t)] + \
        [(n, C.c_int) for n in ("n_users", "n_items", "d", "max_deg", "max_batch")] + \
        [(n, C.c_float) for n in ("lr", "g_reg", "d_reg")] + [("seed", C.c_uint64)]


DEEPICF_MAX_LAYERS = 4


class DeepicfTower(C.Structure):
    """nrhip_deepicf_tower (include/neurec_hip.h)"""
    _fields_ = [(n, C.c_void_p * DEEPICF_MAX_LAYERS) for n in ("W", "b", "gamma", "beta", "mm", "mv")] + \
        [("Wout", C.c_void_p), ("bout", C.c_void_p), ("n_layers", C.c_int), ("batch_norm", C.c_int),
         ("width", C.c_int * DEEPICF_MAX_LAYERS)]


class DeepicfStepArgs(C.Structure):
    """nrhip_deepicf_step_args (include/neurec_hip.h)"""
    _fields_ = [("nais", NaisStepArgs), ("tower", DeepicfTower)] + \
        [(n, C.c_void_p * DEEPICF_MAX_LAYERS) for n in ("G_W", "G_b", "G_gamma", "G_beta")] + \
        [("G_Wout", C.c_void_p), ("G_bout", C.c_void_p), ("ws", C.c_void_p), ("regs", C.c_float * 3),
         ("regw", C.c_float * DEEPICF_MAX_LAYERS), ("bessel", C.c_int)]


class DeepicfScoresArgs(C.Structure):
    """nrhip_deepicf_scores_args (include/neurec_hip.h)"""
    _fields_ = [("nais", NaisScoresArgs), ("wpad", C.c_void_p), ("n_layers", C.c_int), ("mfma", C.c_int),
                ("wtotal", C.c_int), ("tiles", C.c_int * (DEEPICF_MAX_LAYERS + 1))]


# name -> argtypes; every function returns int status except where noted.
SIGNATURES = {
    "nrhip_device_info": [C.POINTER(i32), C.POINTER(i32), psz, C.c_char_p, i32],
    "nrhip_eval_workspace_bytes": [i32, i32, psz],
    "nrhip_mask_train": [p, i64, p, i32, i32, p, p, p],
    "nrhip_eval_scores": [p, i64, i32, i32, p, p, p, C.POINTER(i32), i32, i32, p, p, p, p, sz, p],
    "nrhip_eval_any_k_workspace_bytes": [i32, i32, i32, psz],
    "nrhip_eval_scores_any_k": [p, i64, i32, i32, p, p, p, C.POINTER(i32), i32, i32, p, p, p, sz, p],
    "nrhip_arg_topk": [p, i64, i32, i32, i32, p, p, p, sz, p],
    "nrhip_colsum_workspace_bytes": [i32, i32, psz],
    "nrhip_colsum_f64": [p, i64, i32, i32, p, p, sz, p],
    "nrhip_score_gemm_workspace_bytes": [i32, i32, i32, psz],
    "nrhip_score_gemm_prepare_items": [p, i64, i32, i32, p, sz, p],
    "nrhip_score_tilemax": [p, i64, p, i32, i32, i32, p, p, p, i64, p, sz, p],
    "nrhip_tile_strike_plan": [p, p, i32, i32, p, p, p, p, p, p, p, sz, p],
    "nrhip_score_tilemax_fix": [p, i64, i32, i32, p, p, i32, p, p, p, p, i32, i32, p, i64, p, sz, p],
    "nrhip_score_filter_workspace_bytes": [i32, i32, i32, psz],
    "nrhip_score_filter_kappa": [i32, p],
    "nrhip_score_filter_prepare_items": [p, i64, i32, i32, p, sz, i32, p],
    "nrhip_score_filter_tilemax": [p, i64, p, i32, i32, i32, p, i64, p, p, sz, i32, p],
    "nrhip_score_filter_i8_workspace_bytes": [i32, i32, i32, psz],
    "nrhip_score_filter_i8_prepare_items": [p, i64, i32, i32, p, sz, i32, p],
    "nrhip_score_filter_i8_tilemax": [p, i64, p, i32, i32, i32, p, i64, p, p, sz, i32, p],
    "nrhip_eval_tiles_workspace_bytes": [i32, i32, psz],
    "nrhip_eval_tiles": [p, i64, p, i64, p, i32, p, i32, i32, p, p, p, p, p, i32, i32, p, p, p, sz, p],
    "nrhip_eval_tiles_bounded_workspace_bytes": [i32, i32, i32, i32, psz],
    "nrhip_eval_tiles_bounded": [p, i64, p, i32, p, i64, p, i32, p, i32, i32, p, p, p, p, p, i32, i32, p, p, p, sz, p],
    "nrhip_eval_pruned": [C.POINTER(EvalPrunedArgs), p],
    "nrhip_eval_redo": [C.POINTER(EvalRedoArgs), p],
    "nrhip_vae_step": [C.POINTER(VaeStepArgs), p, i32, f32, f32, f32, u64, i32, i32, p],
    "nrhip_score_gemm_items_kmajor": [p, i32, i32, p, p],
    "nrhip_score_gemm": [p, i64, p, i32, i32, i32, p, i64, p, sz, p],
    "nrhip_sample_bpr_epoch": [p, p, p, i64, i32, i32, u64, u64, i32, i64, i64, p, p, p, p],
    "nrhip_sample_instances_epoch": [p, p, p, p, p, p, p, i64, i32, i32, i32, i32, u64, u64, i32, i64, i64, p, p, p, p, p, p],
    "nrhip_randint_choice_batch": [i32, i32, i64, p, p, p, i32, u64, u64, p, p],
    "nrhip_bpr_plan": [p, p, p, i64, i32, i32, p, p],
    "nrhip_bpr_mf_grad": [p, p, i32, i32, p, p, p, i32, f32, p, p, p, p, p, p],
    "nrhip_adam_sparse_tf": [p, p, p, p, i64, f32, f32, f32, f32, p],
    "nrhip_adam_dense_tf": [p, p, p, p, i64, f32, f32, f32, f32, i32, p],
    "nrhip_adam_dense_tf2": [p, p, p, p, p, i64, f32, f32, f32, f32, p],
    "nrhip_adam_dense_tf_multi": [i32, p, p, p, p, p, p, f32, f32, f32, f32, p],
    "nrhip_rows_div": [p, i32, i32, p, f32, p, p],
    "nrhip_rows_clear": [p, i32, i32, p, p, p, p, p, p],
    "nrhip_spmm_plan_bytes": [i64, i64, psz],
    "nrhip_spmm_plan_create": [p, i64, i32, i32, i64, p, sz, p, C.POINTER(p)],
    "nrhip_spmm_plan_destroy": [p],
    "nrhip_spmm_plan_info": [p, C.POINTER(i64), C.POINTER(i64)],
    "nrhip_spmm_workspace_bytes": [p, i32, psz],
    "nrhip_spmm_csr": [p, p, p, p, p, i32, p, p, p, p, p, sz, p],
    "nrhip_spmm_csr_masked": [p, p, p, p, p, p, p, i32, p, p, p, p, p, sz, p],
    "nrhip_spmm_csr_carry": [p, p, p, p, p, p, i32, i32, p, i32, p, p],
    "nrhip_spmm_chunks_finish": [p, i64, p, i32, p, p, p, p, p, p],
    "nrhip_partials_sum_rows": [p, i32, i64, i32, p, p, p, p, p, p],
    "nrhip_spmm_csr_rows": [p, p, p, p, i32, p, i32, p, p, p, p, p],
    "nrhip_lightgcn_mark_batch": [p, p, p, i32, i32, p, p, p],
    "nrhip_lightgcn_bpr_grad": [p, p, i32, i32, i32, p, p, p, i32, f32, p, p, p, p, p, p],
    "nrhip_lightgcn_bpr_grad_h": [p, p, i32, i32, i32, p, p, p, i32, f32, p, p, p, p, p, p],
    "nrhip_lightgcn_ctx_create": [C.POINTER(LightGCNBuffers), C.POINTER(p)],
    "nrhip_lightgcn_ctx_destroy": [p],
    "nrhip_lightgcn_step": [p, p, p, p, i32, p, f32, f32, f32, f32, p, p],
    "nrhip_lightgcn_step_grad": [p, p, p, p, i32, p, p, p, p],
    "nrhip_lightgcn_step_apply": [p, p, f32, f32, f32, f32, p],
    "nrhip_mf_ctx_create": [C.POINTER(MFBuffers), C.POINTER(p)],
    "nrhip_mf_ctx_destroy": [p],
    "nrhip_mf_step": [p, p, p, p, i32, p, p, i32, i32, f32, f32, f32, f32, p, p],
    "nrhip_mf_flush": [p, i32, f32, f32, f32, p],
    "nrhip_ngcf_ctx_create": [C.POINTER(NGCFBuffers), C.POINTER(p)],
    "nrhip_ngcf_ctx_destroy": [p],
    "nrhip_ngcf_forward": [p, C.c_uint64, C.c_uint64, i32, p],
    "nrhip_ngcf_step": [p, p, p, p, i32, p, C.c_uint64, C.c_uint64, i32, f32, f32, f32, f32, p, p],
    "nrhip_mf_steps": [p, p, p, p, i64, i32, p, i32, p, f32, f32, f32, p, p, p],
    "nrhip_loss_reduce_steps": [p, i32, i32, i32, f32, p, p],
    "nrhip_lightgcn_step_colshard_fwd": [p, p, p, p, i32, p, p],
    "nrhip_lightgcn_step_colshard_fwd_planned": [p, p, p, p, i32, p, i32, p, p],
    "nrhip_lightgcn_step_planned": [p, p, p, p, i32, p, p, i32, f32, f32, f32, f32, p, p],
    "nrhip_lightgcn_step_colshard_bwd": [p, p, p, p, i32, p, p, f32, f32, f32, f32, p, p],
    "nrhip_lightgcn_partial_dots": [p, p, i32, i32, i32, p, p, p, i32, p, p],
    "nrhip_partials_sum": [p, i32, i32, p, p],
    "nrhip_lightgcn_bpr_grad_given": [p, p, i32, i32, i32, p, p, p, i32, f32, p, p, p, p, p, p, i32, p],
    "nrhip_gemm_workspace_bytes": [i32, i32, i32, p],
    "nrhip_gemm_kmajor": [p, i64, p, i64, i32, i32, i32, p, i64, i32, p, i32, i32, p, sz, p],
    "nrhip_gemm_f32": [p, i64, i32, p, i64, i32, i32, i32, i32, p, i64, i32, p, i32, i32, p, sz, p],
    "nrhip_transpose2d": [p, i64, i32, i32, p, i64, p],
    "nrhip_ngcf_wide_forward": [C.POINTER(NGCFWideBuffers), i32, u64, u64, p],
    "nrhip_ngcf_wide_step": [C.POINTER(NGCFWideBuffers), p, p, p, i32, p, i32, u64, u64, f32, f32, f32, f32, p, p],
    "nrhip_vae_bag_fwd": [p, p, p, i32, i32, p, p, i32, f32, p, u64, u64, p, p, p],
    "nrhip_act_bwd": [p, p, i64, i32, p, p],
    "nrhip_vae_sample": [p, i32, i32, p, f32, u64, u64, p, p, p, p],
    "nrhip_vae_sample_bwd": [p, p, p, i32, i32, f32, p, p],
    "nrhip_vae_softmax_dlogits": [p, i64, i32, i32, p, p, p, p, p],
    "nrhip_vae_dwq0_wide": [p, p, p, i32, i32, p, p, p, p],
    "nrhip_colsum_rows": [p, i64, i32, i32, p, p, sz, p],
    "nrhip_ew_mul": [p, i64, p, i64, i64, i32, p, i64, p],
    "nrhip_ngcf_act_fwd": [p, p, i64, i64, i32, i32, f32, p, i32, u64, u64, i32, p, i64, p, i64, p],
    "nrhip_ngcf_act_bwd": [p, i64, p, i64, p, i64, p, p, i64, p, i64, i32, f32, p, p, p],
    "nrhip_lrelu_drop_fwd": [p, i64, i64, i32, i32, f32, p, i32, u64, u64, i32, i32, p, i64, p, i64, p],
    "nrhip_lrelu_drop_bwd": [p, i64, p, i64, p, i64, p, i64, i32, f32, i32, p, p],
    "nrhip_edge_dropout": [p, i64, f32, p, i32, u64, u64, p, p],
    "nrhip_gather_f32": [p, p, i64, p, p],
    "nrhip_ngcf_mix_bwd": [p, p, i64, p, p, i64, i64, i32, i32, p, p, p],
    "nrhip_route_batch": [p, p, p, i32, i32, i32, i32, i32, p, p, p, p, p, i32, p],
    "nrhip_route_owner_keys": [p, p, i32, p, p, i32, i32, i32, p, p, p],
    "nrhip_sort_u64_segments": [p, p, p, i32, i32, p],
    "nrhip_route_epoch": [p, p, p, i64, i32, i32, i32, i32, i32, i32, p, p, p, p, p, p, p, p],
    "nrhip_route_epoch_owner_keys": [p, p, p, i64, p, p, i32, i32, p, p, p, i32, i32, i64, p, p, p],
    "nrhip_bpr_mf_step_fused": [p, p, p, p, p, p, i32, f32, f32, f32, i32, i32, i32, p, p, p, i32, f32, p, p, p,
                                i32, p, i32, i32, p],
    "nrhip_bpr_mf_fused_flush": [p, p, p, p, p, i32, f32, f32, f32, i32, i64, p],
    "nrhip_adam_sparse_tf_lazy": [p, p, p, p, p, p, i64, i32, p, i32, p, i32, p, i32, i32, f32, f32, f32, p],
    "nrhip_bpr_mf_grad_lazy": [p, p, p, p, p, p, i32, f32, f32, f32, i32, i32, p, p, p, i32, f32, p, p, p,
                               p, p],
    "nrhip_ngcf_workspace_bytes": [i64, psz],
    "nrhip_ngcf_layer_fwd": [p, p, p, p, p, p, i64, i32, f32, p, i32, u64, u64, i32, p, p, i64, p],
    "nrhip_ngcf_layer_bwd": [p, p, p, p, p, p, i64, i32, f32, p, p, i64, p, p, p, p, p, p, p, p, p,
                             p, sz, p],
    "nrhip_spmm_blocked_plan_bytes": [i64, i64, i32, psz],
    "nrhip_spmm_blocked_pack": [p, p, p, p],
    "nrhip_spmm_blocked_pack_factored": [p, p, p, p, p, i64, p, C.POINTER(i32)],
    "nrhip_spmm_blocked_is_packed": [p],
    "nrhip_spmm_blocked_tune_packed": [i32],
    "nrhip_spmm_blocked_plan_create": [p, p, i64, i64, i32, i64, i32, i32, i32, i32, i32, p, sz, p,
                                       C.POINTER(p)],
    "nrhip_spmm_blocked_plan_destroy": [p],
    "nrhip_spmm_blocked_plan_info": [p, p, p, p, p],
    "nrhip_spmm_blocked_tune": [i32],
    "nrhip_spmm_blocked_tune_store": [i32],
    "nrhip_spmm_blocked": [p, p, p, p, p, p, p, p, p, p, p],
    "nrhip_spmm_blocked_flagged": [p, p, p, p, p, p, p, p, p, p, p, p],
    "nrhip_spmm_csr_flagged": [p, p, p, p, p, i32, p, p, p, p, p, p, sz, p],
    "nrhip_spmm_blocked_tune_addend_flag": [i32],
    "nrhip_spmm_plan_attach_blocked": [p, p, i32],
    "nrhip_spmm_plan_has_blocked": [p, i32],
    "nrhip_spmm_plan_has_wanted": [p, i32],
    "nrhip_spmm_blocked_has_wanted": [p],
    "nrhip_spmm_plan_has_wanted_planned": [p, i32],
    "nrhip_spmm_blocked_has_wanted_planned": [p],
    "nrhip_spmm_wanted_epoch_plan_bytes": [p, i32, i32, i64, psz, C.POINTER(i32)],
    "nrhip_spmm_blocked_wanted_epoch_plan_bytes": [p, i32, i64, psz, C.POINTER(i32)],
    "nrhip_spmm_wanted_epoch_plan": [p, i32, p, p, i32, i64, i32, p, sz, p],
    "nrhip_spmm_blocked_wanted_epoch_plan": [p, p, p, i32, i64, i32, p, sz, p],
    "nrhip_spmm_csr_wanted_planned": [p, p, p, p, i32, p, p, p, p, p, p, p, i32, i32, p, p, p, i32, p],
    "nrhip_spmm_blocked_wanted_planned": [p, p, p, p, p, p, p, p, p, p, p, i32, i32, p, p, p, i32, p],
    "nrhip_spmm_csr_wanted_layers": [p, p, p, p, i32, p, p, p, p, p, p],
    "nrhip_spmm_blocked_wanted_layers": [p, p, p, p, p, p, p, p, p, p],
    "nrhip_spmm_csr_wanted_batch": [p, p, p, p, i32, p, p, p, p, p, p, p, i32, i32, p, p, p],
    "nrhip_spmm_blocked_wanted_batch": [p, p, p, p, p, p, p, p, p, p, p, i32, i32, p, p, p],
    "nrhip_spmm_csr_adam": [p, p, p, p, i32, p, p, p, p, p, f32, f32, f32, f32, i32, p, p],
    "nrhip_spmm_blocked_adam": [p, p, p, p, p, p, p, p, p, f32, f32, f32, f32, i32, p, p],
    "nrhip_vae_encode": [p, p, p, i32, i32, i32, p, p, p, p, p, p, i32, f32, p, p, f32, u64, u64,
                         p, p, p, p, p, p, p, p, p],
    "nrhip_add_row_bias": [p, i64, i32, i32, p, p],
    "nrhip_vae_workspace_bytes": [i32, i32, psz],
    "nrhip_vae_decoder_loss_grad": [p, i64, i32, i32, i32, p, p, p, p, p, p, p, p, p, p, p, sz, p],
    "nrhip_vae_decoder_fused_workspace_bytes": [i32, i32, psz],
    "nrhip_vae_decoder_fused": [i32, i32, i32, p, p, p, p, p, p, p, p, p, p, p, sz, p, p],
    "nrhip_vae_mid_backward": [i32, i32, i32, i32, f32, p, p, p, p, p, p, p, p, p, p, p, p, p, p,
                               p, p, p, p],
    "nrhip_vae_dwq0": [p, p, p, i32, i32, p, p, p, p],
    "nrhip_axpy": [f32, p, p, i64, p],
    "nrhip_sumsq_accumulate": [p, i64, p, p],
    "nrhip_mean_f32": [p, i32, p, p],
    "nrhip_mean2_f32": [p, p, i32, p, p],
    "nrhip_pairwise_mf_grad": [p, p, i32, i32, p, p, p, i32, f32, i32, p, p, p, p, p, p],
    "nrhip_pointwise_mf_grad": [p, p, i32, i32, p, p, p, i32, f32, i32, p, p, p, p, p, p],
    "nrhip_gather_u8": [p, p, i64, p, p],
    "nrhip_mark_rows": [p, i32, i32, p, p],
    "nrhip_sort_u64": [p, i32, p],
    "nrhip_rows_sum_sorted": [p, i32, p, i32, p, i64, p, p],
    "nrhip_rows_sum_sorted2": [p, i32, p, i32, p, i64, p, p, i64, p, p],
    "nrhip_optimizer_rows_tf": [i32, p, p, p, p, p, i64, i32, f32, f32, f32, f32, p],
    "nrhip_optimizer_dense_tf": [i32, p, p, p, p, i64, f32, f32, f32, f32, i32, p],
    "nrhip_rows_gather": [p, i32, i32, p, p, i64, p],
    "nrhip_rows_gather_ld": [p, i32, i32, p, i64, p, i64, p],
    "nrhip_rows_gather2": [p, i32, i32, p, i64, p, i64, p, i64, p, i64, p],
    "nrhip_rows_scatter_add": [p, i32, i32, p, i64, p, p],
    "nrhip_scale": [p, f32, p, i64, p],
    "nrhip_add": [p, p, p, i64, p],
    "nrhip_div_scalar": [p, f32, p, i64, p],
    "nrhip_add2d": [p, i64, p, i64, p, i64, i64, i32, p],
    "nrhip_copy2d": [p, i64, p, i64, i64, i32, p],
    "nrhip_wrmf_chunk_plan": [p, i32, p, p, C.POINTER(i32)],
    "nrhip_wrmf_workspace_bytes": [i32, i32, psz],
    "nrhip_wrmf_gram": [p, i32, i32, p, p, sz, p],
    "nrhip_wrmf_solve": [p, p, i32, p, i32, p, i32, f32, f32, p, p, i32, p, p, sz, p],
    "nrhip_itemknn_workspace_bytes": [i32, i32, i32, psz],
    "nrhip_itemknn_build": [p, p, p, p, p, p, p, p, i32, i32, i32, f32, f32, f32, i32, i32, p, p, p, p, p, p, p, sz, p],
    "nrhip_itemknn_score": [p, i32, p, p, p, i32, i32, p, p, p, p, i64, p],
    "nrhip_fism_step": [C.POINTER(FismStepArgs), p],
    "nrhip_fism_user_factors": [p, p, i32, p, i32, f32, p, i32, p, i64, p],
    "nrhip_nais_step": [C.POINTER(NaisStepArgs), p],
    "nrhip_nais_scores": [C.POINTER(NaisScoresArgs), p],
    "nrhip_fpmc_step": [C.POINTER(FpmcStepArgs), p],
    "nrhip_fpmc_user_factors": [p, p, i32, i32, i32, p, p, i32, p, i64, p],
    "nrhip_fossil_step": [C.POINTER(FossilStepArgs), p],
    "nrhip_fossil_user_factors": [p, p, i32, i32, p, p, p, p, i32, i32, f32, p, i32, p, i64, p],
    "nrhip_hrm_step": [C.POINTER(HrmStepArgs), p],
    "nrhip_hrm_user_factors": [p, p, i32, i32, i32, i32, i32, i32, p, p, i32, p, i64, p],
    "nrhip_npe_step": [C.POINTER(NpeStepArgs), p],
    "nrhip_npe_user_factors": [p, p, i32, i32, i32, i32, p, p, i32, p, i64, p],
    "nrhip_npe_item_factors": [p, i32, i32, p, p],
    "nrhip_fpmcplus_step": [C.POINTER(FpmcplusStepArgs), p],
    "nrhip_fpmcplus_scores": [C.POINTER(FpmcplusScoresArgs), p],
    "nrhip_transrec_step": [C.POINTER(TransrecStepArgs), p],
    "nrhip_transrec_queries": [p, p, p, i32, i32, i32, p, p, i32, p, i64, p],
    "nrhip_transrec_scores": [p, i64, p, p, i32, i32, i32, p, i64, p],
    "nrhip_gru4rec_workspace_floats": [i32, C.POINTER(i32), i32, psz],
    "nrhip_gru4rec_step": [C.POINTER(Gru4recStepArgs), p],
    "nrhip_gru4rec_advance": [C.POINTER(p), C.POINTER(p), C.POINTER(i32), i32, i32, p, p],
    "nrhip_gru4rec_user_states": [p, p, i32, i32, p, p, i32, p, C.POINTER(Gru4recWeights), p, i64, p],
    "nrhip_gru4rec_scores": [p, i64, p, p, i32, i32, i32, i32, p, i64, p],
    "nrhip_gru4recplus_workspace_floats": [i32, C.POINTER(i32), i32, i32, psz],
    "nrhip_gru4recplus_step": [C.POINTER(Gru4recplusStepArgs), p],
    "nrhip_sasrec_workspace_floats": [i32, i32, i32, i32, i32, psz],
    "nrhip_sasrec_step": [C.POINTER(SasrecStepArgs), p],
    "nrhip_sasrec_forward": [C.POINTER(SasrecWeights), p, i32, p, C.c_float, p, i64, p],
    "nrhip_caser_workspace_floats": [i32, i32, i32, i32, i32, i32, i32, psz],
    "nrhip_caser_step": [C.POINTER(CaserStepArgs), p],
    "nrhip_caser_forward": [C.POINTER(CaserWeights), p, p, i32, p, p, i64, p],
    "nrhip_caser_scores": [p, i64, p, i32, i32, i32, p, i64, p],
    "nrhip_srgnn_workspace_floats": [i32, i32, i32, i32, i32, psz],
    "nrhip_srgnn_step": [C.POINTER(SrgnnStepArgs), p],
    "nrhip_srgnn_forward": [C.POINTER(SrgnnWeights), C.POINTER(SrgnnFeed), i32, p, p, i64, p],
    "nrhip_neumf_workspace_floats": [C.POINTER(NeumfWeights), i32, psz],
    "nrhip_neumf_step": [C.POINTER(NeumfStepArgs), p],
    "nrhip_neumf_forward": [C.POINTER(NeumfWeights), p, p, i32, p, p],
    "nrhip_neumf_scores_workspace_floats": [C.POINTER(NeumfWeights), i32, psz],
    "nrhip_neumf_scores": [C.POINTER(NeumfWeights), p, i32, p, p, i64, p],
    "nrhip_cdae_batch": [C.POINTER(CdaeBatchArgs), p],
    "nrhip_cdae_step": [C.POINTER(CdaeStepArgs), p],
    "nrhip_cdae_user_factors": [p, p, i32, i32, p, p, p, i32, i32, p, p, i32, p, i32, f32, u64, u64, p, i64, p],
    "nrhip_cdae_pairs": [p, i64, p, p, i32, i32, p, p, i64, p, p],
    "nrhip_deepicf_workspace_floats": [C.POINTER(DeepicfTower), i32, i32, psz],
    "nrhip_deepicf_step": [C.POINTER(DeepicfStepArgs), p],
    "nrhip_deepicf_scores": [C.POINTER(DeepicfScoresArgs), p],
    "nrhip_convncf_workspace_floats": [C.POINTER(ConvncfWeights), i32, psz],
    "nrhip_convncf_step": [C.POINTER(ConvncfStepArgs), p],
    "nrhip_convncf_pairs": [C.POINTER(ConvncfWeights), p, p, i32, p, p],
    "nrhip_convncf_scores": [C.POINTER(ConvncfWeights), p, i32, p, i64, p],
    "nrhip_cfgan_workspace": [C.POINTER(CfganStepArgs), psz, psz],
    "nrhip_cfgan_masks": [p, p, p, p, i32, i32, i32, u64, u64, p, p, p],
    "nrhip_cfgan_d_step": [C.POINTER(CfganStepArgs), p],
    "nrhip_cfgan_g_step": [C.POINTER(CfganStepArgs), p],
    "nrhip_cfgan_apply": [C.POINTER(CfganNet), i32, i32, i32, f32, f32, f32, f32, f32, p, p, p],
    "nrhip_cfgan_hidden": [C.POINTER(CfganNet), p, p, p, i32, i32, p, p, i64, p],
    "nrhip_cfgan_pairs": [p, i64, p, i64, i32, p, p, i64, p, p],
    "nrhip_irgan_workspace": [i32, i32, i32, psz],
    "nrhip_irgan_weights": [p, i64, i32, i32, C.c_double, p],
    "nrhip_irgan_draws": [p, i64, i32, i32, p, p, p, p, i32, u64, u64, p, p, p, p],
    "nrhip_irgan_d_pass": [C.POINTER(IrganArgs), p, p, p, p, i64, i32, p, p],
    "nrhip_irgan_g_pass": [C.POINTER(IrganArgs), p, i32, p, u64, p],
    "nrhip_sbpr_expansion_sizes": [p, p, p, i32, p, p],
    "nrhip_sbpr_sets_block": [C.POINTER(SbprSetsArgs), p],
    "nrhip_sbpr_stream": [C.POINTER(SbprStreamArgs), p],
    "nrhip_sbpr_step": [C.POINTER(SbprStepArgs), p],
    "nrhip_jca_workspace": [i32, i32, i32, i32, i32, p],
    "nrhip_jca_pairs": [C.POINTER(JcaArgs), p],
    "nrhip_jca_step": [C.POINTER(JcaArgs), p],
    "nrhip_jca_apply": [C.POINTER(JcaArgs), i32, C.c_float, C.c_float, C.c_float, C.c_float, p],
    "nrhip_jca_encode": [C.POINTER(JcaArgs), i32, p, i32, p, p],
    "nrhip_jca_score": [C.POINTER(JcaArgs), p, i32, p, p, p, i64, p],
    "nrhip_jca_score_pairs": [C.POINTER(JcaArgs), p, p, p, i64, p, p, p, p],
    "nrhip_apr_step": [C.POINTER(AprStepArgs), p],
}

for _name, _args in SIGNATURES.items():
    _fn = getattr(lib, _name)          # AttributeError here == ABI mismatch: fail loudly
    _fn.argtypes = _args
    _fn.restype = C.c_int
lib.nrhip_abi_version.argtypes = []
lib.nrhip_abi_version.restype = C.c_int
lib.nrhip_last_error.argtypes = []
lib.nrhip_last_error.restype = C.c_char_p

EXPORTED = sorted(list(SIGNATURES) + ["nrhip_abi_version", "nrhip_last_error"])

ABI_VERSION = 4      # 2: deterministic row-gradient sums (batch plans); 3: one-launch BPR-MF step (mf_buffers.tw);
                     # 4: nrhip_mf_steps takes a per-step terms buffer (one loss reduction per call)
if lib.nrhip_abi_version() != ABI_VERSION:  # pragma: no cover
    raise ImportError("libneurec_hip.so ABI version %d, expected %d"
                      % (lib.nrhip_abi_version(), ABI_VERSION))


def last_error():
    return lib.nrhip_last_error().decode("utf-8", "replace")


def check(rc):
    """Translate a status code into the exception type the reference would raise."""
    if rc == 0:
        return
    msg = last_error()
    if rc == ERR_ARG:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise NeuRecHipError("libneurec_hip status %d: %s" % (rc, msg))


def call(name, *args):
    check(getattr(lib, name)(*args))


def is_stale():
    """True when the .so on disk was built from different sources than the tree holds."""
    return not _build.is_current()
