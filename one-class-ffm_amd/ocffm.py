"""Python mirror of the reference's C++ interface over the C ABI (include/ocffm.h).

Names follow the reference (``ffm.h:42-154``): ``Parameter``, ``ImpData``,
``ImpProblem`` with ``init``, ``one_epoch``, ``solve``, ``validate`` and
``save_model``.  Every call runs the HIP path in ``libocffm.so``; there is no
CPU fallback: if the library or a GPU is missing, calls raise ``OcffmError``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

try:  # one HIP runtime per process: let torch's libamdhip64 load first if present
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the library itself
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCFFM_LIB") or os.path.join(HERE, "libocffm.so")  # override: experiment builds

OK, E_ARG, E_IO, E_DATA, E_HIP, E_COMM, E_STATE = range(7)
FP64, FP32 = 64, 32
REC_MAX_TOPN, REC_EXCLUDE_LABELS, REC_NONE = 128, 1, 0xFFFFFFFF
RANK_NONE, EVAL_MAX_CUTS = 0xFFFFFFFF, 8
SIM_DOT, SIM_KEEP_SELF = 1, 2
DIV_MAX_POOL = REC_MAX_TOPN
COMM_ID_BYTES = 128


class OcffmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[ocffm error {code}] {msg}")
        self.code = code


class _Param(C.Structure):
    _fields_ = [("omega", C.c_double), ("lambda_", C.c_double), ("r", C.c_double),
                ("nr_pass", C.c_uint32), ("k", C.c_uint32), ("nr_threads", C.c_uint32),
                ("self_side", C.c_int32), ("freq", C.c_int32), ("precision", C.c_int32),
                ("device", C.c_int32)]


class _Info(C.Structure):
    _fields_ = [("m", C.c_uint64), ("n", C.c_uint64), ("f", C.c_uint64), ("nnz_x", C.c_uint64),
                ("nnz_y", C.c_uint64)]


class _Metrics(C.Structure):
    _fields_ = [("loss", C.c_double), ("prec", C.c_double * 5), ("ndcg", C.c_double * 5),
                ("top_k", C.c_uint32 * 5)]


class _Eval(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("rows_used", C.c_uint64), ("labels", C.c_uint64),
                ("labels_ranked", C.c_uint64), ("ncut", C.c_uint32), ("cuts", C.c_uint32 * 8),
                ("loss", C.c_double), ("mrr", C.c_double), ("auc", C.c_double), ("prec", C.c_double * 8),
                ("recall", C.c_double * 8), ("ndcg", C.c_double * 8), ("map", C.c_double * 8),
                ("hit", C.c_double * 8)]

    def as_dict(self) -> dict:
        nc = int(self.ncut)
        d = dict(rows=int(self.rows), rows_used=int(self.rows_used), labels=int(self.labels),
                 labels_ranked=int(self.labels_ranked), cuts=list(self.cuts[:nc]), loss=self.loss, mrr=self.mrr,
                 auc=self.auc)
        for key in ("prec", "recall", "ndcg", "map", "hit"):
            d[key] = np.array(getattr(self, key)[:nc])
        return d


class _Objective(C.Structure):
    _fields_ = [("value", C.c_double), ("pos", C.c_double), ("on_pos", C.c_double), ("all", C.c_double),
                ("reg", C.c_double), ("m", C.c_uint64), ("n", C.c_uint64), ("labels", C.c_uint64)]


class _SolveOpts(C.Structure):
    _fields_ = [("objective_every", C.c_uint32), ("tol", C.c_double), ("min_pass", C.c_uint32)]


class _SolveReport(C.Structure):
    _fields_ = [("epochs", C.c_uint32), ("converged", C.c_int32), ("objective0", C.c_double),
                ("objective", C.c_double)]


class _KStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint64), ("total_ms", C.c_double),
                ("alg_bytes", C.c_double), ("alg_flops", C.c_double)]


class _ModelInfo(C.Structure):
    _fields_ = [("f", C.c_uint32), ("fu", C.c_uint32), ("fv", C.c_uint32), ("k", C.c_uint32), ("kp", C.c_uint32),
                ("nblocks", C.c_uint32), ("nused", C.c_uint32), ("self_side", C.c_int32),
                ("precision", C.c_int32), ("device", C.c_int32), ("has_items", C.c_int32),
                ("n", C.c_uint64), ("npop", C.c_uint64), ("Ds", C.c_void_p), ("used", C.c_void_p),
                ("ds_cap", C.c_uint32), ("used_cap", C.c_uint32)]


class _Fold(C.Structure):
    _fields_ = [("field", C.c_uint32), ("omega", C.c_double), ("lambda_", C.c_double), ("r", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p)

EXPORTS = [
    "ocffm_param_default", "ocffm_last_error", "ocffm_device_count", "ocffm_data_read",
    "ocffm_data_from_rows", "ocffm_data_trans_y", "ocffm_data_get_info", "ocffm_data_get_ds",
    "ocffm_data_get_labels", "ocffm_data_get_field", "ocffm_data_free", "ocffm_problem_create", "ocffm_comm_id", "ocffm_problem_create_dist",
    "ocffm_problem_create_dist_host", "ocffm_problem_init", "ocffm_problem_one_epoch",
    "ocffm_problem_solve_block", "ocffm_problem_cache_sasb", "ocffm_problem_solve",
    "ocffm_problem_objective", "ocffm_problem_solve_ex",
    "ocffm_problem_validate", "ocffm_print_header", "ocffm_print_epoch", "ocffm_problem_get",
    "ocffm_problem_set", "ocffm_problem_grad", "ocffm_problem_hv", "ocffm_problem_save_model",
    "ocffm_problem_validate_forced", "ocffm_problem_test_rows", "ocffm_problem_save_binary", "ocffm_problem_load_binary",
    "ocffm_problem_recommend", "ocffm_problem_label_ranks", "ocffm_eval_from_ranks", "ocffm_problem_evaluate",
    "ocffm_problem_score", "ocffm_problem_recommend_among", "ocffm_problem_label_ranks_among",
    "ocffm_problem_evaluate_among",
    "ocffm_problem_cg_log", "ocffm_problem_set_profiling", "ocffm_problem_set_profile_filter",
    "ocffm_problem_kernel_stats",
    "ocffm_problem_reset_stats", "ocffm_problem_alg_bytes", "ocffm_problem_counter", "ocffm_problem_sync",
    "ocffm_problem_layout_digest", "ocffm_problem_destroy",
    "ocffm_sgd_param_default", "ocffm_sgd_create", "ocffm_sgd_create_dist", "ocffm_sgd_create_dist_host", "ocffm_sgd_epoch",
    "ocffm_sgd_average", "ocffm_sgd_phi", "ocffm_sgd_get", "ocffm_sgd_set_w", "ocffm_sgd_get_info",
    "ocffm_sgd_sync", "ocffm_sgd_destroy",
    "ocffm_sgd_recommend", "ocffm_sgd_label_ranks", "ocffm_sgd_evaluate", "ocffm_sgd_counter",
    "ocffm_sgd_score", "ocffm_sgd_recommend_among", "ocffm_sgd_label_ranks_among", "ocffm_sgd_evaluate_among",
    "ocffm_model_file_info", "ocffm_model_load_text", "ocffm_model_load_binary", "ocffm_model_from_problem",
    "ocffm_model_set_items", "ocffm_model_set_popularity", "ocffm_model_recommend", "ocffm_model_score",
    "ocffm_model_recommend_among", "ocffm_model_label_ranks", "ocffm_model_label_ranks_among",
    "ocffm_model_evaluate", "ocffm_model_evaluate_among", "ocffm_model_counter", "ocffm_model_get_info",
    "ocffm_model_get_ds", "ocffm_model_get", "ocffm_model_destroy",
]
# include/ocffm_fold.h (included by ocffm.h): the fold entries of a model
FOLD_EXPORTS = [
    "ocffm_model_fold_in", "ocffm_model_recommend_fold", "ocffm_model_label_ranks_fold", "ocffm_model_evaluate_fold",
]
# include/ocffm_similar.h (included by ocffm.h): items like this one, on a model
SIMILAR_EXPORTS = ["ocffm_model_similar_items", "ocffm_model_similar_to", "ocffm_model_item_similarity"]
# include/ocffm_diverse.h (included by ocffm.h): diversified top-N, on a model
DIVERSE_EXPORTS = ["ocffm_model_recommend_diverse"]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OcffmError(E_STATE, f"{LIB_PATH} not built (run __graft_entry__.build() or make -C one-class-ffm_amd)")
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32, dbl = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
    L.ocffm_last_error.restype = C.c_char_p
    L.ocffm_param_default.argtypes = [C.POINTER(_Param)]
    L.ocffm_device_count.argtypes = [C.POINTER(C.c_int)]
    L.ocffm_data_read.argtypes = [C.c_char_p, i32, vp, u32, C.POINTER(vp)]
    L.ocffm_data_from_rows.argtypes = [u64, vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(vp)]
    L.ocffm_data_trans_y.argtypes = [vp, vp]
    L.ocffm_data_get_info.argtypes = [vp, C.POINTER(_Info)]
    L.ocffm_data_get_ds.argtypes = [vp, vp]
    L.ocffm_data_get_labels.argtypes = [vp, vp, vp]
    L.ocffm_data_get_field.argtypes = [vp, u32, vp, vp, vp, vp]
    L.ocffm_data_free.argtypes = [vp]
    L.ocffm_data_free.restype = None
    L.ocffm_problem_create.argtypes = [vp, vp, vp, C.POINTER(_Param), C.POINTER(vp)]
    L.ocffm_comm_id.argtypes = [vp]
    L.ocffm_problem_create_dist.argtypes = [vp, vp, vp, C.POINTER(_Param), i32, i32, vp, C.POINTER(vp)]
    L.ocffm_problem_create_dist_host.argtypes = [vp, vp, vp, C.POINTER(_Param), i32, i32, ALLREDUCE_FN, vp,
                                                 C.POINTER(vp)]
    for name in ("ocffm_problem_init", "ocffm_problem_one_epoch", "ocffm_problem_cache_sasb",
                 "ocffm_problem_solve", "ocffm_problem_reset_stats", "ocffm_problem_sync"):
        getattr(L, name).argtypes = [vp]
    L.ocffm_problem_solve_block.argtypes = [vp, u32, u32]
    L.ocffm_problem_validate.argtypes = [vp, C.POINTER(_Metrics)]
    L.ocffm_problem_objective.argtypes = [vp, C.POINTER(_Objective)]
    L.ocffm_problem_solve_ex.argtypes = [vp, C.POINTER(_SolveOpts), C.POINTER(_SolveReport)]
    L.ocffm_print_epoch.argtypes = [C.POINTER(_Metrics), u32]
    L.ocffm_problem_get.argtypes = [vp, C.c_char, u32, vp, u64, C.POINTER(u64)]
    L.ocffm_problem_set.argtypes = [vp, C.c_char, u32, vp, u64]
    L.ocffm_problem_grad.argtypes = [vp, u32, u32, i32, vp]
    L.ocffm_problem_hv.argtypes = [vp, u32, u32, i32, vp, vp]
    L.ocffm_problem_save_model.argtypes = [vp, C.c_char_p]
    L.ocffm_problem_validate_forced.argtypes = [vp, C.POINTER(_Metrics), vp, u64]
    L.ocffm_problem_test_rows.argtypes = [vp, C.POINTER(u64)]
    L.ocffm_problem_recommend.argtypes = [vp, vp, u64, u64, u32, u32, vp, vp]
    L.ocffm_problem_label_ranks.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ocffm_problem_score.argtypes = [vp, vp, u64, vp, vp, vp]
    L.ocffm_problem_recommend_among.argtypes = [vp, vp, u64, u64, vp, vp, u32, u32, vp, vp]
    L.ocffm_eval_from_ranks.argtypes = [u64, vp, vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_problem_evaluate.argtypes = [vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_problem_label_ranks_among.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ocffm_problem_evaluate_among.argtypes = [vp, vp, vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_problem_save_binary.argtypes = [vp, C.c_char_p]
    L.ocffm_problem_load_binary.argtypes = [vp, C.c_char_p]
    L.ocffm_problem_cg_log.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.ocffm_problem_set_profiling.argtypes = [vp, i32]
    L.ocffm_problem_set_profile_filter.argtypes = [vp, C.c_char_p]
    L.ocffm_problem_kernel_stats.argtypes = [vp, C.POINTER(_KStat), i32, C.POINTER(C.c_int)]
    L.ocffm_problem_alg_bytes.argtypes = [vp, C.POINTER(dbl)]
    L.ocffm_problem_counter.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.ocffm_problem_layout_digest.argtypes = [vp, vp, vp, i32, C.POINTER(C.c_int)]
    L.ocffm_problem_destroy.argtypes = [vp]
    L.ocffm_problem_destroy.restype = None
    L.ocffm_sgd_param_default.argtypes = [vp]
    L.ocffm_sgd_param_default.restype = None
    L.ocffm_sgd_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.ocffm_sgd_create_dist.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(vp)]
    L.ocffm_sgd_create_dist_host.argtypes = [vp, vp, vp, i32, i32, ALLREDUCE_FN, vp, C.POINTER(vp)]
    L.ocffm_sgd_epoch.argtypes = [vp, C.POINTER(dbl)]
    L.ocffm_sgd_average.argtypes = [vp]
    L.ocffm_sgd_phi.argtypes = [vp, u64, vp, vp, vp]
    L.ocffm_sgd_get.argtypes = [vp, C.c_char, vp, u64, C.POINTER(u64)]
    L.ocffm_sgd_set_w.argtypes = [vp, vp, u64]
    L.ocffm_sgd_get_info.argtypes = [vp, vp]
    L.ocffm_sgd_sync.argtypes = [vp]
    L.ocffm_sgd_destroy.argtypes = [vp]
    L.ocffm_sgd_recommend.argtypes = [vp, vp, u64, u64, u32, u32, vp, vp]
    L.ocffm_sgd_label_ranks.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ocffm_sgd_evaluate.argtypes = [vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_sgd_counter.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.ocffm_sgd_score.argtypes = [vp, vp, u64, vp, vp, vp]
    L.ocffm_sgd_recommend_among.argtypes = [vp, vp, u64, u64, vp, vp, u32, u32, vp, vp]
    L.ocffm_sgd_label_ranks_among.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ocffm_sgd_evaluate_among.argtypes = [vp, vp, vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_sgd_destroy.restype = None
    L.ocffm_model_file_info.argtypes = [C.c_char_p, i32, C.POINTER(_ModelInfo)]
    L.ocffm_model_load_text.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.ocffm_model_load_binary.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.ocffm_model_from_problem.argtypes = [vp, C.POINTER(vp)]
    L.ocffm_model_set_items.argtypes = [vp, vp]
    L.ocffm_model_set_popularity.argtypes = [vp, vp, u64]
    L.ocffm_model_recommend.argtypes = [vp, vp, u64, u64, u32, u32, vp, vp]
    L.ocffm_model_score.argtypes = [vp, vp, u64, vp, vp, vp]
    L.ocffm_model_recommend_among.argtypes = [vp, vp, u64, u64, vp, vp, u32, u32, vp, vp]
    L.ocffm_model_label_ranks.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ocffm_model_label_ranks_among.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ocffm_model_evaluate.argtypes = [vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_model_evaluate_among.argtypes = [vp, vp, vp, vp, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_model_counter.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.ocffm_model_get_info.argtypes = [vp, C.POINTER(_ModelInfo)]
    L.ocffm_model_get_ds.argtypes = [vp, vp]
    L.ocffm_model_get.argtypes = [vp, C.c_char, u32, vp, u64, C.POINTER(u64)]
    L.ocffm_model_destroy.argtypes = [vp]
    L.ocffm_model_destroy.restype = None
    fo = C.POINTER(_Fold)
    L.ocffm_model_fold_in.argtypes = [vp, vp, vp, fo, vp, vp]
    L.ocffm_model_recommend_fold.argtypes = [vp, vp, vp, fo, u64, u64, u32, u32, vp, vp]
    L.ocffm_model_label_ranks_fold.argtypes = [vp, vp, vp, fo, vp, vp, vp, vp]
    L.ocffm_model_evaluate_fold.argtypes = [vp, vp, vp, fo, vp, vp, u32, C.POINTER(_Eval)]
    L.ocffm_model_similar_items.argtypes = [vp, u64, vp, vp, vp, u32, u32, vp, vp]
    L.ocffm_model_similar_to.argtypes = [vp, vp, u64, u64, vp, vp, u32, u32, vp, vp]
    L.ocffm_model_item_similarity.argtypes = [vp, u64, vp, vp, u32, vp]
    L.ocffm_model_recommend_diverse.argtypes = [vp, vp, u64, u64, vp, vp, u32, u32, dbl, u32, vp, vp, vp, vp]
    _lib = L
    return L


def _check(st: int) -> None:
    if st != OK:
        raise OcffmError(st, lib().ocffm_last_error().decode(errors="replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lists(candidates, rows: int):
    """``candidates=(cptr, ccol)`` as the C entries take it: ``rows + 1`` uint64
    offsets into the uint32 entries (and a pointer for an empty ``ccol``)."""
    cptr = np.ascontiguousarray(candidates[0], dtype=np.uint64).reshape(-1)
    ccol = np.ascontiguousarray(candidates[1], dtype=np.uint32).reshape(-1)
    if cptr.size != rows + 1 or int(cptr.max()) > ccol.size:
        raise OcffmError(E_ARG, "candidates: cptr needs rows + 1 offsets into ccol")
    return cptr, (ccol if ccol.size else np.zeros(1, dtype=np.uint32))


def _sim_flags(metric: str, keep_self: bool = False) -> int:
    """The flags of the similarity entries (include/ocffm_similar.h)."""
    if metric not in ("cosine", "dot"):
        raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
    return (SIM_DOT if metric == "dot" else 0) | (SIM_KEEP_SELF if keep_self else 0)


def _label_ranks(fn, among, h, X, seen, candidates):
    """label_ranks of a problem or a trainer (``fn``; ``among`` with candidates)."""
    i = X.info
    ranks = np.full(max(1, i["nnz_y"]), RANK_NONE, dtype=np.uint32)
    scores = np.full(max(1, i["nnz_y"]), -np.inf, dtype=np.float64)
    ncand = np.zeros(max(1, i["m"]), dtype=np.uint32)
    sh = None if seen is None else seen.h
    if candidates is None:
        _check(fn(h, X.h, sh, _ptr(ranks), _ptr(scores), _ptr(ncand)))
    else:
        cptr, ccol = _lists(candidates, int(i["m"]))
        _check(among(h, X.h, sh, _ptr(cptr), _ptr(ccol), _ptr(ranks), _ptr(scores), _ptr(ncand)))
    return ranks[: i["nnz_y"]], scores[: i["nnz_y"]], ncand[: i["m"]]


def _evaluate(fn, among, h, X, cuts, seen, candidates) -> dict:
    c = np.ascontiguousarray(cuts, dtype=np.uint32).reshape(-1)
    e = _Eval()
    sh = None if seen is None else seen.h
    if candidates is None:
        _check(fn(h, X.h, sh, _ptr(c), c.size, C.byref(e)))
    else:
        cptr, ccol = _lists(candidates, int(X.info["m"]))
        _check(among(h, X.h, sh, _ptr(cptr), _ptr(ccol), _ptr(c), c.size, C.byref(e)))
    return e.as_dict()


def _score(fn, h, X, rows, items) -> np.ndarray:
    r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    j = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1)
    if r.size != j.size:
        raise OcffmError(E_ARG, "score: rows and items differ in length")
    out = np.full(max(1, r.size), -np.inf, dtype=np.float64)
    pad = np.zeros(1, dtype=np.uint32)
    _check(fn(h, X.h, r.size, _ptr(r if r.size else pad), _ptr(j if j.size else pad), _ptr(out)))
    return out[: r.size]


def device_count() -> int:
    c = C.c_int(0)
    _check(lib().ocffm_device_count(C.byref(c)))
    return c.value


def block_index(f1: int, f2: int, f: int) -> int:
    """index_vec (ffm.cpp:53-55)."""
    return f2 + (f - 1) * f1 - f1 * (f1 - 1) // 2


class Parameter:
    """class Parameter (ffm.h:42-49) with the reference's code defaults."""

    def __init__(self, **kw):
        p = _Param()
        lib().ocffm_param_default(C.byref(p))
        self._p = p
        for key, v in kw.items():
            setattr(self, key, v)

    def __setattr__(self, key, value):
        if key == "_p":
            object.__setattr__(self, key, value)
            return
        if key == "lambda":
            key = "lambda_"
        setattr(self._p, key, value)

    def __getattr__(self, key):
        if key == "lambda":
            key = "lambda_"
        return getattr(object.__getattribute__(self, "_p"), key)


class ImpData:
    """class ImpData (ffm.h:51-79): read + split_fields, transY."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def read(cls, path: str, has_label: bool, ds: Optional[np.ndarray] = None) -> "ImpData":
        h = C.c_void_p()
        dsa = None if ds is None else np.ascontiguousarray(ds, dtype=np.uint64)
        _check(lib().ocffm_data_read(path.encode(), int(has_label), _ptr(dsa), 0 if dsa is None else len(dsa),
                                     C.byref(h)))
        return cls(h)

    @classmethod
    def from_rows(cls, rows, ds: Optional[np.ndarray] = None) -> "ImpData":
        h = C.c_void_p()
        dsa = None if ds is None else np.ascontiguousarray(ds, dtype=np.uint64)
        arrs = [np.ascontiguousarray(rows.xptr, np.uint64), np.ascontiguousarray(rows.fid, np.uint32),
                np.ascontiguousarray(rows.idx, np.uint64), np.ascontiguousarray(rows.val, np.float64)]
        ya = None if rows.yptr is None else np.ascontiguousarray(rows.yptr, np.uint64)
        yc = None if rows.ycol is None else np.ascontiguousarray(rows.ycol, np.uint64)
        _check(lib().ocffm_data_from_rows(rows.m, *[_ptr(a) for a in arrs], _ptr(ya), _ptr(yc), _ptr(dsa),
                                          0 if dsa is None else len(dsa), C.byref(h)))
        return cls(h)

    def trans_y(self, U: "ImpData") -> None:
        _check(lib().ocffm_data_trans_y(self.h, U.h))

    @property
    def info(self) -> dict:
        i = _Info()
        _check(lib().ocffm_data_get_info(self.h, C.byref(i)))
        return dict(m=i.m, n=i.n, f=i.f, nnz_x=i.nnz_x, nnz_y=i.nnz_y)

    @property
    def Ds(self) -> np.ndarray:
        out = np.zeros(max(1, self.info["f"]), dtype=np.uint64)
        _check(lib().ocffm_data_get_ds(self.h, _ptr(out)))
        return out[: self.info["f"]]

    def labels(self):
        """(yptr, ycol) as parsed (ffm.cpp:93-101)."""
        i = self.info
        yptr = np.zeros(i["m"] + 1, dtype=np.uint64)
        ycol = np.zeros(max(1, i["nnz_y"]), dtype=np.uint64)
        _check(lib().ocffm_data_get_labels(self.h, _ptr(yptr), _ptr(ycol)))
        return yptr, ycol[: i["nnz_y"]]

    def field(self, fi: int):
        """(xptr, xidx, xval) of one field after split_fields (ffm.cpp:185-257)."""
        nnz = C.c_uint64(0)
        _check(lib().ocffm_data_get_field(self.h, fi, None, None, None, C.byref(nnz)))
        xptr = np.zeros(self.info["m"] + 1, dtype=np.int64)
        xidx = np.zeros(max(1, nnz.value), dtype=np.uint32)
        xval = np.zeros(max(1, nnz.value), dtype=np.float64)
        _check(lib().ocffm_data_get_field(self.h, fi, _ptr(xptr), _ptr(xidx), _ptr(xval), C.byref(nnz)))
        return xptr, xidx[: nnz.value], xval[: nnz.value]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.ocffm_data_free(self.h)
            self.h = None


class _SgdParam(C.Structure):
    _fields_ = [("k", C.c_uint32), ("eta", C.c_float), ("lambda_", C.c_float), ("nneg", C.c_uint32),
                ("neg_power", C.c_double), ("adagrad", C.c_int32), ("norm", C.c_int32), ("serial", C.c_int32),
                ("seed", C.c_uint64), ("device", C.c_int32)]


class _SgdInfo(C.Structure):
    _fields_ = [("n_features", C.c_uint64), ("n_fields", C.c_uint32), ("kp", C.c_uint32),
                ("positives", C.c_uint64), ("instances", C.c_uint64)]


class SgdTrainer:
    """Field-aware FM by per-instance SGD / AdaGrad with HOGWILD writes and
    on-device negative sampling (include/ocffm.h, SGD mode).  North-star
    extra with no reference counterpart: parity is against
    oracle/sgd_oracle.cpp, not the reference."""

    def __init__(self, U: "ImpData", V: "ImpData", rank: int = 0, nranks: int = 1, comm: Optional[bytes] = None,
                 allreduce=None, **kw):
        p = _SgdParam()
        lib().ocffm_sgd_param_default(C.byref(p))
        for key, val in kw.items():
            setattr(p, "lambda_" if key == "lambda" else key, val)
        self.param = p
        self._keep = (U, V)
        h = C.c_void_p()
        if allreduce is not None:  # average() through a host all-reduce (float32 arrays)
            def cb(buf, count, is_double, user):
                try:
                    allreduce(np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_float)), shape=(count,)))
                    return 0
                except Exception:  # pragma: no cover
                    return 1
            self._cb = ALLREDUCE_FN(cb)
            _check(lib().ocffm_sgd_create_dist_host(U.h, V.h, C.byref(p), rank, nranks, self._cb, None, C.byref(h)))
        elif nranks > 1 or comm is not None:
            idb = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(comm)
            _check(lib().ocffm_sgd_create_dist(U.h, V.h, C.byref(p), rank, nranks, idb, C.byref(h)))
        else:
            _check(lib().ocffm_sgd_create(U.h, V.h, C.byref(p), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.ocffm_sgd_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def info(self) -> dict:
        i = _SgdInfo()
        _check(lib().ocffm_sgd_get_info(self.h, C.byref(i)))
        return dict(n_features=i.n_features, n_fields=i.n_fields, kp=i.kp, positives=i.positives,
                    instances=i.instances)

    def epoch(self) -> float:
        loss = C.c_double(0)
        _check(lib().ocffm_sgd_epoch(self.h, C.byref(loss)))
        return loss.value

    def average(self) -> None:
        _check(lib().ocffm_sgd_average(self.h))

    def phi(self, users, items) -> np.ndarray:
        u = np.ascontiguousarray(users, dtype=np.uint32)
        v = np.ascontiguousarray(items, dtype=np.uint32)
        out = np.zeros(max(1, u.size), dtype=np.float32)
        _check(lib().ocffm_sgd_phi(self.h, u.size, _ptr(u), _ptr(v), _ptr(out)))
        return out[: u.size]

    def get(self, what: str) -> np.ndarray:
        n = C.c_uint64(0)
        _check(lib().ocffm_sgd_get(self.h, what.encode(), None, 0, C.byref(n)))
        dt = {"W": np.float32, "G": np.float32, "p": np.float32, "a": np.uint32, "o": np.uint64}[what]
        out = np.zeros(max(1, n.value), dtype=dt)
        _check(lib().ocffm_sgd_get(self.h, what.encode(), _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def set_w(self, w) -> None:
        a = np.ascontiguousarray(w, dtype=np.float32)
        _check(lib().ocffm_sgd_set_w(self.h, _ptr(a), a.size))

    def sync(self) -> None:
        _check(lib().ocffm_sgd_sync(self.h))

    def recommend(self, X: "ImpData", topn: int = 10, exclude_labels: bool = False, row0: int = 0,
                  rows: Optional[int] = None, candidates=None):
        """Top-``topn`` items of rows [row0, row0 + rows) of ``X`` (default: to its
        end) under the current W (include/ocffm.h ocffm_sgd_recommend):
        ``(items uint32 [rows, topn], scores float64 [rows, topn])``, score
        descending, equal scores by ascending item; unfilled slots hold
        ``REC_NONE`` / ``-inf``.  ``exclude_labels`` drops each row's own labels.
        With ``candidates=(cptr, ccol)`` each row is ranked among its own list
        only (ocffm_sgd_recommend_among), as in ``ImpProblem.recommend``."""
        if rows is None:
            rows = max(0, int(X.info["m"]) - row0)
        shape = (rows, max(0, min(int(topn), REC_MAX_TOPN)))
        items = np.full(shape, REC_NONE, dtype=np.uint32)
        scores = np.full(shape, -np.inf, dtype=np.float64)
        flags = REC_EXCLUDE_LABELS if exclude_labels else 0
        if candidates is None:
            _check(lib().ocffm_sgd_recommend(self.h, X.h, row0, rows, topn, flags, items.ctypes.data_as(C.c_void_p),
                                             scores.ctypes.data_as(C.c_void_p)))
            return items, scores
        cptr, ccol = _lists(candidates, rows)
        _check(lib().ocffm_sgd_recommend_among(self.h, X.h, row0, rows, _ptr(cptr), _ptr(ccol), topn, flags,
                                               items.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p)))
        return items, scores

    def score(self, X: "ImpData", rows, items) -> np.ndarray:
        """Scores of the pairs (row ``rows[e]`` of ``X``, item ``items[e]``) under
        the current W (include/ocffm.h ocffm_sgd_score): float64 [npairs], the
        values ``recommend`` returns for those pairs bit for bit; ``-inf`` for an
        item that is no candidate."""
        return _score(lib().ocffm_sgd_score, self.h, X, rows, items)

    def label_ranks(self, X: "ImpData", seen: Optional["ImpData"] = None, candidates=None):
        """Exact rank of every label of ``X`` among its row's candidates
        (include/ocffm.h ocffm_sgd_label_ranks): ``(ranks uint32 [nnz_y], scores
        float64 [nnz_y], ncand uint32 [m])`` in ``X.labels()`` order.  ``seen``
        (same row count) removes its rows' labels from the candidates; a label
        that is no candidate has ``RANK_NONE`` / ``-inf``.  With
        ``candidates=(cptr, ccol)`` (one list per row of ``X``) each label is
        ranked among its row's list and labels only
        (ocffm_sgd_label_ranks_among)."""
        L = lib()
        return _label_ranks(L.ocffm_sgd_label_ranks, L.ocffm_sgd_label_ranks_among, self.h, X, seen, candidates)

    def evaluate(self, X: "ImpData", cuts=(5, 10, 20, 40, 80), seen: Optional["ImpData"] = None,
                 candidates=None) -> dict:
        """Ranking metrics of the current W on the labelled rows ``X``
        (include/ocffm.h ocffm_sgd_evaluate; with ``candidates``
        ocffm_sgd_evaluate_among): the dict of ``ImpProblem.evaluate``."""
        L = lib()
        return _evaluate(L.ocffm_sgd_evaluate, L.ocffm_sgd_evaluate_among, self.h, X, cuts, seen, candidates)

    def counter(self, name: str) -> int:
        """Serving counter (include/ocffm.h ocffm_sgd_counter)."""
        v = C.c_int64(0)
        _check(lib().ocffm_sgd_counter(self.h, name.encode(), C.byref(v)))
        return v.value


def comm_id() -> bytes:
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().ocffm_comm_id(buf))
    return bytes(buf)


class ImpProblem:
    """class ImpProblem (ffm.h:82-151) on the GPU.

    ``nranks > 1`` shards the training rows (one process per GPU); the
    partial gradient / Hessian-vector sums are all-reduced with RCCL
    (``comm_id`` from rank 0), or through ``allreduce(np_array)`` on the host
    when given (tests: gloo)."""

    def __init__(self, U: ImpData, Uva: Optional[ImpData], V: ImpData, param: Parameter, rank: int = 0,
                 nranks: int = 1, comm: Optional[bytes] = None, allreduce=None):
        h = C.c_void_p()
        self._keep = (U, Uva, V)
        self.param = param
        uva = None if Uva is None else Uva.h
        if allreduce is not None:
            def cb(buf, count, is_double, user):
                try:
                    ctype = C.c_double if is_double else C.c_float
                    arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ctype)), shape=(count,))
                    allreduce(arr)
                    return 0
                except Exception:  # pragma: no cover
                    return 1
            self._cb = ALLREDUCE_FN(cb)
            _check(lib().ocffm_problem_create_dist_host(U.h, uva, V.h, C.byref(param._p), rank, nranks, self._cb,
                                                        None, C.byref(h)))
        elif nranks > 1 or comm is not None:
            idb = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(comm)
            _check(lib().ocffm_problem_create_dist(U.h, uva, V.h, C.byref(param._p), rank, nranks, idb,
                                                   C.byref(h)))
        else:
            _check(lib().ocffm_problem_create(U.h, uva, V.h, C.byref(param._p), C.byref(h)))
        self.h = h
        self.f = int(U.info["f"] + V.info["f"])
        self.k = int(param.k)

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.ocffm_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def n_blocks(self) -> int:
        """Field-pair blocks f(f+1)/2 (ffm.cpp:53-55); unused ones (--ns) included."""
        return self.f * (self.f + 1) // 2

    def init(self):
        _check(lib().ocffm_problem_init(self.h))

    def one_epoch(self):
        _check(lib().ocffm_problem_one_epoch(self.h))

    def solve_block(self, f1, f2):
        _check(lib().ocffm_problem_solve_block(self.h, f1, f2))

    def cache_sasb(self):
        _check(lib().ocffm_problem_cache_sasb(self.h))

    def solve(self, objective_every: int = 0, tol: float = 0.0, min_pass: int = 0) -> dict:
        """``nr_pass`` epochs (ffm.cpp:1147-1161).  ``objective_every=e`` evaluates the
        objective before the first epoch and after every e-th and prints it; ``tol``
        stops after the epoch whose relative decrease is at most ``tol`` (not
        before ``min_pass`` epochs).  Returns ``epochs``, ``converged``,
        ``objective0`` and ``objective`` (the last two None when never evaluated)."""
        if objective_every == 0 and tol <= 0.0:
            _check(lib().ocffm_problem_solve(self.h))
            return dict(epochs=int(self.param.nr_pass), converged=False, objective0=None, objective=None)
        o = _SolveOpts(int(objective_every), float(tol), int(min_pass))
        r = _SolveReport()
        _check(lib().ocffm_problem_solve_ex(self.h, C.byref(o), C.byref(r)))
        return dict(epochs=int(r.epochs), converged=bool(r.converged), objective0=r.objective0,
                    objective=r.objective)

    def objective(self) -> dict:
        """The training objective of the current state (``ocffm_problem_objective``):
        ``value = 0.5 (pos + omega (all - on_pos) + reg)`` and its terms."""
        o = _Objective()
        _check(lib().ocffm_problem_objective(self.h, C.byref(o)))
        return dict(value=o.value, pos=o.pos, on_pos=o.on_pos, all=o.all, reg=o.reg, m=int(o.m), n=int(o.n),
                    labels=int(o.labels))

    def validate(self) -> dict:
        m = _Metrics()
        _check(lib().ocffm_problem_validate(self.h, C.byref(m)))
        return dict(loss=m.loss, prec=np.array(m.prec[:]), ndcg=np.array(m.ndcg[:]), top_k=list(m.top_k))

    def test_rows(self) -> int:
        """This rank's test rows (0 without a test set)."""
        n = C.c_uint64()
        _check(lib().ocffm_problem_test_rows(self.h, C.byref(n)))
        return int(n.value)

    def validate_forced(self):
        """The reference's nDCG known-answer build (ffm.cpp:988-993): metrics
        and the per-row nDCG@5,10,20,40,80 (shape rows x 5) with the scores
        forced to z_j = n - j."""
        m = _Metrics()
        mt = self.test_rows()
        rows = np.zeros(max(1, mt) * 5, dtype=np.float64)
        _check(lib().ocffm_problem_validate_forced(self.h, C.byref(m), _ptr(rows), rows.size))
        return dict(loss=m.loss, prec=np.array(m.prec[:]), ndcg=np.array(m.ndcg[:])), rows[:mt * 5].reshape(mt, 5)

    def recommend(self, X: ImpData, topn: int = 10, exclude_labels: bool = False, row0: int = 0,
                  rows: Optional[int] = None, candidates=None):
        """Top-``topn`` items of rows [row0, row0 + rows) of ``X`` (default: to its
        end) under the current model (include/ocffm.h ocffm_problem_recommend):
        ``(items uint32 [rows, topn], scores float64 [rows, topn])``, score
        descending, equal scores by ascending item; unfilled slots hold
        ``REC_NONE`` / ``-inf``.  ``exclude_labels`` drops each row's own labels.
        With ``candidates=(cptr, ccol)`` each row is ranked among its own list
        only (ocffm_problem_recommend_among): row ``row0 + i``'s list is
        ``ccol[cptr[i]:cptr[i + 1]]``, ``cptr`` holding ``rows + 1`` offsets."""
        if rows is None:
            rows = max(0, int(X.info["m"]) - row0)
        shape = (rows, max(0, min(int(topn), REC_MAX_TOPN)))
        items = np.full(shape, REC_NONE, dtype=np.uint32)
        scores = np.full(shape, -np.inf, dtype=np.float64)
        flags = REC_EXCLUDE_LABELS if exclude_labels else 0
        if candidates is None:
            _check(lib().ocffm_problem_recommend(self.h, X.h, row0, rows, topn, flags,
                                                 items.ctypes.data_as(C.c_void_p),
                                                 scores.ctypes.data_as(C.c_void_p)))
            return items, scores
        cptr, ccol = _lists(candidates, rows)
        _check(lib().ocffm_problem_recommend_among(self.h, X.h, row0, rows, _ptr(cptr), _ptr(ccol), topn, flags,
                                                   items.ctypes.data_as(C.c_void_p),
                                                   scores.ctypes.data_as(C.c_void_p)))
        return items, scores

    def score(self, X: ImpData, rows, items) -> np.ndarray:
        """Scores of the pairs (row ``rows[e]`` of ``X``, item ``items[e]``) under
        the current model (include/ocffm.h ocffm_problem_score): float64
        [npairs], the values ``recommend`` returns for those pairs bit for bit;
        ``-inf`` for an item that is no candidate of its row."""
        return _score(lib().ocffm_problem_score, self.h, X, rows, items)

    def label_ranks(self, X: ImpData, seen: Optional[ImpData] = None, candidates=None):
        """Exact rank of every label of ``X`` among its row's candidates
        (include/ocffm.h ocffm_problem_label_ranks): ``(ranks uint32 [nnz_y],
        scores float64 [nnz_y], ncand uint32 [m])`` in ``X.labels()`` order.
        ``seen`` (same row count) removes its rows' labels from the candidates;
        a label that is no candidate has ``RANK_NONE`` / ``-inf``.  With
        ``candidates=(cptr, ccol)`` (one list per row of ``X``, as in
        ``recommend``) each label is ranked among the distinct candidates of its
        row's list united with the row's labels
        (ocffm_problem_label_ranks_among): the sampled-negatives protocol."""
        L = lib()
        return _label_ranks(L.ocffm_problem_label_ranks, L.ocffm_problem_label_ranks_among, self.h, X, seen,
                            candidates)

    def evaluate(self, X: ImpData, cuts=(5, 10, 20, 40, 80), seen: Optional[ImpData] = None,
                 candidates=None) -> dict:
        """Ranking metrics of the current model on the labelled rows ``X``
        (include/ocffm.h ocffm_problem_evaluate; with ``candidates``
        ocffm_problem_evaluate_among): a dict with ``rows``, ``rows_used``,
        ``labels``, ``labels_ranked``, ``cuts``, ``loss``, ``mrr``, ``auc`` and
        one array per cut for ``prec``, ``recall``, ``ndcg``, ``map`` and
        ``hit``."""
        L = lib()
        return _evaluate(L.ocffm_problem_evaluate, L.ocffm_problem_evaluate_among, self.h, X, cuts, seen, candidates)

    def save_binary(self, path: str) -> None:
        _check(lib().ocffm_problem_save_binary(self.h, path.encode()))

    def load_binary(self, path: str) -> None:
        _check(lib().ocffm_problem_load_binary(self.h, path.encode()))

    def get(self, what: str, b12: int = 0) -> np.ndarray:
        n = C.c_uint64(0)
        _check(lib().ocffm_problem_get(self.h, what.encode(), b12, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float64)
        _check(lib().ocffm_problem_get(self.h, what.encode(), b12, _ptr(out), n.value, C.byref(n)))
        return out

    def set(self, what: str, b12: int, arr) -> None:
        a = np.ascontiguousarray(arr, dtype=np.float64)
        _check(lib().ocffm_problem_set(self.h, what.encode(), b12, _ptr(a), a.size))

    def grad(self, f1, f2, half) -> np.ndarray:
        size = self.get("W" if half == 0 else "H", block_index(f1, f2, self.f)).size
        out = np.zeros(size, dtype=np.float64)
        _check(lib().ocffm_problem_grad(self.h, f1, f2, half, _ptr(out)))
        return out

    def hv(self, f1, f2, half, v) -> np.ndarray:
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.zeros_like(v)
        _check(lib().ocffm_problem_hv(self.h, f1, f2, half, _ptr(v), _ptr(out)))
        return out

    def save_model(self, path: str) -> None:
        _check(lib().ocffm_problem_save_model(self.h, path.encode()))

    def cg_log(self) -> np.ndarray:
        n = C.c_int(0)
        _check(lib().ocffm_problem_cg_log(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.int32)
        _check(lib().ocffm_problem_cg_log(self.h, _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def set_profiling(self, on: bool) -> None:
        _check(lib().ocffm_problem_set_profiling(self.h, int(on)))

    def set_profile_filter(self, name: Optional[str]) -> None:
        _check(lib().ocffm_problem_set_profile_filter(self.h, (name or "").encode()))

    def kernel_stats(self) -> dict:
        n = C.c_int(0)
        _check(lib().ocffm_problem_kernel_stats(self.h, None, 0, C.byref(n)))
        arr = (_KStat * max(1, n.value))()
        _check(lib().ocffm_problem_kernel_stats(self.h, arr, n.value, C.byref(n)))
        return {arr[i].name.decode(): dict(launches=arr[i].launches, total_ms=arr[i].total_ms,
                                           alg_bytes=arr[i].alg_bytes, alg_flops=arr[i].alg_flops)
                for i in range(n.value)}

    def reset_stats(self) -> None:
        _check(lib().ocffm_problem_reset_stats(self.h))

    def alg_bytes(self) -> float:
        b = C.c_double(0)
        _check(lib().ocffm_problem_alg_bytes(self.h, C.byref(b)))
        return b.value

    def counter(self, name: str) -> int:
        """Diagnostic event counter (include/ocffm.h ocffm_problem_counter)."""
        v = C.c_int64(0)
        _check(lib().ocffm_problem_counter(self.h, name.encode(), C.byref(v)))
        return v.value

    def sync(self) -> None:
        _check(lib().ocffm_problem_sync(self.h))

    def layout_digest(self) -> dict:
        """{array name: FNV-1a digest} of the device data layout (ocffm.h)."""
        n = C.c_int(0)
        _check(lib().ocffm_problem_layout_digest(self.h, None, None, 0, C.byref(n)))
        names = C.create_string_buffer(48 * max(1, n.value))
        dig = (C.c_uint64 * max(1, n.value))()
        _check(lib().ocffm_problem_layout_digest(self.h, names, dig, n.value, C.byref(n)))
        raw = names.raw
        return {raw[48 * i:48 * (i + 1)].split(b"\0", 1)[0].decode(): int(dig[i]) for i in range(n.value)}


def _model_info(fill) -> dict:
    """Two calls of an info entry (``fill(info) -> status``): the sizes, then
    Ds and the used-block flags."""
    i = _ModelInfo()
    _check(fill(i))
    ds = np.zeros(max(1, i.f), dtype=np.uint64)
    used = np.zeros(max(1, i.nblocks), dtype=np.uint8)
    i.Ds, i.used, i.ds_cap, i.used_cap = ds.ctypes.data, used.ctypes.data, ds.size, used.size
    _check(fill(i))
    return dict(f=int(i.f), fu=int(i.fu), fv=int(i.fv), k=int(i.k), kp=int(i.kp), nblocks=int(i.nblocks),
                nused=int(i.nused), self_side=bool(i.self_side), precision=int(i.precision), device=int(i.device),
                has_items=bool(i.has_items), n=int(i.n), npop=int(i.npop), Ds=ds[: i.f].copy(),
                used=used[: i.nblocks].astype(bool))


def model_file_info(path: str, binary: bool = False) -> dict:
    """Read and fully validate a saved model on the host (include/ocffm.h
    ocffm_model_file_info; no GPU): ``f``, ``fu``, ``fv``, ``k``, ``kp``, ``Ds``
    and the ``used`` flag of every block.  A malformed file raises
    ``OcffmError`` with ``E_DATA``, a missing one with ``E_IO``."""
    return _model_info(lambda i: lib().ocffm_model_file_info(path.encode(), int(binary), C.byref(i)))


class Model:
    """A stand-alone model handle (include/ocffm.h ocffm_model): W / H of a
    saved or trained model and an item catalogue, on one GPU, with the serving
    calls of ``ImpProblem`` and no training rows."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def load_text(cls, path: str, precision: int = FP64, device: int = 0) -> "Model":
        """The text model ``ImpProblem.save_model`` writes (six digits per value)."""
        h = C.c_void_p()
        _check(lib().ocffm_model_load_text(path.encode(), precision, device, C.byref(h)))
        return cls(h)

    @classmethod
    def load_binary(cls, path: str, precision: int = FP64, device: int = 0) -> "Model":
        """The snapshot ``ImpProblem.save_binary`` writes."""
        h = C.c_void_p()
        _check(lib().ocffm_model_load_binary(path.encode(), precision, device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_problem(cls, g: "ImpProblem") -> "Model":
        """The problem's current W / H with its item side and popularity as the
        catalogue, copied device to device: results on the training catalogue
        are the problem's own bits."""
        h = C.c_void_p()
        _check(lib().ocffm_model_from_problem(g.h, C.byref(h)))
        return cls(h)

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.ocffm_model_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def info(self) -> dict:
        return _model_info(lambda i: lib().ocffm_model_get_info(self.h, C.byref(i)))

    @property
    def Ds(self) -> np.ndarray:
        """The f field sizes, user fields first."""
        out = np.zeros(max(1, self.info["f"]), dtype=np.uint64)
        _check(lib().ocffm_model_get_ds(self.h, _ptr(out)))
        return out[: self.info["f"]]

    @property
    def item_Ds(self) -> np.ndarray:
        """The item fields' sizes: read an item file with these before ``set_items``."""
        return self.Ds[self.info["fu"]:]

    def set_items(self, V: ImpData) -> None:
        """Replace the catalogue by the item rows ``V`` (include/ocffm.h
        ocffm_model_set_items); clears the popularity."""
        _check(lib().ocffm_model_set_items(self.h, V.h))

    def set_popularity(self, pop) -> None:
        """Cold rows' scores over the catalogue items ``j < len(pop)`` (catalogue
        indices); an empty ``pop`` clears them."""
        a = np.ascontiguousarray(pop, dtype=np.float64).reshape(-1)
        _check(lib().ocffm_model_set_popularity(self.h, _ptr(a) if a.size else None, a.size))

    def get(self, what: str, b12: int = 0) -> np.ndarray:
        """``'W'`` / ``'H'`` of block ``b12``, ``'Q'`` (the catalogue's cross table
        of cross block ``b12``) or ``'b'``, as float64."""
        n = C.c_uint64(0)
        _check(lib().ocffm_model_get(self.h, what.encode(), b12, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float64)
        _check(lib().ocffm_model_get(self.h, what.encode(), b12, _ptr(out), n.value, C.byref(n)))
        return out

    @staticmethod
    def _fold(fold, candidates):
        """``fold=(hist, field, omega, lam, r)`` as the C entries take it."""
        if candidates is not None:
            raise ValueError("fold= cannot be combined with candidates=: the list forms do not fold")
        hist, field, omega, lam, r = fold
        return hist, _Fold(int(field), float(omega), float(lam), float(r))

    def fold_in(self, X: ImpData, hist: ImpData, field: int, omega: float, lam: float, r: float):
        """Fold the rows of ``X`` in from their histories, the labels of the
        same rows of ``hist`` (include/ocffm_fold.h ocffm_model_fold_in):
        ``(delta, nhist)``, float64 [m, fv * k] (item field major) and uint32
        [m]; a row without a history item below ``n`` has ``delta == 0``."""
        i = self.info
        m, d = int(X.info["m"]), int(i["fv"]) * int(i["k"])
        delta = np.zeros((m, d), dtype=np.float64)
        nhist = np.zeros(max(1, m), dtype=np.uint32)
        fo = _Fold(int(field), float(omega), float(lam), float(r))
        pad = np.zeros(1, dtype=np.float64)
        _check(lib().ocffm_model_fold_in(self.h, X.h, None if hist is None else hist.h, C.byref(fo),
                                         _ptr(delta if delta.size else pad), _ptr(nhist)))
        return delta, nhist[:m]

    def recommend(self, X: ImpData, topn: int = 10, exclude_labels: bool = False, row0: int = 0,
                  rows: Optional[int] = None, candidates=None, fold=None):
        """Top-``topn`` catalogue items of rows [row0, row0 + rows) of ``X``
        (include/ocffm.h ocffm_model_recommend): the shape, order and rules of
        ``ImpProblem.recommend``; with ``candidates=(cptr, ccol)`` each row is
        ranked among its own list (ocffm_model_recommend_among); with
        ``fold=(hist, field, omega, lam, r)`` the rows with a history are
        folded in first (ocffm_model_recommend_fold)."""
        if rows is None:
            rows = max(0, int(X.info["m"]) - row0)
        shape = (rows, max(0, min(int(topn), REC_MAX_TOPN)))
        items = np.full(shape, REC_NONE, dtype=np.uint32)
        scores = np.full(shape, -np.inf, dtype=np.float64)
        flags = REC_EXCLUDE_LABELS if exclude_labels else 0
        if fold is not None:
            hist, fo = self._fold(fold, candidates)
            _check(lib().ocffm_model_recommend_fold(self.h, X.h, hist.h, C.byref(fo), row0, rows, topn, flags,
                                                    items.ctypes.data_as(C.c_void_p),
                                                    scores.ctypes.data_as(C.c_void_p)))
            return items, scores
        if candidates is None:
            _check(lib().ocffm_model_recommend(self.h, X.h, row0, rows, topn, flags, items.ctypes.data_as(C.c_void_p),
                                               scores.ctypes.data_as(C.c_void_p)))
            return items, scores
        cptr, ccol = _lists(candidates, rows)
        _check(lib().ocffm_model_recommend_among(self.h, X.h, row0, rows, _ptr(cptr), _ptr(ccol), topn, flags,
                                                 items.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p)))
        return items, scores

    def score(self, X: ImpData, rows, items) -> np.ndarray:
        """Scores of the pairs (row ``rows[e]`` of ``X``, catalogue item
        ``items[e]``) (include/ocffm.h ocffm_model_score): float64 [npairs], the
        values ``recommend`` returns bit for bit; ``-inf`` for no candidate."""
        return _score(lib().ocffm_model_score, self.h, X, rows, items)

    def label_ranks(self, X: ImpData, seen: Optional[ImpData] = None, candidates=None, fold=None):
        """Exact rank of every label of ``X`` among its row's candidates
        (include/ocffm.h ocffm_model_label_ranks; with ``candidates``
        ocffm_model_label_ranks_among; with ``fold`` as in ``recommend``
        ocffm_model_label_ranks_fold): ``(ranks, scores, ncand)`` as
        ``ImpProblem.label_ranks``; labels are catalogue indices."""
        L = lib()
        if fold is not None:
            hist, fo = self._fold(fold, candidates)
            return _label_ranks(lambda h, x, sh, *out: L.ocffm_model_label_ranks_fold(h, x, hist.h, C.byref(fo), sh, *out),
                                None, self.h, X, seen, None)
        return _label_ranks(L.ocffm_model_label_ranks, L.ocffm_model_label_ranks_among, self.h, X, seen, candidates)

    def evaluate(self, X: ImpData, cuts=(5, 10, 20, 40, 80), seen: Optional[ImpData] = None,
                 candidates=None, fold=None) -> dict:
        """Ranking metrics on the labelled rows ``X`` (include/ocffm.h
        ocffm_model_evaluate; with ``candidates`` ocffm_model_evaluate_among;
        with ``fold`` as in ``recommend`` ocffm_model_evaluate_fold): the dict
        of ``ImpProblem.evaluate``."""
        L = lib()
        if fold is not None:
            hist, fo = self._fold(fold, candidates)
            return _evaluate(lambda h, x, sh, *a: L.ocffm_model_evaluate_fold(h, x, hist.h, C.byref(fo), sh, *a),
                             None, self.h, X, cuts, seen, None)
        return _evaluate(L.ocffm_model_evaluate, L.ocffm_model_evaluate_among, self.h, X, cuts, seen, candidates)

    def similar_items(self, items, topn: int = 10, metric: str = "cosine", keep_self: bool = False, exclude=None):
        """Top-``topn`` catalogue items by similarity to each catalogue item of
        ``items`` (include/ocffm_similar.h ocffm_model_similar_items): cosine of
        the items' cross-table embeddings, or their inner product with
        ``metric="dot"``.  A query item is left out of its own row unless
        ``keep_self``; ``exclude=(cptr, ccol)`` gives per-query lists of further
        items to leave out.  ``(items uint32 [nq, topn], scores float64)`` as
        ``recommend`` returns them."""
        flags = _sim_flags(metric, keep_self)
        q = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1)
        xptr, xcol = (None, None) if exclude is None else _lists(exclude, q.size)
        shape = (q.size, max(0, min(int(topn), REC_MAX_TOPN)))
        out = np.full(shape, REC_NONE, dtype=np.uint32)
        scores = np.full(shape, -np.inf, dtype=np.float64)
        pad = np.zeros(1, dtype=np.uint32)
        _check(lib().ocffm_model_similar_items(self.h, q.size, _ptr(q if q.size else pad), _ptr(xptr), _ptr(xcol),
                                               topn, flags, out.ctypes.data_as(C.c_void_p),
                                               scores.ctypes.data_as(C.c_void_p)))
        return out, scores

    def similar_to(self, V: ImpData, topn: int = 10, row0: int = 0, rows: Optional[int] = None,
                   metric: str = "cosine", exclude=None):
        """The same for rows [row0, row0 + rows) of the item rows ``V`` (read
        with ``item_Ds``), which need not be in the catalogue
        (ocffm_model_similar_to); nothing is left out but the ``exclude``
        lists."""
        flags = _sim_flags(metric)
        if rows is None:
            rows = max(0, int(V.info["m"]) - row0)
        xptr, xcol = (None, None) if exclude is None else _lists(exclude, rows)
        shape = (rows, max(0, min(int(topn), REC_MAX_TOPN)))
        out = np.full(shape, REC_NONE, dtype=np.uint32)
        scores = np.full(shape, -np.inf, dtype=np.float64)
        _check(lib().ocffm_model_similar_to(self.h, V.h, row0, rows, _ptr(xptr), _ptr(xcol), topn, flags,
                                            out.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p)))
        return out, scores

    def item_similarity(self, a, b, metric: str = "cosine") -> np.ndarray:
        """Similarity of the catalogue pairs ``(a[e], b[e])``
        (ocffm_model_item_similarity): float64 [npairs], the values
        ``similar_items`` returns bit for bit; ``-inf`` for an index outside the
        catalogue."""
        flags = _sim_flags(metric)
        pa = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
        pb = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1)
        if pa.size != pb.size:
            raise OcffmError(E_ARG, "item_similarity: a and b differ in length")
        out = np.full(max(1, pa.size), -np.inf, dtype=np.float64)
        pad = np.zeros(1, dtype=np.uint32)
        _check(lib().ocffm_model_item_similarity(self.h, pa.size, _ptr(pa if pa.size else pad),
                                                 _ptr(pb if pb.size else pad), flags, _ptr(out)))
        return out[: pa.size]

    def recommend_diverse(self, X: ImpData, topn: int = 10, theta: float = 0.3, pool: Optional[int] = None,
                          exclude_labels: bool = False, row0: int = 0, rows: Optional[int] = None, candidates=None):
        """Diversified top-``topn`` of rows [row0, row0 + rows) of ``X``
        (include/ocffm_diverse.h ocffm_model_recommend_diverse): greedy MMR on
        each row's top-``pool`` list (``recommend``'s, or with
        ``candidates=(cptr, ccol)`` the one among the row's own list), trading
        the normalised model score, weight ``1 - theta``, against the largest
        cosine similarity to an item already taken, weight ``theta``.
        ``pool=None`` means ``min(REC_MAX_TOPN, 4 * topn)``.  Returns ``(items
        uint32 [rows, topn], scores float64, mmr float64, pos uint32)``: the
        items in the order they were taken, their model scores, the value each
        was taken at and its position in the pool; ``theta=0`` is ``recommend``."""
        if rows is None:
            rows = max(0, int(X.info["m"]) - row0)
        if pool is None:
            pool = min(REC_MAX_TOPN, 4 * int(topn))
        shape = (rows, max(0, min(int(topn), REC_MAX_TOPN)))
        items = np.full(shape, REC_NONE, dtype=np.uint32)
        scores = np.full(shape, -np.inf, dtype=np.float64)
        mmr = np.full(shape, -np.inf, dtype=np.float64)
        pos = np.full(shape, REC_NONE, dtype=np.uint32)
        flags = REC_EXCLUDE_LABELS if exclude_labels else 0
        cptr, ccol = (None, None) if candidates is None else _lists(candidates, rows)
        _check(lib().ocffm_model_recommend_diverse(self.h, X.h, row0, rows, _ptr(cptr), _ptr(ccol), topn, pool,
                                                   float(theta), flags, items.ctypes.data_as(C.c_void_p),
                                                   scores.ctypes.data_as(C.c_void_p), mmr.ctypes.data_as(C.c_void_p),
                                                   pos.ctypes.data_as(C.c_void_p)))
        return items, scores, mmr, pos

    def counter(self, name: str) -> int:
        """Serving counter (include/ocffm.h ocffm_model_counter)."""
        v = C.c_int64(0)
        _check(lib().ocffm_model_counter(self.h, name.encode(), C.byref(v)))
        return v.value


def eval_from_ranks(yptr, ranks, ncand, scores=None, cuts=(5, 10, 20, 40, 80)) -> dict:
    """Ranking metrics from label ranks (include/ocffm.h ocffm_eval_from_ranks;
    host code, no GPU): ``yptr`` the m + 1 label offsets, ``ranks`` / ``scores``
    one entry per label, ``ncand`` one per row."""
    yp = np.ascontiguousarray(yptr, dtype=np.uint64)
    rk = np.ascontiguousarray(ranks, dtype=np.uint32)
    nc = np.ascontiguousarray(ncand, dtype=np.uint32)
    sc = None if scores is None else np.ascontiguousarray(scores, dtype=np.float64)
    c = np.ascontiguousarray(cuts, dtype=np.uint32).reshape(-1)
    m = yp.size - 1
    if m < 0 or nc.size < m or rk.size < int(yp[-1]) or (sc is not None and sc.size < int(yp[-1])):
        raise OcffmError(E_ARG, "eval_from_ranks: array sizes do not match yptr")
    pad = np.zeros(1, dtype=np.uint32)  # (a pointer for empty arrays)
    e = _Eval()
    _check(lib().ocffm_eval_from_ranks(m, _ptr(yp), _ptr(rk if rk.size else pad), _ptr(sc),
                                       _ptr(nc if nc.size else pad), _ptr(c if c.size else pad), c.size, C.byref(e)))
    return e.as_dict()


def srand(seed: int = 1) -> None:
    """glibc srand(): the reference's init draws from the process rand() stream."""
    C.CDLL(None).srand(C.c_uint(seed))


def problem_from_dataset(ds, precision=FP64, with_test=True, device=0, rank=0, nranks=1, comm=None,
                         allreduce=None, **overrides) -> ImpProblem:
    """Build an ImpProblem from a synth.Dataset (train.cpp:177-196 order)."""
    p = ds.params
    prm = Parameter(omega=overrides.get("omega", p["w"]), lambda_=overrides.get("lam", p["l"]),
                    r=overrides.get("r", p["r"]), nr_pass=overrides.get("t", p["t"]),
                    k=overrides.get("k", p["k"]), precision=precision, device=device,
                    self_side=int(overrides.get("self_side", True)), freq=int(overrides.get("freq", False)))
    U = ImpData.from_rows(ds.train)
    V = ImpData.from_rows(ds.item)
    V.trans_y(U)
    Ut = ImpData.from_rows(ds.test, ds=U.Ds) if (with_test and ds.test is not None) else None
    return ImpProblem(U, Ut, V, prm, rank=rank, nranks=nranks, comm=comm, allreduce=allreduce)
