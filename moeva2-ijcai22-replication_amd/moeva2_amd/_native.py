"""ctypes binding of libmoeva_mi355x.so (include/moeva_mi355x.h).

This is the only door from Python to the engine.  There is no CPU fallback: if the
library is missing or no GPU is visible, the calls raise.  Device buffers are torch
tensors (PyTorch is used for HBM allocation and streams only).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MOEVA_MI355X_LIB", os.path.join(PKG_ROOT, "lib", "libmoeva_mi355x.so"))

MV_GENE_REAL, MV_GENE_INT, MV_GENE_OHE = 0, 1, 2
OP = dict(DIFF=1, RATIO_SAFE=2, ABS_SUMDIFF=3, LCLD_INSTALL=4, LCLD_TERM=5, ABS_RATIO=6,
          MONTHDIFF=7, RATIO_MASKED=8, XOR_AUG=9,
          # tensor-path ops (C-PGD; mv_pgd_* only)
          TF_INSTALL_MIN=10, TF_HINGE_DIFF=11, TF_TERM_MIN=12, TF_RATIO_ALPHA_NEG=13,
          TF_RATIO_ALPHA_ZERO=14, TF_ABS_SUMDIFF_OFF=15,
          # user-defined expression column (attacks/moeva2/expr.py bytecode)
          EXPR=16)

EXPORTED = [
    "mv_last_error", "mv_device_count", "mv_engine_create", "mv_engine_destroy",
    "mv_set_states", "mv_evaluate", "mv_decode", "mv_constraints", "mv_survive", "mv_select_parents",
    "mv_variation", "mv_attack_run", "mv_attack_population", "mv_attack_front",
    "mv_attack_history", "mv_get_survival_carry",
    "mv_set_profiling", "mv_get_kernel_times", "mv_get_phase_times", "mv_get_row_kernel",
    "mv_get_mlp_kernel", "mv_set_attack_mode",
    "mv_set_crossover", "mv_set_mlp_precision",
    "mv_get_attack_time", "mv_mlp_create", "mv_mlp_destroy",
    "mv_mlp_predict", "mv_objcalc_create", "mv_objcalc_destroy", "mv_objcalc_run",
    "mv_objcalc_score", "mv_det_pow", "mv_debug_checks", "mv_set_state_streams",
    "mv_debug_survival_dump", "mv_get_stored_genes", "mv_gene_layout", "mv_set_gene_layout",
    "mv_pgd_create", "mv_pgd_destroy", "mv_pgd_grad", "mv_pgd_run", "mv_pgd_repair",
    "mv_train_create", "mv_train_destroy", "mv_train_steps", "mv_train_eval", "mv_train_grad",
    "mv_train_get", "mv_train_get_state", "mv_train_set_state", "mv_train_set_profiling",
    "mv_train_get_kernel_times",
    "mv_forest_create", "mv_forest_destroy", "mv_forest_predict", "mv_engine_set_forest",
    "mv_objcalc_run_forest", "mv_front", "mv_survive_wide",
    "mv_boost_create", "mv_engine_set_boost", "mv_det_exp",
    "mv_svm_create", "mv_engine_set_svm", "mv_svm_sums",
]

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_f32p = C.POINTER(C.c_float)


class ProblemDesc(C.Structure):
    _fields_ = [
        ("D", C.c_int32), ("V", C.c_int32), ("Dm", C.c_int32), ("C", C.c_int32),
        ("n_ohe", C.c_int32), ("gene_kind", _i32p), ("gene_feat", _i32p),
        ("ohe_offsets", _i32p), ("ohe_feats", _i32p), ("mut_feats", _i32p),
        ("ml_scale", _f64p), ("ml_min", _f64p), ("op_code", _i32p), ("op_arg", _i32p),
        ("op_karg", _f64p), ("n_pool", C.c_int32), ("idx_pool", _i32p), ("tol", C.c_double),
        ("norm", C.c_int32), ("scale_objectives", C.c_int32),
        ("n_expr_code", C.c_int32), ("expr_code", _i32p),
        ("n_expr_const", C.c_int32), ("expr_const", _f64p),
    ]


class ModelDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("dims", _i32p), ("W", C.POINTER(_f32p)),
                ("b", C.POINTER(_f32p))]


class AttackParams(C.Structure):
    _fields_ = [("n_gen", C.c_int32), ("pop_size", C.c_int32), ("n_offsprings", C.c_int32),
                ("seed", C.c_uint64), ("n_ref", C.c_int32), ("ref_points", _f64p),
                ("mu", C.c_double), ("history", C.c_int32)]


class ObjCalcDesc(C.Structure):
    _fields_ = [("D", C.c_int32), ("n_ohe", C.c_int32), ("ohe_offsets", _i32p),
                ("ohe_feats", _i32p), ("mm_scale", _f64p), ("mm_min", _f64p),
                ("ml_scale", _f64p), ("ml_min", _f64p), ("norm", C.c_int32)]


class ForestDesc(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_classes", C.c_int32), ("n_trees", C.c_int32),
                ("n_leaves", C.c_int32), ("n_nodes", C.c_int64), ("feature", _i32p),
                ("threshold", _f64p), ("left", _i32p), ("right", _i32p), ("tree_root", _i32p),
                ("leaf_value", _f64p)]


class BoostDesc(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_classes", C.c_int32), ("n_outputs", C.c_int32),
                ("n_trees", C.c_int32), ("n_leaves", C.c_int32), ("n_nodes", C.c_int64),
                ("feature", _i32p), ("threshold", _f64p), ("left", _i32p), ("right", _i32p),
                ("tree_root", _i32p), ("leaf_value", _f64p), ("base", _f64p)]


class SvmDesc(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("n_classes", C.c_int32), ("n_out", C.c_int32),
                ("n_vec", C.c_int32), ("kernel", C.c_int32), ("degree", C.c_int32),
                ("link", C.c_int32), ("gamma", C.c_double), ("coef0", C.c_double),
                ("probA", C.c_double), ("probB", C.c_double), ("vectors", _f64p),
                ("coef", _f64p), ("intercept", _f64p)]


class PgdDesc(C.Structure):
    _fields_ = [("D", C.c_int32), ("ml_scale", _f64p), ("ml_min", _f64p),
                ("mutable_mask", _i32p), ("C", C.c_int32), ("op_code", _i32p), ("op_arg", _i32p),
                ("op_karg", _f64p), ("n_pool", C.c_int32), ("idx_pool", _i32p),
                ("n_ohe", C.c_int32), ("ohe_offsets", _i32p), ("ohe_feats", _i32p),
                ("repair_install", C.c_int32 * 4), ("tol", C.c_double),
                ("n_expr_code", C.c_int32), ("expr_code", _i32p),
                ("n_expr_const", C.c_int32), ("expr_const", _f64p)]


class PgdParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("norm", C.c_int32), ("eps", C.c_double),
                ("eps_step", C.c_double), ("loss_flags", C.c_int32), ("adaptive", C.c_int32),
                ("repair", C.c_int32)]


PGD_LOSS_FLIP, PGD_LOSS_CONSTRAINTS = 1, 2


class TrainOpt(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("epsilon", C.c_double)]


class NativeError(RuntimeError):
    pass


_LIB = None


def lib():
    """Load the engine library (raises if it was not built: no silent fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} not found: build it with `make -C moeva2-ijcai22-replication_amd/csrc`"
                " (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        L.mv_last_error.restype = C.c_char_p
        vp = C.c_void_p
        sig = {
            "mv_device_count": [_i32p],
            "mv_engine_create": [C.c_int32, C.POINTER(ProblemDesc), C.POINTER(ModelDesc),
                                 C.POINTER(vp)],
            "mv_set_states": [vp, C.c_int32, _f64p, _f64p, _f64p, _i32p, vp],
            "mv_evaluate": [vp, C.c_int32, vp, vp, vp, vp],
            "mv_decode": [vp, C.c_int32, vp, vp, vp],
            "mv_constraints": [vp, C.c_int32, vp, vp, vp],
            "mv_survive": [C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_double,
                           C.c_uint64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
            "mv_survive_wide": [C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_double,
                                C.c_uint64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                C.c_int32, vp],
            "mv_select_parents": [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, vp, vp],
            "mv_variation": [vp, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, vp, vp, vp, vp],
            "mv_attack_run": [vp, C.POINTER(AttackParams), vp],
            "mv_attack_population": [vp, vp, vp, vp],
            "mv_attack_front": [vp, vp, vp, vp, vp, vp],
            "mv_front": [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp],
            "mv_attack_history": [vp, vp, vp],
            "mv_get_survival_carry": [vp, _i32p, _i32p],
            "mv_set_profiling": [vp, C.c_int32],
            "mv_get_kernel_times": [vp, _f64p, _f64p, _f64p, _i32p],
            "mv_get_phase_times": [vp, _f64p, _i32p],
            "mv_get_row_kernel": [vp, _i32p],
            "mv_get_mlp_kernel": [vp, _i32p],
            "mv_set_attack_mode": [vp, C.c_int32],
            "mv_set_crossover": [vp, C.c_int32, C.c_double, C.c_double],
            "mv_set_mlp_precision": [vp, C.c_int32],
            "mv_get_attack_time": [vp, _f64p, _i32p],
            "mv_mlp_create": [C.c_int32, C.POINTER(ModelDesc), C.POINTER(vp)],
            "mv_mlp_predict": [vp, C.c_int32, vp, vp, vp],
            "mv_objcalc_create": [C.c_int32, C.POINTER(ObjCalcDesc), C.POINTER(vp)],
            "mv_objcalc_run": [vp, vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, vp],
            "mv_objcalc_score": [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32,
                                 C.c_int32, vp, vp, vp],
            "mv_det_pow": [C.c_int64, _f64p, _f64p, _f64p],
            "mv_debug_checks": [_i32p, _i32p],
            "mv_set_state_streams": [vp, C.c_int32, C.c_int64],
            "mv_debug_survival_dump": [_f64p],
            "mv_get_stored_genes": [vp, _i32p, _i32p],
            "mv_gene_layout": [vp, C.c_int32, _f64p, _f64p, _f64p, _i32p, _i32p],
            "mv_set_gene_layout": [vp, _i32p, C.c_int32],
            "mv_pgd_create": [C.c_int32, C.POINTER(PgdDesc), C.POINTER(ModelDesc), C.POINTER(vp)],
            "mv_pgd_grad": [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp],
            "mv_pgd_run": [vp, C.POINTER(PgdParams), C.c_int32, vp, vp, vp, vp],
            "mv_pgd_repair": [vp, C.c_int32, vp, vp],
            "mv_train_create": [C.c_int32, C.POINTER(ModelDesc), C.POINTER(TrainOpt),
                                C.POINTER(vp)],
            "mv_train_steps": [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp],
            "mv_train_eval": [vp, C.c_int32, vp, vp, vp, vp],
            "mv_train_grad": [vp, C.c_int32, vp, vp, vp, vp, vp, vp],
            "mv_train_get": [vp, C.POINTER(_f32p), C.POINTER(_f32p)],
            "mv_train_get_state": [vp, _f32p, _f32p, C.POINTER(C.c_int64)],
            "mv_train_set_state": [vp, _f32p, _f32p, C.c_int64],
            "mv_train_set_profiling": [vp, C.c_int32],
            "mv_train_get_kernel_times": [vp, _f64p, _f64p, C.POINTER(C.c_int64)],
            "mv_forest_create": [C.c_int32, C.POINTER(ForestDesc), C.POINTER(vp)],
            "mv_forest_predict": [vp, C.c_int32, vp, vp, vp],
            "mv_engine_set_forest": [vp, C.POINTER(ForestDesc)],
            "mv_objcalc_run_forest": [vp, vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp,
                                      vp, vp],
            "mv_boost_create": [C.c_int32, C.POINTER(BoostDesc), C.POINTER(vp)],
            "mv_engine_set_boost": [vp, C.POINTER(BoostDesc)],
            "mv_det_exp": [C.c_int64, _f64p, _f64p],
            "mv_svm_create": [C.c_int32, C.POINTER(SvmDesc), C.POINTER(vp)],
            "mv_engine_set_svm": [vp, C.POINTER(SvmDesc)],
            "mv_svm_sums": [C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, _f64p],
        }
        for name, args in sig.items():
            try:
                fn = getattr(L, name)
            except AttributeError:  # an older build (A/B runs): the call itself will fail
                continue
            fn.argtypes = args
            fn.restype = C.c_int
        L.mv_engine_destroy.argtypes = [vp]
        L.mv_engine_destroy.restype = None
        L.mv_mlp_destroy.argtypes = [vp]
        L.mv_mlp_destroy.restype = None
        L.mv_objcalc_destroy.argtypes = [vp]
        L.mv_objcalc_destroy.restype = None
        L.mv_pgd_destroy.argtypes = [vp]
        L.mv_pgd_destroy.restype = None
        L.mv_train_destroy.argtypes = [vp]
        L.mv_train_destroy.restype = None
        if hasattr(L, "mv_forest_destroy"):
            L.mv_forest_destroy.argtypes = [vp]
            L.mv_forest_destroy.restype = None
        _LIB = L
    return _LIB


MV_ERR_ARG = 1


def check(rc: int):
    if rc != 0:
        raise NativeError(f"libmoeva_mi355x error {rc}: {lib().mv_last_error().decode()}")


def debug_checks():
    """(compiled, record) of the device index checks (csrc/check.h; a -DMV_CHECKS build):
    record = [code, workgroup, thread, value, bound, failures], cleared by the call.
    Synchronises the device."""
    rec = (C.c_int32 * 8)()
    on = C.c_int32(0)
    check(lib().mv_debug_checks(rec, C.byref(on)))
    return bool(on.value), list(rec)[:6]


def debug_survival_dump() -> np.ndarray:
    """Checks builds: the first duplicate-survivor state's inputs (mv_debug_survival_dump)."""
    out = np.zeros(24 + 3 * 1024)
    check(lib().mv_debug_survival_dump(out.ctypes.data_as(_f64p)))
    return out


def det_pow(x, y) -> np.ndarray:
    """The engine's variation pow (csrc/detmath.h), host build: elementwise, broadcast."""
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    out = np.empty(x.shape, np.float64)
    f64 = lambda a: a.ctypes.data_as(_f64p)  # noqa: E731
    check(lib().mv_det_pow(x.size, f64(x), f64(y), f64(out)))
    return out


def det_exp(x) -> np.ndarray:
    """The engine's exp for boosted ensembles (csrc/detmath.h det_exp2(x, 0.0)), host build:
    elementwise."""
    x = np.ascontiguousarray(np.asarray(x, np.float64))
    out = np.empty(x.shape, np.float64)
    f64 = lambda a: a.ctypes.data_as(_f64p)  # noqa: E731
    check(lib().mv_det_exp(x.size, f64(x), f64(out)))
    return out


def svm_sums(x, vectors, rbf) -> np.ndarray:
    """The feature sums of k_svm (csrc/svm.h svm_term, one fma per feature in ascending order),
    host build: x [n][D], vectors [n_vec][D] -> [n][n_vec] of x.v, or of |x - v|^2 when rbf."""
    x = np.ascontiguousarray(np.atleast_2d(x), np.float64)
    v = np.ascontiguousarray(np.atleast_2d(vectors), np.float64)
    if x.shape[1] != v.shape[1]:
        raise ValueError(f"x has {x.shape[1]} features, the vectors {v.shape[1]}")
    out = np.empty((x.shape[0], v.shape[0]), np.float64)
    f64 = lambda a: a.ctypes.data_as(_f64p)  # noqa: E731
    check(lib().mv_svm_sums(x.shape[0], x.shape[1], v.shape[0], int(bool(rbf)), f64(x), f64(v),
                            f64(out)))
    return out


def _ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("expected a contiguous device tensor")
    return C.c_void_p(t.data_ptr())


def _stream(stream=None):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _arr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def norm_code(norm) -> int:
    """2 for the L2 distance, 0 for L-inf; anything else is rejected like the reference
    DefaultProblem._obj_distance (default_problem.py:80-88 raises NotImplementedError)."""
    if isinstance(norm, str):
        norm = norm.strip().lower()
        if norm in ("2", "l2"):
            return 2
        if norm in ("inf", "np.inf", "linf"):
            return 0
    elif norm == 2:
        return 2
    elif norm == np.inf:
        return 0
    raise ValueError(f"norm {norm!r} is not supported (2 or np.inf)")


@dataclass
class DeviceProgram:
    """Host description of one problem: genetic layout + constraint program."""

    D: int
    gene_kind: np.ndarray  # (V,) int32
    gene_feat: np.ndarray  # (V,)
    ohe_offsets: np.ndarray  # (n_ohe+1,)
    ohe_feats: np.ndarray
    mut_feats: np.ndarray  # (Dm,) ascending
    op_code: np.ndarray  # (C,)
    op_arg: np.ndarray  # (C,4)
    op_karg: np.ndarray  # (C,2)
    idx_pool: np.ndarray
    tol: float = 1e-3
    expr_code: Optional[np.ndarray] = None  # int32 bytecode of the MV_OP_EXPR columns
    expr_const: Optional[np.ndarray] = None  # fp64 constants of that bytecode

    @property
    def V(self):
        return int(self.gene_kind.shape[0])

    @property
    def C(self):
        return int(self.op_code.shape[0])


class Engine:
    """One engine per (device, problem, classifier)."""

    def __init__(self, prog: DeviceProgram, weights: Optional[Sequence[np.ndarray]],
                 biases: Optional[Sequence[np.ndarray]], ml_scale=None, ml_min=None, norm=2,
                 scale_objectives=True, device: int = 0):
        L = lib()
        self.prog = prog
        self.device = device
        keep = []

        def P(a, dt, ct):
            a = _arr(a, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))

        pd = ProblemDesc()
        pd.D = prog.D
        pd.V = prog.V
        pd.Dm = int(prog.mut_feats.shape[0])
        pd.C = prog.C
        pd.n_ohe = int(prog.ohe_offsets.shape[0]) - 1
        pd.gene_kind = P(prog.gene_kind, np.int32, C.c_int32)
        pd.gene_feat = P(prog.gene_feat, np.int32, C.c_int32)
        pd.ohe_offsets = P(prog.ohe_offsets, np.int32, C.c_int32)
        pd.ohe_feats = P(prog.ohe_feats if prog.ohe_feats.size else np.zeros(1), np.int32,
                         C.c_int32)
        pd.mut_feats = P(prog.mut_feats, np.int32, C.c_int32)
        pd.ml_scale = P(ml_scale, np.float64, C.c_double) if ml_scale is not None else None
        pd.ml_min = P(ml_min, np.float64, C.c_double) if ml_min is not None else None
        pd.op_code = P(prog.op_code, np.int32, C.c_int32)
        pd.op_arg = P(prog.op_arg, np.int32, C.c_int32)
        pd.op_karg = P(prog.op_karg, np.float64, C.c_double)
        pd.n_pool = int(prog.idx_pool.shape[0])
        pd.idx_pool = P(prog.idx_pool if prog.idx_pool.size else np.zeros(1), np.int32, C.c_int32)
        xc = np.zeros(0, np.int32) if prog.expr_code is None else prog.expr_code
        xk = np.zeros(0) if prog.expr_const is None else prog.expr_const
        pd.n_expr_code = int(xc.shape[0])
        pd.expr_code = P(xc if xc.size else np.zeros(1), np.int32, C.c_int32)
        pd.n_expr_const = int(xk.shape[0])
        pd.expr_const = P(xk if xk.size else np.zeros(1), np.float64, C.c_double)
        pd.tol = prog.tol
        pd.norm = norm_code(norm)
        pd.scale_objectives = int(bool(scale_objectives))
        md = ModelDesc()
        if weights is not None:
            n = len(weights)
            dims = [int(weights[0].shape[0])] + [int(w.shape[1]) for w in weights]
            md.n_layers = n
            md.dims = P(np.array(dims), np.int32, C.c_int32)
            Ws = (_f32p * n)(*[P(w, np.float32, C.c_float) for w in weights])
            bs = (_f32p * n)(*[P(b, np.float32, C.c_float) for b in biases])
            keep += [Ws, bs]
            md.W = Ws
            md.b = bs
        self._h = C.c_void_p()
        check(L.mv_engine_create(device, C.byref(pd), C.byref(md) if weights is not None else None,
                                 C.byref(self._h)))
        self.B = 0
        self.dims = dims if weights is not None else []
        self.n_out = dims[-1] if weights is not None else 0
        self.forest = None

    def set_forest(self, tables):
        """Make a tree ensemble (models.forest.ForestTables) the engine's classifier
        (mv_engine_set_forest): only on an engine built without weights, before set_states.
        Tables outside the engine's limits raise ValueError."""
        d, keep = _forest_desc(tables)
        _check_forest(lib().mv_engine_set_forest(self._h, C.byref(d)))
        self.forest = tables
        self.n_out = tables.n_classes

    def set_boost(self, tables):
        """Make a boosted ensemble (models.boost.BoostTables) the engine's classifier
        (mv_engine_set_boost): set_forest's preconditions and errors."""
        d, keep = _boost_desc(tables)
        _check_forest(lib().mv_engine_set_boost(self._h, C.byref(d)))
        self.forest = tables
        self.n_out = tables.n_classes

    def set_svm(self, tables):
        """Make a kernel machine or logistic regression (models.svm.SvmTables) the engine's
        classifier (mv_engine_set_svm): set_forest's preconditions and errors."""
        d, keep = _svm_desc(tables)
        _check_forest(lib().mv_engine_set_svm(self._h, C.byref(d)))
        self.forest = tables
        self.n_out = tables.n_classes

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _LIB is not None:
            _LIB.mv_engine_destroy(h)
            self._h = None

    # -- per-state constants
    def set_states(self, x_init, xl, xu, minimize_class, stream=None, owner=None):
        """Bind B initial states (mv_set_states).  ``owner`` tags the binding so a caller
        that evaluates repeatedly on the same states (DefaultProblem) binds only once."""
        self.bound_by = None
        x_init = _arr(x_init, np.float64)
        xl = _arr(xl, np.float64)
        xu = _arr(xu, np.float64)
        mc = _arr(np.broadcast_to(np.asarray(minimize_class), (x_init.shape[0],)), np.int32)
        check(lib().mv_set_states(self._h, x_init.shape[0],
                                  x_init.ctypes.data_as(_f64p), xl.ctypes.data_as(_f64p),
                                  xu.ctypes.data_as(_f64p), mc.ctypes.data_as(_i32p),
                                  _stream(stream)))
        self.B = x_init.shape[0]
        self.bound_by = owner  # only once the engine holds these states

    def evaluate(self, genes, F, G=None, stream=None):
        """genes (B, n, V) fp64 device tensor -> F (B, n, 3) [, G (B, n, C)]."""
        check(lib().mv_evaluate(self._h, genes.shape[1], _ptr(genes), _ptr(F), _ptr(G),
                                _stream(stream)))

    def decode(self, genes, x, stream=None):
        """genes (B, n, V) -> ML-space rows x (B, n, D) (FeatureEncoder.genetic_to_ml)."""
        check(lib().mv_decode(self._h, genes.shape[1], _ptr(genes), _ptr(x), _stream(stream)))

    def constraints(self, x, G, stream=None):
        """x (n, D) fp64 device tensor -> G (n, C) (the numpy-path Constraints.evaluate)."""
        check(lib().mv_constraints(self._h, x.shape[0], _ptr(x), _ptr(G), _stream(stream)))

    def variation(self, P, O, seed, gen, pop, parents, off, stream=None):
        check(lib().mv_variation(self._h, P, O, seed, gen, _ptr(pop), _ptr(parents), _ptr(off),
                                 _stream(stream)))

    def attack_run(self, n_gen, pop_size, n_offsprings, seed, ref_points, mu=0.05, history=0,
                   stream=None):
        ref = _arr(ref_points, np.float64)
        self._ref_keep = ref
        prm = AttackParams(n_gen, pop_size, n_offsprings, seed, ref.shape[0],
                           ref.ctypes.data_as(_f64p), mu, history)
        check(lib().mv_attack_run(self._h, C.byref(prm), _stream(stream)))

    def attack_population(self, genes=None, F=None, stream=None):
        check(lib().mv_attack_population(self._h, _ptr(genes), _ptr(F), _stream(stream)))

    def attack_front(self, front=None, offsets=None, X=None, Fx=None, stream=None):
        """The final population's non-dominated members (mv_attack_front): front (B, P)
        uint8, offsets (B + 1,) int32 and the members' genes X (B * P, V) / objectives
        Fx (B * P, 3) packed by state in population order (first offsets[B] rows)."""
        check(lib().mv_attack_front(self._h, _ptr(front), _ptr(offsets), _ptr(X), _ptr(Fx),
                                    _stream(stream)))

    def attack_history(self, hist, stream=None, host=False):
        """History rows (B, P + (n_gen - 1) O, 3 | 3 + C) into a device tensor, or with
        host=True a contiguous host tensor -- page-locked (pinned / hipHostRegister'ed) for a
        direct DMA; mv_attack_history copies with hipMemcpyDefault."""
        if host:
            if hist.is_cuda or not hist.is_contiguous():
                raise ValueError("attack_history(host=True): a contiguous host tensor")
            p = C.c_void_p(hist.data_ptr())
        else:
            p = _ptr(hist)
        check(lib().mv_attack_history(self._h, p, _stream(stream)))

    def survival_carry(self):
        """Per state, the survival calls of the last attack that skipped dominance work among
        the survivors and that reused their association (mv_get_survival_carry): two int32
        arrays (B,)."""
        dom = np.zeros(self.B, np.int32)
        assoc = np.zeros(self.B, np.int32)
        check(lib().mv_get_survival_carry(self._h, dom.ctypes.data_as(_i32p),
                                          assoc.ctypes.data_as(_i32p)))
        return dom, assoc

    def set_profiling(self, on: bool):
        check(lib().mv_set_profiling(self._h, int(on)))

    def set_crossover(self, kind: str = "two_point", eta: float = 30.0, prob: float = 0.9):
        """"two_point" (the reference's operator) or "sbx" (SimulatedBinaryCrossover)."""
        check(lib().mv_set_crossover(self._h, {"two_point": 0, "sbx": 1}[kind], float(eta),
                                     float(prob)))

    def set_state_streams(self, enabled: bool, first_state: int = 0):
        """Per-state random streams (engine option, off = the reference's shared draws):
        state b draws from Philox stream first_state + b, its GLOBAL index."""
        check(lib().mv_set_state_streams(self._h, 1 if enabled else 0, int(first_state)))
        self.state_streams = (bool(enabled), int(first_state))

    def stored_genes(self) -> np.ndarray:
        """The attack's gene layout for the bound states (mv_get_stored_genes): bool [V],
        False for a gene no attack on these states can change (integer, xl == xu == its
        initial value in every state), which the attack does not store or sum."""
        st = np.zeros(self.prog.V, np.int32)
        n = C.c_int32(0)
        check(lib().mv_get_stored_genes(self._h, st.ctypes.data_as(_i32p), C.byref(n)))
        return st.astype(bool)

    def gene_layout(self, x_init, xl, xu) -> np.ndarray:
        """The layout mv_set_states would derive for these states (mv_gene_layout; host
        computation): bool [V], True = stored."""
        x_init, xl, xu = (_arr(a, np.float64) for a in (x_init, xl, xu))
        st = np.zeros(self.prog.V, np.int32)
        n = C.c_int32(0)
        check(lib().mv_gene_layout(self._h, x_init.shape[0], x_init.ctypes.data_as(_f64p),
                                   xl.ctypes.data_as(_f64p), xu.ctypes.data_as(_f64p),
                                   st.ctypes.data_as(_i32p), C.byref(n)))
        return st.astype(bool)

    def set_gene_layout(self, stored=None):
        """Fix the layout of the next set_states calls (mv_set_gene_layout): bool [V] as
        gene_layout returned it for the whole job, or None to derive it per bound batch."""
        if stored is None:
            check(lib().mv_set_gene_layout(self._h, None, 0))
            return
        st = np.ascontiguousarray(np.asarray(stored, bool), np.int32)
        check(lib().mv_set_gene_layout(self._h, st.ctypes.data_as(_i32p), int(st.shape[0])))

    def set_mlp_precision(self, dtype: str = "fp32"):
        """Classifier precision of the fitness path: "fp32" (parity default) or "bf16" (perf
        mode: bf16 weights/activations on bf16 MFMA, fp32 accumulation)."""
        if dtype not in ("fp32", "bf16"):
            raise ValueError(f"mlp dtype {dtype!r}: 'fp32' or 'bf16'")
        if dtype == "bf16" and self.forest is not None:
            raise ValueError("mlp_dtype='bf16' is the Dense MLP's perf mode; a forest runs in "
                             "fp64 only")
        check(lib().mv_set_mlp_precision(self._h, 1 if dtype == "bf16" else 0))
        self.mlp_dtype = dtype

    def set_attack_mode(self, mode: str):
        """"chain"/"auto": the per-phase kernel chain (k_gen, k_cons, k_mlp2, k_survive per
        generation), the engine's only schedule.  The whole-attack kernel ("whole") was
        retired (measured slower)."""
        if mode not in ("auto", "chain"):
            raise ValueError(f"attack mode {mode!r}: 'auto' or 'chain' (the whole-attack "
                             "kernel was retired)")
        check(lib().mv_set_attack_mode(self._h, {"auto": 0, "chain": 1}[mode]))

    def kernel_times(self):
        """Summed device ms of k_vary / k_mlp / k_survive over the last profiled attack."""
        tv, tm, ts = C.c_double(), C.c_double(), C.c_double()
        n = C.c_int32()
        check(lib().mv_get_kernel_times(self._h, C.byref(tv), C.byref(tm), C.byref(ts),
                                        C.byref(n)))
        ph = (C.c_double * 4)()
        check(lib().mv_get_phase_times(self._h, ph, C.byref(n)))
        rk = C.c_int32()
        check(lib().mv_get_row_kernel(self._h, C.byref(rk)))
        mk = C.c_int32()
        check(lib().mv_get_mlp_kernel(self._h, C.byref(mk)))
        return {"vary_ms": tv.value, "mlp_ms": tm.value, "survive_ms": ts.value,
                "gen_ms": ph[0], "cons_ms": ph[1], "generations": n.value,
                "row_kernel": ("k_gen+k_cons", "k_narrow", "k_genc")[rk.value],
                "mlp_kernel": {-1: None, 0: "k_mlp", 1: "k_mlp2(genes)", 2: "k_mlp2",
                               4: "k_mlpw", 5: "k_mlpw32", 6: "k_mlpr(genes)", 7: "k_mlpr",
                               8: "k_forest", 9: "k_boost", 10: "k_boost(lds)",
                               11: "k_svm"}[mk.value]}

    def mlp_kernel(self) -> int:
        """mv_get_mlp_kernel's kind (csrc/routes.h MlpKind; 8 = k_forest, 9 / 10 = k_boost,
        11 = k_svm)."""
        mk = C.c_int32()
        check(lib().mv_get_mlp_kernel(self._h, C.byref(mk)))
        return int(mk.value)


def survive(F, ref_points, n_survive, mu, seed, gen, ideal, worst, extreme, has_extreme,
            survivors, rank=None, order=None, n_ranked=None, niche=None, dist=None, nadir=None,
            stream=None, wide=None):
    """Batched R-NSGA-III survival on device tensors (see mv_survive).  wide (0, 1, 2) picks
    the kernel instance for N <= 512 as an attack does from its number of states
    (mv_survive_wide; None: mv_survive, which is wide 0); every instance computes the same
    bits."""
    B, N, _ = F.shape
    if wide is None:
        check(lib().mv_survive(B, N, n_survive, _ptr(F), ref_points.shape[0], _ptr(ref_points),
                               mu, seed, gen, _ptr(ideal), _ptr(worst), _ptr(extreme),
                               _ptr(has_extreme), _ptr(survivors), _ptr(rank), _ptr(order),
                               _ptr(n_ranked), _ptr(niche), _ptr(dist), _ptr(nadir),
                               _stream(stream)))
        return
    check(lib().mv_survive_wide(B, N, n_survive, _ptr(F), ref_points.shape[0], _ptr(ref_points),
                                mu, seed, gen, _ptr(ideal), _ptr(worst), _ptr(extreme),
                                _ptr(has_extreme), _ptr(survivors), _ptr(rank), _ptr(order),
                                _ptr(n_ranked), _ptr(niche), _ptr(dist), _ptr(nadir), wide,
                                _stream(stream)))


def front(F, front, offsets, genes=None, X=None, Fx=None, stream=None):
    """Non-dominated members of caller-supplied populations (mv_front): F (B, P, 3) and
    optionally genes (B, P, V) device tensors -> front (B, P) uint8, offsets (B + 1,) int32,
    X (B * P, V) / Fx (B * P, 3) packed as Engine.attack_front packs them."""
    B, P, _ = F.shape
    V = 0 if genes is None else int(genes.shape[2])
    check(lib().mv_front(B, P, V, _ptr(F), _ptr(genes), _ptr(front), _ptr(offsets), _ptr(X),
                         _ptr(Fx), _stream(stream)))


def select_parents(B, P, O, seed, gen, parents, stream=None):
    check(lib().mv_select_parents(B, P, O, seed, gen, _ptr(parents), _stream(stream)))


def device_count() -> int:
    n = C.c_int32()
    check(lib().mv_device_count(C.byref(n)))
    return n.value


def _model_desc(weights, biases, keep):
    n = len(weights)
    dims = np.array([int(weights[0].shape[0])] + [int(w.shape[1]) for w in weights], np.int32)
    Wc = [np.ascontiguousarray(w, np.float32) for w in weights]
    bc = [np.ascontiguousarray(b, np.float32) for b in biases]
    Ws = (_f32p * n)(*[w.ctypes.data_as(_f32p) for w in Wc])
    bs = (_f32p * n)(*[b.ctypes.data_as(_f32p) for b in bc])
    keep += [dims, Wc, bc, Ws, bs]
    md = ModelDesc()
    md.n_layers = n
    md.dims = dims.ctypes.data_as(_i32p)
    md.W = Ws
    md.b = bs
    return md


class Mlp:
    """Device classifier for Classifier.predict_proba (mv_mlp_*)."""

    def __init__(self, weights, biases, device=0):
        keep = []
        md = _model_desc(weights, biases, keep)
        self._h = C.c_void_p()
        check(lib().mv_mlp_create(device, C.byref(md), C.byref(self._h)))
        self.n_out = int(weights[-1].shape[1])
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _LIB is not None:
            _LIB.mv_mlp_destroy(h)
            self._h = None

    def predict(self, x, proba, stream=None):
        check(lib().mv_mlp_predict(self._h, x.shape[0], _ptr(x), _ptr(proba), _stream(stream)))


def _forest_desc(t):
    """ForestDesc of a models.forest.ForestTables (and the arrays it points into)."""
    keep = [np.ascontiguousarray(t.feature, np.int32), np.ascontiguousarray(t.threshold, np.float64),
            np.ascontiguousarray(t.left, np.int32), np.ascontiguousarray(t.right, np.int32),
            np.ascontiguousarray(t.tree_root, np.int32),
            np.ascontiguousarray(t.leaf_value, np.float64)]
    d = ForestDesc()
    d.n_features = int(t.n_features)
    d.n_classes = int(keep[5].shape[1]) if keep[5].ndim == 2 else 0
    d.n_trees = int(keep[4].shape[0])
    d.n_leaves = int(keep[5].shape[0])
    d.n_nodes = int(keep[0].shape[0])
    d.feature = keep[0].ctypes.data_as(_i32p)
    d.threshold = keep[1].ctypes.data_as(_f64p)
    d.left = keep[2].ctypes.data_as(_i32p)
    d.right = keep[3].ctypes.data_as(_i32p)
    d.tree_root = keep[4].ctypes.data_as(_i32p)
    d.leaf_value = keep[5].ctypes.data_as(_f64p)
    return d, keep


def _check_forest(rc: int):
    """MV_ERR_ARG from a forest call is a table outside the limits: ValueError."""
    if rc == MV_ERR_ARG:
        raise ValueError(lib().mv_last_error().decode())
    check(rc)


class Forest:
    """Device tree ensemble for Classifier.predict_proba (mv_forest_*)."""

    def __init__(self, tables, device=0):
        d, keep = _forest_desc(tables)
        self._h = C.c_void_p()
        _check_forest(lib().mv_forest_create(device, C.byref(d), C.byref(self._h)))
        self.n_out = int(tables.n_classes)
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _LIB is not None:
            _LIB.mv_forest_destroy(h)
            self._h = None

    def predict(self, x, proba, stream=None):
        check(lib().mv_forest_predict(self._h, x.shape[0], _ptr(x), _ptr(proba), _stream(stream)))


def _boost_desc(t):
    """BoostDesc of a models.boost.BoostTables (and the arrays it points into)."""
    keep = [np.ascontiguousarray(t.feature, np.int32), np.ascontiguousarray(t.threshold, np.float64),
            np.ascontiguousarray(t.left, np.int32), np.ascontiguousarray(t.right, np.int32),
            np.ascontiguousarray(t.tree_root, np.int32),
            np.ascontiguousarray(t.leaf_value, np.float64).reshape(-1),
            np.ascontiguousarray(t.base, np.float64).reshape(-1)]
    d = BoostDesc()
    d.n_features = int(t.n_features)
    d.n_classes = int(t.n_classes)
    d.n_outputs = int(keep[6].shape[0])
    d.n_trees = int(keep[4].shape[0])
    d.n_leaves = int(keep[5].shape[0])
    d.n_nodes = int(keep[0].shape[0])
    d.feature = keep[0].ctypes.data_as(_i32p)
    d.threshold = keep[1].ctypes.data_as(_f64p)
    d.left = keep[2].ctypes.data_as(_i32p)
    d.right = keep[3].ctypes.data_as(_i32p)
    d.tree_root = keep[4].ctypes.data_as(_i32p)
    d.leaf_value = keep[5].ctypes.data_as(_f64p)
    d.base = keep[6].ctypes.data_as(_f64p)
    return d, keep


class Boost(Forest):
    """Device boosted ensemble behind the forest handle (mv_boost_create): predict, the
    destructor and ObjCalc.run are Forest's."""

    def __init__(self, tables, device=0):
        d, keep = _boost_desc(tables)
        self._h = C.c_void_p()
        _check_forest(lib().mv_boost_create(device, C.byref(d), C.byref(self._h)))
        self.n_out = int(tables.n_classes)
        self.device = device


def _svm_desc(t):
    """SvmDesc of a models.svm.SvmTables (and the arrays it points into)."""
    from .models.svm import KERNELS, LINKS

    vec = np.ascontiguousarray(t.vectors, np.float64)
    if vec.ndim != 2:
        raise ValueError("vectors must be [n_vec][n_features]")
    icpt = np.ascontiguousarray(t.intercept, np.float64).reshape(-1)
    coef = None if t.coef is None else np.ascontiguousarray(t.coef, np.float64)
    if coef is not None and coef.shape != (icpt.shape[0], vec.shape[0]):
        raise ValueError(f"coef {coef.shape}: expected ({icpt.shape[0]}, {vec.shape[0]})")
    if t.kernel not in KERNELS or t.link not in LINKS:
        raise ValueError(f"kernel {t.kernel!r} / link {t.link!r} outside the engine's")
    if float(t.degree) != int(t.degree):
        raise ValueError(f"degree={t.degree!r} is not an integer")
    if vec.shape[0] and vec.shape[1] != int(t.n_features):
        raise ValueError("vectors' width is not n_features")
    d = SvmDesc()
    d.n_features = int(t.n_features)
    d.n_classes = int(t.n_classes)
    d.n_out = int(icpt.shape[0])
    d.n_vec = int(vec.shape[0])
    d.kernel = KERNELS.index(t.kernel)
    d.degree = int(t.degree)
    d.link = LINKS.index(t.link)
    d.gamma, d.coef0 = float(t.gamma), float(t.coef0)
    d.probA, d.probB = float(t.probA), float(t.probB)
    d.vectors = vec.ctypes.data_as(_f64p)
    d.coef = None if coef is None else coef.ctypes.data_as(_f64p)
    d.intercept = icpt.ctypes.data_as(_f64p)
    return d, [vec, coef, icpt]


class Svm(Forest):
    """Device kernel machine / logistic regression behind the forest handle (mv_svm_create):
    predict, the destructor and ObjCalc.run are Forest's."""

    def __init__(self, tables, device=0):
        d, keep = _svm_desc(tables)
        self._h = C.c_void_p()
        _check_forest(lib().mv_svm_create(device, C.byref(d), C.byref(self._h)))
        self.n_out = int(tables.n_classes)
        self.device = device


class ObjCalc:
    """Device ObjectiveCalculator._calculate_objective (mv_objcalc_*): one per (type mask,
    min_max_scaler, ml_scaler, norm)."""

    def __init__(self, D, ohe_groups, mm_scale, mm_min, ml_scale=None, ml_min=None, norm=2,
                 device=0):
        keep = []

        def P(a, dt, ct):
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))

        offs = np.zeros(len(ohe_groups) + 1, np.int32)
        for g, m in enumerate(ohe_groups):
            offs[g + 1] = offs[g] + len(m)
        feats = (np.concatenate([np.asarray(m, np.int32) for m in ohe_groups])
                 if ohe_groups else np.zeros(1, np.int32))
        d = ObjCalcDesc()
        d.D = int(D)
        d.n_ohe = len(ohe_groups)
        d.ohe_offsets = P(offs, np.int32, C.c_int32)
        d.ohe_feats = P(feats, np.int32, C.c_int32)
        d.mm_scale = P(mm_scale, np.float64, C.c_double)
        d.mm_min = P(mm_min, np.float64, C.c_double)
        if ml_scale is not None:
            d.ml_scale = P(ml_scale, np.float64, C.c_double)
            d.ml_min = P(ml_min, np.float64, C.c_double)
        d.norm = norm_code(norm)
        self._h = C.c_void_p()
        check(lib().mv_objcalc_create(device, C.byref(d), C.byref(self._h)))
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _LIB is not None:
            _LIB.mv_objcalc_destroy(h)
            self._h = None

    def run(self, engine: "Engine", mlp: "Mlp", x_init, x, minimize_class, obj, range_bad,
            stream=None):
        """x_init (B, D), x (B, n, D) device tensors -> obj (B, n, 3), range_bad (B, n)."""
        B, n = int(x.shape[0]), int(x.shape[1])
        run = lib().mv_objcalc_run_forest if isinstance(mlp, Forest) else lib().mv_objcalc_run
        check(run(self._h, engine._h, mlp._h, B, n, _ptr(x_init), _ptr(x), int(minimize_class),
                  _ptr(obj), _ptr(range_bad), _stream(stream)))

    def score(self, x_init, x, G, proba, minimize_class, obj, range_bad, stream=None):
        """Scoring with a caller-supplied constraint matrix G (B*n, C) (None: C = 0) and
        class probabilities proba (B*n, n_out), all device tensors (mv_objcalc_score)."""
        B, n = int(x.shape[0]), int(x.shape[1])
        C_ = 0 if G is None else int(G.shape[-1])
        check(lib().mv_objcalc_score(self._h, B, n, _ptr(x_init), _ptr(x), _ptr(G), C_,
                                     _ptr(proba), int(proba.shape[-1]), int(minimize_class),
                                     _ptr(obj), _ptr(range_bad), _stream(stream)))


class Pgd:
    """Device C-PGD (mv_pgd_*): one per (device, tensor program, scaler, classifier).

    ``program`` is a ConstraintProgram built by ``Constraints.tensor_program()``;
    ``ohe_groups`` / ``repair_install`` describe ``fix_features_types`` (empty / None: the
    identity)."""

    def __init__(self, program, weights, biases, ml_scale, ml_min, mutable_mask,
                 ohe_groups=(), repair_install=None, tol=1e-3, device=0):
        keep = []

        def P(a, dt, ct):
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))

        code, arg, karg, pool = program.arrays()
        d = PgdDesc()
        d.D = int(np.asarray(ml_scale).shape[0])
        d.ml_scale = P(ml_scale, np.float64, C.c_double)
        d.ml_min = P(ml_min, np.float64, C.c_double)
        d.mutable_mask = P(np.asarray(mutable_mask).astype(bool), np.int32, C.c_int32)
        d.C = int(code.shape[0])
        d.op_code = P(code if code.size else np.zeros(1), np.int32, C.c_int32)
        d.op_arg = P(arg if arg.size else np.zeros(4), np.int32, C.c_int32)
        d.op_karg = P(karg if karg.size else np.zeros(2), np.float64, C.c_double)
        d.n_pool = int(pool.shape[0])
        d.idx_pool = P(pool if pool.size else np.zeros(1), np.int32, C.c_int32)
        offs = np.zeros(len(ohe_groups) + 1, np.int32)
        for g, m in enumerate(ohe_groups):
            offs[g + 1] = offs[g] + len(m)
        feats = (np.concatenate([np.asarray(m, np.int32) for m in ohe_groups])
                 if len(ohe_groups) else np.zeros(1, np.int32))
        d.n_ohe = len(ohe_groups)
        d.ohe_offsets = P(offs, np.int32, C.c_int32)
        d.ohe_feats = P(feats, np.int32, C.c_int32)
        ri = list(repair_install) if repair_install is not None else [-1, -1, -1, -1]
        d.repair_install = (C.c_int32 * 4)(*[int(v) for v in ri])
        d.tol = float(tol)
        xc, xk = program.expr_arrays()  # both empty without an EXPR column
        d.n_expr_code = int(xc.shape[0])
        d.expr_code = P(xc if xc.size else np.zeros(1), np.int32, C.c_int32)
        d.n_expr_const = int(xk.shape[0])
        d.expr_const = P(xk if xk.size else np.zeros(1), np.float64, C.c_double)
        md = _model_desc(weights, biases, keep)
        self._h = C.c_void_p()
        check(lib().mv_pgd_create(device, C.byref(d), C.byref(md), C.byref(self._h)))
        self.device = device
        self.D = d.D
        self.C = d.C

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _LIB is not None:
            _LIB.mv_pgd_destroy(h)
            self._h = None

    def grad(self, x, y, loss_flags, grad=None, losses=None, iter_i=0, stream=None):
        """x (n, D) fp32, y (n,) int32 device tensors -> grad (n, D), losses (n, 2 + C)."""
        check(lib().mv_pgd_grad(self._h, int(x.shape[0]), _ptr(x), _ptr(y), int(loss_flags),
                                int(iter_i), _ptr(grad), _ptr(losses), _stream(stream)))

    def run(self, x_init, x_adv, max_iter, norm, eps, eps_step, loss_flags, adaptive=False,
            repair=False, y=None, stream=None):
        prm = PgdParams(int(max_iter), norm_code(norm), float(eps), float(eps_step),
                        int(loss_flags), int(bool(adaptive)), int(bool(repair)))
        check(lib().mv_pgd_run(self._h, C.byref(prm), int(x_init.shape[0]), _ptr(x_init),
                               _ptr(y), _ptr(x_adv), _stream(stream)))

    def repair(self, x, stream=None):
        """fix_features_types on feature-space rows x (n, D) fp32, in place."""
        check(lib().mv_pgd_repair(self._h, int(x.shape[0]), _ptr(x), _stream(stream)))


class Trainer:
    """Device training of a Dense(relu)...Dense(softmax) model (mv_train_*): Adam on the mean
    cross-entropy, one per (device, model).  Flat arrays hold, per layer, W row-major
    (in, out) then b."""

    def __init__(self, weights, biases, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, device=0):
        keep = []
        md = _model_desc(weights, biases, keep)
        opt = TrainOpt(float(lr), float(beta1), float(beta2), float(epsilon))
        self._h = C.c_void_p()
        check(lib().mv_train_create(device, C.byref(md), C.byref(opt), C.byref(self._h)))
        self.device = device
        self.dims = [int(weights[0].shape[0])] + [int(w.shape[1]) for w in weights]
        self.n_params = sum(k * n + n for k, n in zip(self.dims[:-1], self.dims[1:]))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _LIB is not None:
            _LIB.mv_train_destroy(h)
            self._h = None

    def steps(self, x, y, batch, n_steps, first_row=0, perm=None, step_losses=None, stream=None):
        """x (n, D) fp32, y (n,) int32, perm (n,) int32 or None: n_steps Adam steps."""
        check(lib().mv_train_steps(self._h, int(x.shape[0]), _ptr(x), _ptr(y), _ptr(perm),
                                   int(first_row), int(batch), int(n_steps), _ptr(step_losses),
                                   _stream(stream)))

    def eval(self, x, y, out, stream=None):
        """out (2,) fp32 device tensor <- (mean cross-entropy, argmax-correct rows)."""
        check(lib().mv_train_eval(self._h, int(x.shape[0]), _ptr(x), _ptr(y), _ptr(out),
                                  _stream(stream)))

    def grad(self, x, y, grad, loss=None, perm=None, stream=None):
        """The mean cross-entropy's gradient over all rows: grad (n_params,), loss (1,)."""
        check(lib().mv_train_grad(self._h, int(x.shape[0]), _ptr(x), _ptr(y), _ptr(perm),
                                  _ptr(grad), _ptr(loss), _stream(stream)))

    def get(self):
        """(weights, biases) as host fp32 arrays; synchronises the device."""
        import torch

        torch.cuda.synchronize(self.device)
        W = [np.empty((k, n), np.float32) for k, n in zip(self.dims[:-1], self.dims[1:])]
        b = [np.empty(n, np.float32) for n in self.dims[1:]]
        n = len(W)
        check(lib().mv_train_get(self._h, (_f32p * n)(*[w.ctypes.data_as(_f32p) for w in W]),
                                 (_f32p * n)(*[v.ctypes.data_as(_f32p) for v in b])))
        return W, b

    def get_state(self):
        """(m, v, step): Adam's flat moments and the step count; synchronises the device."""
        import torch

        torch.cuda.synchronize(self.device)
        m, v = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.float32)
        step = C.c_int64(0)
        check(lib().mv_train_get_state(self._h, m.ctypes.data_as(_f32p), v.ctypes.data_as(_f32p),
                                       C.byref(step)))
        return m, v, int(step.value)

    def set_state(self, m, v, step):
        import torch

        torch.cuda.synchronize(self.device)
        m, v = _arr(m, np.float32), _arr(v, np.float32)
        if m.shape != (self.n_params,) or v.shape != (self.n_params,):
            raise ValueError("set_state: m and v are flat (n_params,) arrays")
        check(lib().mv_train_set_state(self._h, m.ctypes.data_as(_f32p), v.ctypes.data_as(_f32p),
                                       int(step)))

    def set_profiling(self, on: bool):
        check(lib().mv_train_set_profiling(self._h, int(bool(on))))

    def kernel_times(self):
        """Device ms in k_train_grad / k_train_adam over the profiled steps."""
        g, u, n = C.c_double(), C.c_double(), C.c_int64()
        check(lib().mv_train_get_kernel_times(self._h, C.byref(g), C.byref(u), C.byref(n)))
        return {"grad_ms": g.value, "adam_ms": u.value, "steps": int(n.value)}


def flatten_params(weights, biases) -> np.ndarray:
    """The flat parameter layout of mv_train_*: per layer W row-major (in, out), then b."""
    return np.concatenate([np.concatenate([np.asarray(w, np.float32).ravel(),
                                           np.asarray(b, np.float32).ravel()])
                           for w, b in zip(weights, biases)])


_MLPS = {}


def predict_proba(mlp, x):
    """Host convenience: numpy rows (already ML-scaled) -> probabilities, on the GPU."""
    import torch

    m = _MLPS.get(id(mlp))
    if m is None:
        m = _MLPS[id(mlp)] = (Mlp(mlp.weights, mlp.biases), mlp)
    m = m[0]
    xd = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x), np.float64)).cuda(m.device)
    out = torch.empty((xd.shape[0], m.n_out), dtype=torch.float64, device=xd.device)
    m.predict(xd, out)
    return out.cpu().numpy()


_FORESTS = {}


def forest_predict_proba(tables, x):
    """Host convenience: numpy rows (already ML-scaled) -> a forest's probabilities, on the
    GPU."""
    import torch

    m = _FORESTS.get(id(tables))
    if m is None:
        m = _FORESTS[id(tables)] = (Forest(tables), tables)
    m = m[0]
    xd = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x), np.float64)).cuda(m.device)
    out = torch.empty((xd.shape[0], m.n_out), dtype=torch.float64, device=xd.device)
    m.predict(xd, out)
    return out.cpu().numpy()


def boost_predict_proba(tables, x):
    """forest_predict_proba for a models.boost.BoostTables."""
    import torch

    m = _FORESTS.get(id(tables))
    if m is None:
        m = _FORESTS[id(tables)] = (Boost(tables), tables)
    m = m[0]
    xd = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x), np.float64)).cuda(m.device)
    out = torch.empty((xd.shape[0], m.n_out), dtype=torch.float64, device=xd.device)
    m.predict(xd, out)
    return out.cpu().numpy()


def svm_predict_proba(tables, x):
    """forest_predict_proba for a models.svm.SvmTables."""
    import torch

    m = _FORESTS.get(id(tables))
    if m is None:
        m = _FORESTS[id(tables)] = (Svm(tables), tables)
    m = m[0]
    xd = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x), np.float64)).cuda(m.device)
    out = torch.empty((xd.shape[0], m.n_out), dtype=torch.float64, device=xd.device)
    m.predict(xd, out)
    return out.cpu().numpy()
