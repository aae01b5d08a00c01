"""Synthetic problems at the row kernels' shape edges (helper module, not a test file).

The shipped problems give the row kernels four shapes.  ``build(case, tmp_path)`` makes a
problem of any shape from a ``Case``: the host side goes through the product's own classes --
a features CSV and a constraints CSV written to ``tmp_path``, a ``TabularConstraints`` subclass
whose ``device_program()`` is built with ``ConstraintProgram.add`` / ``add_sumdiff``, and
``get_encoder_from_constraints(...).device_layout()`` -- so nothing of ``TabularConstraints`` had
to be bypassed.  The oracle side is ``mo.make_layout`` / ``mo.make_problem`` with a plain numpy
fp64 statement of the same ops (``eval_ops``: the formulas of include/moeva_mi355x.h, then the
``tol`` clamp, as ``mo.botnet_constraints`` / ``mo.lcld_constraints`` do).

Feature order: the mutable features (first one-hot group, the plain features with the middle
groups spread among them, last group), with one immutable feature after every third mutable
one and the remaining immutable features at the end.  Every constraint op owns one immutable
"partner" feature whose value in a state makes the op satisfied with slack in states 1 and 2
and, for a random 60 % of the ops, violated in state 0: the columns bite on the perturbed rows
of ``test_gpu_row_routes`` without saturating (tests/test_synth_problem_cpu.py checks the
shares on the oracle alone).  The mutable operands go round the plain features from both ends
(first, last, second, ...), so the first and the last gene of a shape are always read by an op.

Bounds lie on a 1/8 grid (any float parser reads them exactly) with every lower bound >= 1,
so a ratio's denominator is >= 1 inside the bounds; every seventh plain feature has a
``dynamic`` lower bound (the input's value); the compact cases fix genes by ``dynamic`` on both
sides.  The classifier is a fixed-seed Dense D-32-16-2 net with non-zero biases (``Case.net``
gives another one: MLP_CASES, the shapes of the classifier's fallback kernel), the ML scaler
has scale != 1 and min != 0.

``Case.expr`` ("all" / "mixed") restates the selected columns as MV_OP_EXPR expressions in
``device_program()`` (``op_expression``: the way moeva2_amd/examples/generic.py writes the
shipped programs); ``eval_ops`` stays the statement of the values, and ``Synth.codes`` holds 16
for the restated columns, so the engine-order oracle sums f3 in the engine's lane order.
"""
import dataclasses
import os
from typing import Callable, Optional, Tuple

import numpy as np

from oracle import moeva_oracle as mo
from moeva2_amd._native import OP
from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram, TabularConstraints

B = 3  # states per case
N_PERTURBED = 37
TINY = 5e-324  # a non-zero denominator whose quotient overflows: RATIO_MASKED's "inf" branch


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n_plain: int                       # plain (real / int) mutable features = plain genes
    ohe: Tuple[int, ...] = ()          # one-hot group sizes: the first group opens the mutable
    #                                    features, the last closes them, the others lie between
    C: int = 0                         # constraint columns (the ABS_SUMDIFF ones included)
    full: bool = False                 # add the LCLD financial ops
    install: bool = False              # ... and one LCLD_INSTALL column (calls pow)
    xor: bool = True                   # plain programs: XOR_AUG columns (never slim)
    sumdiff: Tuple[int, ...] = ()      # first-side pool size of each ABS_SUMDIFF column
    fixed: Optional[Callable] = None   # compact cases: gene -> states in which it is fixed
    all_int: bool = False
    sbx: bool = False                  # run a second time with crossover="sbx"
    planovf: bool = False              # also run under the plan-overflow build
    expr: str = ""                     # "all": every column restated as an MV_OP_EXPR expression;
    #                                    "mixed": the columns c % 3 == 2 (ABS_SUMDIFF stays dedicated)
    seed: int = 0                      # the attack's seed where the common one does not do (0)
    net: Tuple[int, ...] = ()          # classifier (hidden..., classes); () = the D-32-16-2 net
    mlp_v1: str = ""                   # the classifier kernel under MV_MLP_V1, where a test runs it
    # what the engine is expected to run (csrc/routes.h; pinned by tests/test_routes_cpu.py)
    row: str = "k_gen+k_cons"
    row_sbx: str = ""                  # with crossover="sbx" (default: the same)
    mlp: str = "k_mlpr"
    note: str = ""

    @property
    def V(self):
        return self.n_plain + len(self.ohe)

    @property
    def Dm(self):
        return self.n_plain + sum(self.ohe)

    @property
    def ident(self):
        return not self.ohe


def _every(k, states=(0, 1, 2)):
    return lambda g: states if k(g) else ()


_GENC = dict(xor=False, row="k_genc")
CASES = [
    # --- narrow family (two-point crossover)
    Case("n8p", 8, C=5, sbx=True, row="k_narrow", row_sbx="k_gen+k_cons", mlp="k_mlpr(genes)",
         note="k_narrow<8,false>; SBX: k_gen<true,1,true> at a handful of genes"),
    Case("n8f", 6, ohe=(2, 5), C=8, full=True, row="k_narrow", note="k_narrow<8,true>"),
    Case("n9", 9, C=6, row="k_narrow", mlp="k_mlp2(genes)", note="k_narrow<16,false>, odd Dm"),
    Case("n16f", 15, ohe=(4,), C=10, full=True, row="k_narrow", note="k_narrow<16,true>"),
    Case("n17f", 16, ohe=(6,), C=10, full=True, row="k_narrow", note="k_narrow<32,true>"),
    Case("n32", 30, ohe=(17, 17), C=64, row="k_narrow",
         note="k_narrow<32,false>: V 32, Dm4 64, C 64, every guard at its limit"),
    Case("n32d", 30, ohe=(17, 18), C=64, note="Dm 65 (Dm4 80): k_gen<false,2> + k_cons"),
    Case("n32c", 30, ohe=(17, 17), C=65, note="C 65: k_gen<false,1> + k_cons"),
    Case("n8s", 8, C=6, sumdiff=(2,), mlp="k_mlpr(genes)",
         note="a sum-difference op in a small problem: k_gen<true,1> + k_cons"),
    Case("n2", 2, C=2, row="k_narrow", mlp="k_mlpr(genes)",
         note="k_narrow<8,false>; one real and one integer gene: both crossover subsets of size 1"),
    # --- wave-per-row family
    Case("g33", 33, C=20, sbx=True, mlp="k_mlp2(genes)",
         note="k_gen<true,1> + k_cons<false,true,1>"),
    Case("g64", 64, C=40, mlp="k_mlpr(genes)", note="NT 1, every lane used"),
    Case("g65", 65, C=40, sbx=True, mlp="k_mlp2(genes)",
         note="NT 2 with one gene in the second slab"),
    Case("g128", 128, C=70, mlp="k_mlpr(genes)", note="NT 2, the last k_gen size"),
    Case("o40f", 37, ohe=(3, 2, 9), C=24, full=True, install=True,
         note="k_gen<false,1> + k_cons<true,false,1>; the LCLD_INSTALL case"),
    Case("o100p", 94, ohe=(2, 3, 9, 14, 14, 14), C=70, sbx=True,
         note="Dm 150 (Dm4 160): NT 4, IDENT false"),
    Case("o300f", 294, ohe=(2, 3, 5, 7, 9, 10), C=100, full=True, note="Dm 330: NT 8, FULL"),
    Case("o520p", 512, ohe=(11,) * 8, C=150, note="Dm 600: NT 16"),
    # --- k_genc family (IDENT, DIFF / RATIO_SAFE programs: slim)
    Case("c129", 129, C=70, sbx=True, planovf=True, mlp="k_mlp2(genes)", note="NT 4, first size",
         **_GENC),
    Case("c256", 256, C=100, mlp="k_mlpr(genes)", note="NT 4 full", **_GENC),
    Case("c257", 257, C=100, mlp="k_mlp2(genes)", note="NT 5", **_GENC),
    Case("c384", 384, C=130, sbx=True, planovf=True, mlp="k_mlpr(genes)", note="NT 6 full",
         **_GENC),
    Case("c385", 385, C=130, mlp="k_mlp2(genes)", note="NT 7", **_GENC),
    Case("c512", 512, C=150, mlp="k_mlpr(genes)", note="NT 8 full", **_GENC),
    Case("c513", 513, C=150, mlp="k_mlp2(genes)", note="NT 16", **_GENC),
    Case("c1024", 1024, C=300, mlp="k_mlpr(genes)", note="NT 16 at VARY_MAX_V", **_GENC),
    Case("c300x", 300, C=400, mlp="k_mlpr(genes)",
         note="400 lane ops > 64 OPS_REG = 384: SLIM false in the product route", **_GENC),
    Case("c300d", 300, C=100, sumdiff=(1, 64, 65), mlp="k_mlpr(genes)",
         note="slim; 97 lane ops and 3 ABS_SUMDIFF over pools of 1, 64 and 65", **_GENC),
    # --- compact layouts (IDENT V 200)
    Case("k_slab", 200, C=80, fixed=_every(lambda g: g < 64), mlp="k_mlpr(genes)",
         note="genes 0..63 fixed: a whole 64-gene slab", **_GENC),
    Case("k_last", 200, C=80, fixed=_every(lambda g: g == 199), mlp="k_mlp2(genes)",
         note="only the last gene fixed (199 stored: odd)", **_GENC),
    Case("k_odd", 200, C=80, fixed=_every(lambda g: g % 7 in (1, 4) and g < 199),
         mlp="k_mlp2(genes)", note="57 scattered fixed genes, 143 stored: off k_mlpr", **_GENC),
    Case("k_few", 200, C=80, fixed=_every(lambda g: g not in (1, 76, 199)), xor=False,
         mlp="k_mlp2(genes)", note="3 stored genes: k_gen<true,1> + k_cons with compact set"),
    Case("k_mixed", 200, C=80,
         fixed=lambda g: (0, 1, 2) if g % 5 == 0 else (0, 1) if g == 7 else (),
         mlp="k_mlpr(genes)",
         note="gene 7 fixed in states 0 and 1, free in state 2: stored", **_GENC),
]
# --- MV_OP_EXPR columns: every program with one runs k_gen +
# k_consx<IDENT, NT>, whatever its shape; the cases sit where vary_nt changes.  The twin of a
# case is the same Case with expr="" (the dedicated ops; the kernels of the families above).
_COMPACT_OF = {}
for _c in [c for c in CASES if c.name in ("k_last", "k_odd", "k_few", "k_mixed")]:
    _COMPACT_OF["x" + _c.name] = _c.name
CASES += [
    Case("x64", 64, C=40, expr="all", mlp="k_mlpr(genes)", note="k_consx<true,1>, every lane used"),
    Case("x65", 65, C=40, expr="mixed", sbx=True, mlp="k_mlp2(genes)",
         note="k_consx<true,2>, one gene in the second slab"),
    Case("x128", 128, C=70, expr="all", mlp="k_mlpr(genes)", note="k_consx<true,2> full"),
    Case("x129", 129, C=70, expr="mixed", xor=False, mlp="k_mlp2(genes)",
         note="k_consx<true,4>: the size that goes to k_genc without EXPR"),
    Case("x256", 256, C=100, expr="all", mlp="k_mlpr(genes)", note="k_consx<true,4> full"),
    Case("x257", 257, C=100, expr="mixed", mlp="k_mlp2(genes)", note="k_consx<true,8>"),
    Case("x512", 512, C=150, expr="mixed", mlp="k_mlpr(genes)", note="k_consx<true,8> full"),
    Case("x513", 513, C=150, expr="all", mlp="k_mlp2(genes)", note="k_consx<true,16>"),
    Case("x1024", 1024, C=300, expr="mixed", mlp="k_mlpr(genes)",
         note="k_consx<true,16> at VARY_MAX_V"),
    Case("x300c", 300, C=400, expr="mixed", xor=False, sumdiff=(1, 64, 65), mlp="k_mlpr(genes)",
         note="k_consx<true,8>; 397 lane ops > 64 OPS_REG = 384: the tail loop with EXPR lanes"),
    Case("xo32d", 30, ohe=(17, 18), C=64, full=True, expr="mixed", note="k_consx<false,2>"),
    Case("xo100", 94, ohe=(2, 3, 9, 14, 14, 14), C=70, expr="mixed", sbx=True,
         note="k_consx<false,4>"),
    Case("xo300f", 294, ohe=(2, 3, 5, 7, 9, 10), C=100, full=True, install=True, expr="all",
         note="k_consx<false,8>, the POW column"),
    Case("xo520", 512, ohe=(11,) * 8, C=150, expr="mixed",
         note="k_consx<false,16> (256 VGPRs and AGPRs)"),
    Case("xn8f", 6, ohe=(2, 5), C=8, full=True, expr="all",
         note="k_consx<false,1> on a shape that is k_narrow without EXPR"),
] + [dataclasses.replace(CASES[[c.name for c in CASES].index(k)], name=x, expr="mixed",
                         row="k_gen+k_cons",
                         # xk_few: under the common attack seed, state 0's 3 stored genes of 200
                         # are hit by no mutation that survives (found on the oracle alone)
                         seed=8 if x == "xk_few" else 0,
                         note="k_consx with a compact gene set: " + k)
     for x, k in _COMPACT_OF.items()]
# --- the classifier's 32-row-tile fallback k_mlp<MAXCT, BF> (tests/test_gpu_mlp_fallback.py,
# tests/test_gpu_bf16_routes.py): plain mutable features only, few columns, a net of their own.
# Kept apart from CASES: the row-route tests run every entry of CASES under the D-32-16-2 net.
# The shapes sit at the LDS edges that tests/native/routes_check.cpp computes ("lds" and "mlp
# synth" lines of tests/test_routes_cpu.py): a 512-512-2 net's mlpw32_lds passes 160 KiB from
# Dm4 624 on (a 512-256-2 net's from 640 on: the final layer's weights share the budget), so
# the pair is 608 | 609 features; mv_engine_create's mlp_lds_bytes check accepts 512-512-2 up
# to Dm4 720 (736 is refused), 512-272-3 up to 736 and 144-240-3 up to 1008 (1024 is refused:
# the widest case is 1008 features, not VARY_MAX_V).  m639t has an odd gene count because an even one with hidden
# widths <= 64 stays on k_mlpr under MV_MLP_V1 (mlpr_ok comes first in mlp_route).
_MLP = dict(C=12, xor=False, row="k_genc")
MLP_CASES = [
    Case("m608w", 608, net=(512, 512, 2), mlp="k_mlpw32",
         note="k_mlpw32<4>: the near side of the mlpw32_lds guard", **_MLP),
    Case("m609w", 609, net=(512, 512, 2), sbx=True, mlp="k_mlp",
         note="k_mlp<8,false>; Dm4 624 (bf16: 19.5 steps of 32, the half step in layer 0)", **_MLP),
    Case("m736w", 736, net=(512, 272, 3), mlp="k_mlp",
         note="k_mlp<8,false> at the largest Dm4 this net is accepted at; 32 and 17 column "
              "tiles, 3 classes", **_MLP),
    Case("m1008w", 1008, net=(144, 240, 3), mlp="k_mlp",
         note="k_mlp<4,false> at the largest Dm4 this net is accepted at; 9 and 15 column tiles "
              "(bf16: K 144, the half step)", **_MLP),
    Case("m640n", 640, net=(48, 80, 2), mlp="k_mlp2(genes)", mlp_v1="k_mlp",
         note="MV_MLP_V1: k_mlp<2,false>, U = 8 with K 48 (the kk < K tail); 3 and 5 column tiles",
         **_MLP),
    Case("m639t", 639, net=(32, 16, 8), mlp="k_mlp2(genes)", mlp_v1="k_mlp",
         note="MV_MLP_V1: k_mlp<1,false>, waves 2 and 3 without a column tile, 8 classes", **_MLP),
]
MLP_BY_NAME = {c.name: c for c in MLP_CASES}
CASES_BY_NAME = {c.name: c for c in CASES}
NARROW = [c.name for c in CASES if c.row == "k_narrow"]
COMPACT = [c.name for c in CASES if c.fixed is not None]
EXPR = [c.name for c in CASES if c.expr]
# fixed genes of the compact cases (the x cases share their twin's pattern)
N_FIXED = {"k_slab": 64, "k_last": 1, "k_odd": 57, "k_few": 197, "k_mixed": 40}
N_FIXED.update({x: N_FIXED[k] for x, k in _COMPACT_OF.items()})


def twin(case: Case) -> Case:
    """The same problem with every column a dedicated op (same name: same seeds, same files)."""
    return dataclasses.replace(case, expr="")


def case_seed(name):
    return 1000 + [c.name for c in CASES + MLP_CASES].index(name)


def min_classes(case: Case):
    """The class each state minimises: 1 everywhere for two classes (and for every case of
    CASES), (2, 0, 1) from three classes on, so a wrong state's class shows."""
    return (2, 0, 1) if case.net and case.net[-1] >= 3 else (1, 1, 1)


# ------------------------------------------------------------------ the ops in numpy fp64
def _month(f):
    return np.floor(f / 100) * 12 + (f % 100)


def eval_ops(ops, x, tol=1e-3):
    """(n, D) -> (n, C): each column from its formula in include/moeva_mi355x.h, then values
    <= tol -> 0 (Constraints.evaluate).  Sums of ABS_SUMDIFF pools are over integer-valued
    features here, so their order does not matter."""
    x = np.asarray(x, np.float64)
    cols = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for name, a, k in ops:
            if name == "DIFF":
                g = x[:, a[0]] - x[:, a[1]]
            elif name == "RATIO_SAFE":
                num, den = x[:, a[0]], x[:, a[1]]
                g = np.divide(num, den, out=np.zeros_like(num), where=den != 0) - k[0]
            elif name == "XOR_AUG":
                g = np.abs(x[:, a[0]] - np.logical_xor(x[:, a[1]] >= k[0],
                                                       x[:, a[2]] >= k[1]).astype(np.float64))
            elif name == "ABS_SUMDIFF":
                g = np.abs(x[:, a[0]].sum(axis=1) - x[:, a[1]].sum(axis=1))
            elif name == "LCLD_TERM":
                g = np.abs((36 - x[:, a[0]]) * (60 - x[:, a[0]]))
            elif name == "ABS_RATIO":
                g = np.abs(x[:, a[0]] - x[:, a[1]] / x[:, a[2]])
            elif name == "MONTHDIFF":
                g = np.abs(x[:, a[0]] - (_month(x[:, a[1]]) - _month(x[:, a[2]])))
            elif name == "RATIO_MASKED":
                den = x[:, a[2]]
                ratio = np.full(x.shape[0], -1.0)
                nz = den != 0
                ratio[nz] = x[nz, a[1]] / den[nz]
                ratio[ratio == np.inf] = -1
                ratio[np.isnan(ratio)] = -1
                g = np.abs(x[:, a[0]] - ratio)
            elif name == "LCLD_INSTALL":
                x0, x1, x2, x3 = (x[:, i] for i in a)
                calc = (x0 * (x2 / 1200) * (1 + x2 / 1200) ** x1) / ((1 + x2 / 1200) ** x1 - 1)
                g = np.abs(x3 - calc) - k[0]
            else:
                raise ValueError(name)
            cols.append(g)
    c = np.column_stack(cols)
    c[c <= tol] = 0.0
    return c


def restated(mode, ops):
    """Per column: written as an expression under ``mode`` ("all", "mixed" or "")."""
    if mode == "all":
        return [True] * len(ops)
    if mode == "mixed":
        return [c % 3 == 2 and o[0] != "ABS_SUMDIFF" for c, o in enumerate(ops)]
    assert mode == "", mode
    return [False] * len(ops)


def op_expression(name, a, k):
    """One op as an expression, written as moeva2_amd/examples/generic.py writes the shipped
    programs' columns: the same operands in the same order.  (``eval_ops`` above stays the
    statement of the values; tests/test_synth_problem_cpu.py holds this one against it.)"""
    from moeva2_amd.attacks.moeva2.expr import X, absolute, isnan, power, sum_of, where
    from moeva2_amd.examples.generic import _abs_ratio, _month

    if name == "DIFF":
        return X[a[0]] - X[a[1]]
    if name == "RATIO_SAFE":
        return where(X[a[1]] != 0, X[a[0]] / X[a[1]], 0) - k[0]
    if name == "XOR_AUG":
        return absolute(X[a[0]] - ((X[a[1]] >= k[0]) ^ (X[a[2]] >= k[1])))
    if name == "ABS_SUMDIFF":
        return absolute(sum_of(a[0]) - sum_of(a[1]))
    if name == "LCLD_TERM":
        return absolute((36 - X[a[0]]) * (60 - X[a[0]]))
    if name == "ABS_RATIO":
        return _abs_ratio(*a)
    if name == "MONTHDIFF":
        return absolute(X[a[0]] - (_month(X[a[1]]) - _month(X[a[2]])))
    if name == "RATIO_MASKED":
        ratio = X[a[1]] / X[a[2]]
        masked = where((X[a[2]] == 0) | (ratio == float("inf")) | isnan(ratio), -1, ratio)
        return absolute(X[a[0]] - masked)
    if name == "LCLD_INSTALL":
        growth = power(1 + X[a[2]] / 1200, X[a[1]])
        installment = ((X[a[0]] * (X[a[2]] / 1200)) * growth) / (growth - 1)
        return absolute(X[a[3]] - installment) - k[0]
    raise ValueError(name)


class SynthConstraints(TabularConstraints):
    def __init__(self, feature_path, constraints_path, ops, expr=""):
        super().__init__(feature_path, constraints_path)
        self._ops = list(ops)
        self._expr = restated(expr, self._ops)

    def device_program(self) -> ConstraintProgram:
        prog = ConstraintProgram()
        D = int(self._feature_type.shape[0])
        for (name, a, k), x in zip(self._ops, self._expr):
            if x:
                prog.add_expr(op_expression(name, a, k), D)
            elif name == "ABS_SUMDIFF":
                prog.add_sumdiff(list(a[0]), list(a[1]))
            else:
                prog.add(name, a, k)
        return prog


class Scaler:
    def __init__(self, scale, mn):
        self.scale_, self.min_ = scale, mn


def net(dims, seed):
    """Dense relu .. softmax, weights ~ N(0, 1/fan_in), every bias 0.1 * N(0, 1)."""
    rng = np.random.default_rng(seed)
    W = [(rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32)
         for a, b in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * rng.standard_normal(b)).astype(np.float32) for b in dims[1:]]
    return W, bs


def _both_ends(n):
    """0, n-1, 1, n-2, ..."""
    out = []
    for i in range((n + 1) // 2):
        out.append(i)
        if n - 1 - i != i:
            out.append(n - 1 - i)
    return out


class Synth:
    """One built case: ``lay`` / ``problem(x)`` / ``probs`` for the oracle, ``constraints`` /
    ``scaler`` / ``W`` / ``bs`` for the engine, ``X`` the B initial states, ``ops`` / ``codes``
    the program, ``gene_of`` feature -> plain gene."""

    def __init__(self, case: Case, tmp_path):
        self.case = case
        rng = np.random.default_rng(case_seed(case.name))
        # ---- mutable items in feature order
        n_pl, groups = case.n_plain, list(case.ohe)
        items = [("p", j) for j in range(n_pl)]
        mid = groups[1:-1] if len(groups) > 2 else []
        for q, _ in enumerate(mid):
            items.insert((q + 1) * len(items) // (len(mid) + 1), ("o", 1 + q))
        if groups:
            items.insert(0, ("o", 0))
        if len(groups) > 1:
            items.append(("o", len(groups) - 1))
        # ---- the program's shape decides the number of partner (immutable) features
        n_sd = len(case.sumdiff)
        n_lane = case.C - n_sd
        n_imm = case.C + 2
        types, mutable, slots = [], [], []  # slots: per feature ("p", j) | ("o", k) | ("i", q)
        imm_left = n_imm
        since = 0
        for kind, j in items:
            reps = groups[j] if kind == "o" else 1
            for _ in range(reps):
                slots.append((kind, j))
            since += 1
            if since == 3 and imm_left > 0:
                slots.append(("i", n_imm - imm_left))
                imm_left -= 1
                since = 0
        while imm_left > 0:
            slots.append(("i", n_imm - imm_left))
            imm_left -= 1
        D = len(slots)
        self.D = D
        plain_feat = np.array([f for f, s in enumerate(slots) if s[0] == "p"])
        imm_feat = np.array([f for f, s in enumerate(slots) if s[0] == "i"])
        ohe_feat = [np.array([f for f, s in enumerate(slots) if s == ("o", k)])
                    for k in range(len(groups))]
        fixed_in = [tuple(case.fixed(g)) if case.fixed else () for g in range(n_pl)]
        is_int = np.array([case.all_int or g % 3 != 1 or bool(fixed_in[g]) for g in range(n_pl)])
        # ---- static bounds on a 1/8 grid, lower bounds >= 1
        lo = np.where(is_int, rng.integers(1, 4, n_pl), rng.integers(8, 25, n_pl) / 8.0)
        hi = lo + np.where(is_int, rng.integers(4, 13, n_pl), rng.integers(8, 41, n_pl) / 8.0)
        dyn_lo = np.array([g % 7 == 3 and not fixed_in[g] for g in range(n_pl)])
        order = _both_ends(n_pl)
        ints = [g for g in order if is_int[g]]
        term = None
        if case.full:
            term = [g for g in ints if not dyn_lo[g]][len(ints) // 2]
            lo[term], hi[term] = 36.0, 60.0
        # ---- initial states
        X = np.zeros((B, D))
        for s in range(B):
            v = lo + rng.uniform(0.25, 0.75, n_pl) * (hi - lo)
            v = np.where(is_int, np.round(v), v)
            if term is not None:
                v[term] = (36.0, 60.0, 36.0)[s]
            for g in range(n_pl):  # k_mixed: fixed where x_init is the (static) upper bound
                if fixed_in[g] and len(fixed_in[g]) < B:
                    v[g] = hi[g] if s in fixed_in[g] else hi[g] - 2.0
            X[s, plain_feat] = v
            for k, fs in enumerate(ohe_feat):
                X[s, fs[rng.integers(0, len(fs))]] = 1.0
        # ---- the program: (name, args, kargs); mutable operands from both ends
        F = lambda g: int(plain_feat[g])  # noqa: E731
        lo_eff = lambda s, g: X[s, F(g)] if dyn_lo[g] else lo[g]  # noqa: E731
        ops, partner = [], []  # partner[c](s, violated) -> the partner feature's value
        nxt = iter(np.tile(order, 2 + 2 * case.C // max(n_pl, 1)))
        # the equality ops (FULL) keep to a third of the genes, so a redrawn gene often leaves
        # f3 at 0; RATIO_MASKED columns share one denominator gene that no other equality op
        # reads (the rows that set it to 0 / TINY / inf then stay free of NaN)
        eq_set = order[:max(3, n_pl // 3)]
        mden = int(eq_set[-1])
        eq = iter(np.tile(eq_set[:-1], 2 + 6 * case.C))
        imm = iter(imm_feat)

        def eq_pair():
            a = int(next(eq))
            b = int(next(eq))
            while b == a or b == term or a == term:
                a, b = b, int(next(eq))
            return a, b

        def add(name, args, k, fn):
            ops.append((name, tuple(args), tuple(k)))
            partner.append((args, fn))

        if case.full:
            add("LCLD_TERM", (F(term),), (), None)
            kinds = ["ABS_RATIO", "MONTHDIFF", "RATIO_MASKED"]
            n_full = max(3, min(n_lane // 3, 24))
            for q in range(n_full):
                a, b = eq_pair()
                i = int(next(imm))
                nm = kinds[q % 3]
                if nm == "RATIO_MASKED":
                    b = mden
                if nm == "MONTHDIFF":
                    fn = (lambda s, bad, a=a, b=b: _month(X[s, F(a)]) - _month(X[s, F(b)])
                          + (2.0 if bad else 0.0))
                else:
                    fn = (lambda s, bad, a=a, b=b: X[s, F(a)] / X[s, F(b)]
                          + (0.5 if bad else 0.0))
                add(nm, (i, F(a), F(b)), (), (i, fn))
            if case.install:
                a, r = eq_pair()
                i = int(next(imm))

                def inst(s, bad, a=a, r=r):
                    x0, x1, x2 = X[s, F(a)], X[s, F(term)], X[s, F(r)]
                    c = (x0 * (x2 / 1200) * (1 + x2 / 1200) ** x1) / ((1 + x2 / 1200) ** x1 - 1)
                    return c + (1.0 if bad else 0.0)

                add("LCLD_INSTALL", (F(a), F(term), F(r), i), (0.099999,), (i, inst))
        cyc = ["DIFF_mi", "RATIO_im", "DIFF_im", "XOR", "RATIO_mi"]
        if not case.xor:
            cyc.remove("XOR")
        q = 0
        while len(ops) < n_lane:
            nm = cyc[q % len(cyc)]
            q += 1
            g = int(next(nxt))
            if g == term:
                continue
            i = int(next(imm))
            up = (lambda s, bad, g=g: X[s, F(g)] - 1.0 if bad
                  else X[s, F(g)] + 0.6 * (hi[g] - X[s, F(g)]))
            dn = (lambda s, bad, g=g: X[s, F(g)] * 1.5 if bad
                  else X[s, F(g)] - 0.6 * (X[s, F(g)] - lo_eff(s, g)))
            if nm == "DIFF_mi":      # x[m] - x[i] <= 0
                add("DIFF", (F(g), i), (), (i, up))
            elif nm == "DIFF_im":    # x[i] - x[m] <= 0
                add("DIFF", (i, F(g)), (), (i, dn))
            elif nm == "RATIO_im":   # x[i] / x[m] - 1 <= 0: a mutable denominator
                add("RATIO_SAFE", (i, F(g)), (1.0,), (i, dn))
            elif nm == "RATIO_mi":   # x[m] / x[i] - 1 <= 0
                add("RATIO_SAFE", (F(g), i), (1.0,), (i, up))
            else:
                g2 = int(next(nxt))
                k0, k1 = (lo[g] + hi[g]) / 2, (lo[g2] + hi[g2]) / 2
                fn = (lambda s, bad, g=g, g2=g2, k0=k0, k1=k1:
                      float((X[s, F(g)] >= k0) != (X[s, F(g2)] >= k1)) if not bad
                      else 1.0 - float((X[s, F(g)] >= k0) != (X[s, F(g2)] >= k1)))
                add("XOR_AUG", (i, F(g), F(g2)), (k0, k1), (i, fn))
        ipool = iter(np.tile(ints, 2 + sum(case.sumdiff) // max(len(ints), 1)))
        for size in case.sumdiff:
            first = []
            while len(first) < size:
                g = int(next(ipool))
                if g not in first:
                    first.append(g)
            i = int(next(imm))
            fn = (lambda s, bad, first=tuple(first):
                  sum(X[s, F(g)] for g in first) + (3.0 if bad else 0.0))
            add("ABS_SUMDIFF", ([F(g) for g in first], [i]), (), (i, fn))
        assert len(ops) == case.C, (len(ops), case.C)
        bad0 = rng.random(case.C) < 0.6
        for c, (_, pf) in enumerate(partner):
            if pf is None:
                continue
            i, fn = pf
            for s in range(B):
                X[s, i] = fn(s, bool(s == 0 and bad0[c]))
        for i in imm:  # partner features no op took
            X[:, i] = rng.uniform(-1.0, 1.0, B)
        # ---- CSV columns
        tcol, mcol = np.empty(D, object), np.zeros(D, bool)
        fmin, fmax = np.empty(D, object), np.empty(D, object)
        for f, (kind, j) in enumerate(slots):
            if kind == "p":
                tcol[f], mcol[f] = ("int" if is_int[j] else "real"), True
                fmin[f], fmax[f] = repr(float(lo[j])), repr(float(hi[j]))
                if dyn_lo[j] or fixed_in[j]:
                    fmin[f] = "dynamic"
                if len(fixed_in[j]) == B:
                    fmax[f] = "dynamic"
            elif kind == "o":
                tcol[f], mcol[f], fmin[f], fmax[f] = f"ohe{j}", True, "0.0", "1.0"
            else:
                tcol[f], mcol[f] = "real", False
                fmin[f] = repr(float(np.floor(X[:, f].min()) - 1.0))
                fmax[f] = repr(float(np.ceil(X[:, f].max()) + 1.0))
        self.types, self.mutable, self.fmin, self.fmax = tcol, mcol, fmin, fmax
        self.X, self.ops = X, ops
        self.restated = np.array(restated(case.expr, ops), bool)
        self.codes = np.where(self.restated, OP["EXPR"],
                              np.array([OP[o[0]] for o in ops])).astype(np.int32)
        self.plain_feat, self.is_int, self.term = plain_feat, is_int, term
        self.lay = mo.make_layout(mcol, tcol)
        srng = np.random.default_rng(case_seed(case.name) + 500)
        self.ml = (srng.uniform(0.05, 0.5, D), srng.uniform(-0.5, 0.5, D))
        self.scaler = Scaler(*self.ml)
        self.W, self.bs = net((D,) + (case.net or (32, 16, 2)), case_seed(case.name) + 700)
        self.constraints_fn = lambda x: eval_ops(ops, x)
        fpath = os.path.join(str(tmp_path), f"features_{case.name}.csv")
        cpath = os.path.join(str(tmp_path), f"constraints_{case.name}.csv")
        with open(fpath, "w") as fh:
            fh.write("feature,type,mutable,min,max\n")
            for f in range(D):
                fh.write(f"f{f},{tcol[f]},{bool(mcol[f])},{fmin[f]},{fmax[f]}\n")
        with open(cpath, "w") as fh:
            fh.write("min,max\n" + "0.0,1.0\n" * case.C)
        self.constraints = SynthConstraints(fpath, cpath, ops, case.expr)
        self.probs = [self.problem(X[s], mc) for s, mc in zip(range(B), min_classes(case))]

    def expressions(self):
        """{column: expression} of the restated columns."""
        return {c: op_expression(*self.ops[c]) for c in np.where(self.restated)[0]}

    def pool_parity(self):
        """(caller pool entries + code words) & 1: whether the engine pads one word in front
        of the constants it appends to the index pool (api.cpp)."""
        prog = self.constraints.device_program()
        return (len(prog.pool) + len(prog.expr_code)) & 1

    def problem(self, x_init, min_class=1):
        return mo.make_problem(self.lay, x_init, self.fmin, self.fmax, self.ml, self.W, self.bs,
                               self.constraints_fn, min_class, 2, True)

    def gene_of(self, feature):
        return int(np.where(self.plain_feat == feature)[0][0])

    def bounds(self):
        b = [self.constraints.get_feature_min_max(dynamic_input=x) for x in self.X]
        return np.array([v[0] for v in b]), np.array([v[1] for v in b])

    # ---- the rows mv_evaluate is checked on
    def eval_genes(self, rng):
        """(B, n, V) genes and the rows whose f1 is not compared (an infinite gene): 37
        perturbed rows per state (1..5 genes redrawn inside the bounds), then the initial
        genes with a RATIO_SAFE denominator set to 0 (three ops, cycled) and, for FULL
        programs, a RATIO_MASKED denominator set to 0, to TINY (the quotient overflows to
        inf) and to inf (the quotient is 0): all defined outcomes of those ops."""
        lay = self.lay
        isr = np.array([t == "real" for t in mo.genetic_types(lay)])
        den = [self.gene_of(a[1]) for nm, a, _ in self.ops
               if nm == "RATIO_SAFE" and a[1] in self.plain_feat]
        special = [(den[q % len(den)], 0.0) for q in range(3)] if den else []
        if self.case.full:
            md = [self.gene_of(a[2]) for nm, a, _ in self.ops if nm == "RATIO_MASKED"]
            special += [(md[0], 0.0), (md[-1], TINY), (md[0], np.inf)]
        n = N_PERTURBED + len(special)
        genes = np.empty((B, n, lay.V))
        for b, prob in enumerate(self.probs):
            gl, gu = mo.genetic_bounds(lay, prob.xl, prob.xu)
            g = np.repeat(mo.initial_population(prob, 1), n, axis=0)
            for r in range(N_PERTURBED):
                k = rng.integers(0, lay.V, size=1 + r % 5)
                v = rng.uniform(gl[k], gu[k])
                g[r, k] = np.where(isr[k], v, np.round(v))
            for q, (gene, val) in enumerate(special):
                g[N_PERTURBED + q, gene] = val
            genes[b] = g
        inf_rows = np.array([N_PERTURBED + q for q, (_, v) in enumerate(special) if v == np.inf],
                            dtype=int)
        return genes, inf_rows


def build(case, tmp_path) -> Synth:
    if isinstance(case, str):
        case = CASES_BY_NAME[case] if case in CASES_BY_NAME else MLP_BY_NAME[case]
    return Synth(case, tmp_path)


def engine_shape(case: Case, sy: Synth, fixed=None):
    """(V, Dm4, C, ident, full_ops, n_sumdiff, compact, slim) of the attack's problem as
    csrc/api.cpp build_problem derives them (``fixed``: the compact layout's feature mask)."""
    nfix = 0 if fixed is None else int(np.asarray(fixed).sum())
    V, Dm = case.V - nfix, case.Dm - nfix
    names = ["EXPR" if x else o[0] for o, x in zip(sy.ops, sy.restated)]
    lane = [o for o in names if o != "ABS_SUMDIFF"]
    full = any(o in ("LCLD_INSTALL", "LCLD_TERM", "ABS_RATIO", "MONTHDIFF", "RATIO_MASKED")
               for o in lane)
    if "EXPR" in lane:  # an EXPR column: the interpreter instances
        full = 2
    slim = (case.ident and len(lane) <= 64 * 6 and Dm + sy.D < 0x4000
            and all(o in ("DIFF", "RATIO_SAFE") for o in lane))
    return dict(V=V, Dm4=(Dm + 15) // 16 * 16, C=case.C, ident=int(case.ident),
                full_ops=int(full), sd=len(names) - len(lane), compact=int(nfix > 0),
                slim=int(slim))
