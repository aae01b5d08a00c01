"""MV_OP_EXPR on the device: the shipped LCLD / botnet programs written as generic expressions
equal the dedicated ops bit for bit, every instruction equals its numpy statement, the lane
and column loops hold at their edge shapes, mv_engine_create refuses malformed bytecode, and
the generic programs run through mv_evaluate, the attack and the ObjectiveCalculator.
k_constraintsx's row load at D on both sides of 64 and of a second lane trip, the constant
table on both alignment parities, sum_of pools from 0 to 300 entries and the program that just
fits the LDS (tests/expr_edges.py) close the file.  (The ten k_consx<IDENT, NT> instances are
pinned by the x cases of tests/test_gpu_row_routes.py.)"""
import json
import os

import numpy as np
import pytest

import expr_edges as ee
import synth_problem as sp
from conftest import RES
from oracle import moeva_oracle as mo
from oracle.problems import PROJECTS, Project
from test_expr_cpu import POW_COLUMN, coverage_program, edge_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def feat_path(name):
    return os.path.join(RES, PROJECTS[name][0])


def dedicated(name):
    from moeva2_amd.experiments.united.utils import STR_TO_CONSTRAINTS_CLASS

    feat = feat_path(name)
    return STR_TO_CONSTRAINTS_CLASS[name](feat, feat.replace("features", "constraints"))


def generic_exprs(name):
    from moeva2_amd.examples.generic import botnet_expressions, lcld_expressions

    if name == "lcld":
        return lcld_expressions()
    with open(os.path.join(RES, "data", "botnet", "feat_idx.json")) as f:
        return botnet_expressions(json.load(f))


def generic(name):
    from moeva2_amd.attacks.moeva2.constraints import ExprConstraints

    feat = feat_path(name)
    return ExprConstraints(feat, feat.replace("features", "constraints"), generic_exprs(name))


class NpScaler:
    def __init__(self, path):
        d = np.load(path)
        self.scale_, self.min_ = d["scale_"], d["min_"]


def scaler(name):
    return NpScaler(os.path.join(RES, PROJECTS[name][2]))


def classifier(name):
    from moeva2_amd.attacks.moeva2.classifier import Classifier, load_model

    return Classifier(load_model(os.path.join(RES, PROJECTS[name][1])))


def device_program(prog, D, tol=1e-3):
    """A constraints-only problem over D real features around a ConstraintProgram."""
    from moeva2_amd._native import DeviceProgram

    code, arg, karg, pool = prog.arrays()
    xcode, xconst = prog.expr_arrays()
    return DeviceProgram(D=D, gene_kind=np.zeros(D, np.int32), gene_feat=np.arange(D, dtype=np.int32),
                         ohe_offsets=np.zeros(1, np.int32), ohe_feats=np.zeros(0, np.int32),
                         mut_feats=np.arange(D, dtype=np.int32), op_code=code, op_arg=arg,
                         op_karg=karg, idx_pool=pool, tol=tol, expr_code=xcode, expr_const=xconst)


def run_constraints(dp, x, check_f3=True):
    """G of mv_constraints on the rows x (k_constraintsx: one wave per row).  The same rows go
    through mv_evaluate as the genes of one state (k_gen + k_consx: the real genes are the
    features), whose G is the positive part of the same values and whose f3 is their sum."""
    from moeva2_amd._native import Engine

    eng = Engine(dp, None, None)
    n, D = x.shape
    xd = torch.as_tensor(np.ascontiguousarray(x, np.float64), device="cuda")
    g = torch.full((n, dp.C), -7.0, dtype=torch.float64, device="cuda")
    eng.constraints(xd, g)
    g = g.cpu().numpy()
    eng.set_states(np.zeros((1, D)), np.full((1, D), -5.0), np.full((1, D), 5.0), 0)
    assert eng.kernel_times()["row_kernel"] == "k_gen+k_cons"  # never k_narrow or k_genc
    F = torch.full((1, n, 3), -7.0, dtype=torch.float64, device="cuda")
    Ge = torch.full((1, n, dp.C), -7.0, dtype=torch.float64, device="cuda")
    eng.evaluate(xd[None], F, Ge)
    with np.errstate(invalid="ignore"):
        pos = g * (g > 0)  # default_problem.py:93-97 (NaN stays NaN)
    np.testing.assert_array_equal(Ge.cpu().numpy()[0], pos)
    if check_f3:  # non-negative terms in any order: (C - 1) roundings
        np.testing.assert_allclose(F.cpu().numpy()[0, :, 2], pos.sum(axis=1),
                                   rtol=max(dp.C - 1, 1) * 2.0 ** -53, atol=0)
    return g


# ------------------------------------------------------------------ mv_constraints
@pytest.mark.parametrize("name", ["lcld", "botnet"])
def test_generic_program_equals_dedicated_ops_bit_for_bit(golden, name):
    d = golden(f"{name}_constraints.npz")
    g = generic(name).evaluate(d["x"])
    np.testing.assert_array_equal(g > 0, d["g"] > 0)  # the dedicated programs' assertions
    np.testing.assert_allclose(g, d["g"], rtol=1e-12, atol=0)
    gd = dedicated(name).evaluate(d["x"])
    np.testing.assert_array_equal(g, gd)  # same operations, same order, no contraction
    assert (g[:, 0] > 0).any()  # LCLD: the installment column (POW); botnet: ABS_SUMDIFF


def test_every_instruction_equals_numpy_on_the_device():
    """The coverage program on the edge rows (0/0, x/0, NaN, infinities, negative mod / floor
    operands): exactly evaluate_numpy's values, NaN in the same places.  POW is left out of
    the exact comparison (the device's pow is not numpy's to the last bit); it is checked
    through the LCLD installment column above and here to 17 ulp (OpenCL's bound for a
    double-precision pow is 16 ulp, the host libm's 1).  tol = -inf: only a -inf
    value is clamped, on both sides alike."""
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram

    x = edge_rows()
    exprs = [e for e, _ in coverage_program()] + [POW_COLUMN[0]]
    prog = ConstraintProgram()
    for e in exprs:
        prog.add_expr(e, x.shape[1])
    g = run_constraints(device_program(prog, x.shape[1], tol=-INF), x, check_f3=False)
    ref = E.evaluate_numpy(exprs, x, tol=-INF)
    np.testing.assert_array_equal(g[:, :-1], ref[:, :-1])
    assert np.isnan(ref[:, :-1]).any() and np.isinf(ref[:, :-1]).any()
    np.testing.assert_array_equal(np.isnan(g[:, -1]), np.isnan(ref[:, -1]))
    np.testing.assert_allclose(g[:, -1], ref[:, -1], rtol=17 * 2.0 ** -52, atol=0)


def shape_column(c):
    """Column c of the shape programs: a few forms over 12 features, no POW."""
    from moeva2_amd.attacks.moeva2.expr import X, absolute, floor, maximum, mod, sum_of, where

    a, b, k = X[c % 12], X[(5 * c + 1) % 12], 0.25 * (c % 7) - 0.5
    forms = [lambda: a - b + k, lambda: where(b != 0, a / b, k) - 1, lambda: absolute(a * k - b),
             lambda: maximum(a, b) - floor(a), lambda: mod(a, 3) + k,
             lambda: absolute(sum_of([c % 12, (c + 1) % 12, (c + 2) % 12]) - 1.5 * b)]
    return forms[c % len(forms)]()


@pytest.mark.parametrize("C", [1, 64, 65, 400])  # 400 crosses 64 * OPS_REG
@pytest.mark.parametrize("n", [1, 65, 130])
def test_shapes_rows_and_columns(n, C):
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram

    rng = np.random.default_rng(100 * n + C)
    x = np.round(rng.uniform(-4, 4, size=(n, 12)), 2)
    x[rng.random(x.shape) < 0.1] = 0.0
    exprs = [shape_column(c) for c in range(C)]
    prog = ConstraintProgram()
    for e in exprs:
        prog.add_expr(e, 12)
    g = run_constraints(device_program(prog, 12), x)
    np.testing.assert_array_equal(g, E.evaluate_numpy(exprs, x))


def test_interleaved_dedicated_and_expr_columns_keep_their_places():
    """DIFF, ABS_SUMDIFF and EXPR columns interleaved: the engine sorts the ops by code
    (ABS_SUMDIFF last) and op_col sends every value back to its column.  Integer features,
    so the wave-parallel ABS_SUMDIFF sum is exact."""
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram
    from moeva2_amd.attacks.moeva2.expr import X, absolute, sum_of

    rng = np.random.default_rng(3)
    x = rng.integers(-9, 10, size=(70, 12)).astype(np.float64)
    prog, same = ConstraintProgram(), []
    for c in range(45):
        a, b = c % 12, (7 * c + 3) % 12
        first, second = [a, b, (a + 1) % 12], [(b + 2) % 12, (a + 5) % 12]
        if c % 3 == 0:
            prog.add("DIFF", (a, b))
            same.append(X[a] - X[b])
        elif c % 3 == 1:
            prog.add_sumdiff(first, second)
            same.append(absolute(sum_of(first) - sum_of(second)))
        else:
            e = absolute(X[a] * 2 - sum_of(second)) + c
            prog.add_expr(e, 12)
            same.append(e)
    g = run_constraints(device_program(prog, 12), x)
    np.testing.assert_array_equal(g, E.evaluate_numpy(same, x))
    assert len({tuple(col) for col in g.T}) >= 16  # the columns differ: a swap would show


def test_columns_at_the_stack_and_word_limits():
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram
    from moeva2_amd.attacks.moeva2.expr import X, absolute
    from test_expr_cpu import _long

    nest = X[7]  # right-nested: all eight operands are on the stack before the first operator
    for f in range(6, -1, -1):
        nest = X[f] - nest
    longest = absolute(-_long((E.MAX_WORDS - 4) // 3))
    exprs = [nest, longest]
    prog = ConstraintProgram()
    for e in exprs:
        prog.add_expr(e, 8)
    arg = prog.arrays()[1]
    assert arg[0][2] == E.MAX_DEPTH and arg[1][1] == E.MAX_WORDS
    rng = np.random.default_rng(5)
    x = np.round(rng.uniform(-3, 3, size=(66, 8)), 3)
    g = run_constraints(device_program(prog, 8), x)
    np.testing.assert_array_equal(g, E.evaluate_numpy(exprs, x))


# ------------------------------------------------------------------ mv_engine_create
X_, K_, SUMF_, ADD_, WHERE_ = 1, 2, 3, 4, 27
MALFORMED = {
    "unknown opcode": ([X_, 0, 99], 1),
    "opcode zero": ([0], 1),
    "negative opcode": ([-4], 1),
    "feature past D": ([X_, 6], 1),
    "negative feature": ([X_, -1], 1),
    "constant past the table": ([K_, 2], 1),
    "negative constant": ([K_, -1], 1),
    "pool range past n_pool": ([SUMF_, 0, 4], 1),
    "pool range reversed": ([SUMF_, 2, 1], 1),
    "pool range negative": ([SUMF_, -1, 1], 1),
    "pool entry no feature": ([SUMF_, 2, 3], 1),
    "underflow binary": ([X_, 0, ADD_], 1),
    "underflow where": ([X_, 0, X_, 1, WHERE_], 2),
    "underflow first": ([ADD_], 1),
    "two values left": ([X_, 0, X_, 1], 2),
    "deeper than declared": ([X_, 0, X_, 1, X_, 2, ADD_, ADD_], 2),
    "deeper than the limit": ([X_, 0] * 9 + [ADD_] * 8, 9),
    "declared depth zero": ([X_, 0], 0),
    "operand cut off": ([X_, 0, X_], 1),
    "sumf operand cut off": ([SUMF_, 0], 1),
    "too many words": ([X_, 0] + [X_, 0, ADD_] * 85, 2),
}


@pytest.mark.parametrize("case", list(MALFORMED) + ["empty column", "range past the code",
                                                    "negative offset", "no code table"])
def test_engine_create_refuses_malformed_bytecode(case):
    """Built through _native directly (the Python compiler would not emit them): MV_ERR_ARG
    with a message, before any kernel could interpret the words."""
    from moeva2_amd._native import DeviceProgram, Engine, NativeError

    D = 6
    words, depth = MALFORMED.get(case, ([X_, 0], 1))
    arg = [0, len(words), depth, 0]
    if case == "empty column":
        arg[1] = 0
    elif case == "range past the code":
        arg[0] = 1
    elif case == "negative offset":
        arg[0] = -1
    xcode = np.zeros(0, np.int32) if case == "no code table" else np.asarray(words, np.int32)
    dp = DeviceProgram(D=D, gene_kind=np.zeros(D, np.int32), gene_feat=np.arange(D, dtype=np.int32),
                       ohe_offsets=np.zeros(1, np.int32), ohe_feats=np.zeros(0, np.int32),
                       mut_feats=np.arange(D, dtype=np.int32),
                       op_code=np.array([1, 16], np.int32),
                       op_arg=np.array([[0, 1, 0, 0], arg], np.int32), op_karg=np.zeros((2, 2)),
                       idx_pool=np.array([0, 1, 6], np.int32), expr_code=xcode,
                       expr_const=np.array([1.0, 2.0]))
    with pytest.raises(NativeError, match="error 1: .*MV_OP_EXPR"):
        Engine(dp, None, None)


def test_engine_create_accepts_the_same_table_when_well_formed():
    from moeva2_amd._native import DeviceProgram, Engine

    D = 6
    dp = DeviceProgram(D=D, gene_kind=np.zeros(D, np.int32), gene_feat=np.arange(D, dtype=np.int32),
                       ohe_offsets=np.zeros(1, np.int32), ohe_feats=np.zeros(0, np.int32),
                       mut_feats=np.arange(D, dtype=np.int32),
                       op_code=np.array([1, 16], np.int32),
                       op_arg=np.array([[0, 1, 0, 0], [0, 7, 2, 0]], np.int32),
                       op_karg=np.zeros((2, 2)), idx_pool=np.array([0, 1, 6], np.int32),
                       expr_code=np.array([SUMF_, 0, 2, K_, 1, ADD_, 22], np.int32),
                       expr_const=np.array([1.0, 2.0]))
    x = np.array([[1.0, -8.0, 0, 0, 0, 0]])
    xd = torch.as_tensor(x, device="cuda")
    g = torch.empty((1, 2), dtype=torch.float64, device="cuda")
    Engine(dp, None, None).constraints(xd, g)
    np.testing.assert_array_equal(g.cpu().numpy(), [[9.0, 5.0]])


# ------------------------------------------------------------------ mv_evaluate
def test_evaluate_generic_lcld_against_dedicated(golden):
    from moeva2_amd.problem import get_engine

    d = golden("problem_lcld.npz")
    X = d["x_init"]
    genes = np.stack([d[f"s{s}_genes"] for s in range(X.shape[0])])
    out = []
    for c in (generic("lcld"), dedicated("lcld")):
        eng = get_engine(c, classifier("lcld"), scaler("lcld"), 2)
        bounds = [c.get_feature_min_max(dynamic_input=x) for x in X]
        eng.set_states(X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]), 1)
        gd = torch.as_tensor(genes, device="cuda")
        F0 = torch.empty(genes.shape[:2] + (3,), dtype=torch.float64, device="cuda")
        F1 = torch.empty_like(F0)
        G = torch.empty(genes.shape[:2] + (10,), dtype=torch.float64, device="cuda")
        eng.evaluate(gd, F0)
        eng.evaluate(gd, F1, G)
        out.append((F0.cpu().numpy(), F1.cpu().numpy(), G.cpu().numpy(), eng))
    (F0g, F1g, Gg, eg), (F0d, F1d, Gd, _) = out
    assert eg.kernel_times()["row_kernel"] == "k_gen+k_cons"  # not k_narrow
    np.testing.assert_array_equal(F0g, F1g)  # with and without G
    np.testing.assert_array_equal(F1g[..., :2], F1d[..., :2])
    np.testing.assert_array_equal(Gg, Gd)
    assert (Gg > 0).any()
    # identical non-negative columns; only the lane order of their sum differs
    np.testing.assert_allclose(F1g[..., 2], F1d[..., 2], rtol=9 * 2.0 ** -53, atol=0)


# ------------------------------------------------------------------ attack
@pytest.mark.parametrize("norm", [2, np.inf])
def test_attack_with_generic_lcld_constraints(norm):
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2

    p = Project("lcld")
    X = p.x[:3]
    c = generic("lcld")
    m = Moeva2(os.path.join(RES, PROJECTS["lcld"][1]), c, ml_scaler=scaler("lcld"), norm=norm,
               n_gen=6, n_pop=40, n_offsprings=20, save_history="full", seed=9)
    g_d, F_d, h_d = m.generate(X, 1, return_device=True)
    genes, F, hist = g_d.cpu().numpy(), F_d.cpu().numpy(), h_d.cpu().numpy()
    P, O, tol = 43, 20, c.tol
    assert hist.shape == (3, P + 5 * O, 3 + 10)
    for b in range(3):
        x_f = mo.genetic_to_ml(p.lay, genes[b], X[b])
        f3 = E.evaluate_numpy(c.expressions, x_f).sum(axis=1)
        print("state", b, "max relative f3 difference",
              np.max(np.abs(F[b, :, 2] - f3) / np.where(f3 > 0, f3, 1.0)))
        np.testing.assert_allclose(F[b, :, 2], f3, rtol=9 * 2.0 ** -53, atol=0)
    G = hist[:, :, 3:]
    assert np.isfinite(G).all()
    assert ((G == 0) | (G > tol)).all()
    assert (G > tol).any()


# ------------------------------------------------------------------ ObjectiveCalculator
def test_objective_calculator_with_generic_botnet_constraints(golden):
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator

    d = golden("objective_calculator_botnet.npz")
    sc = scaler("botnet")
    calc = ObjectiveCalculator(classifier("botnet"), generic("botnet"), minimize_class=1,
                               thresholds={"f1": 0.5, "f2": 4}, min_max_scaler=sc, norm=2,
                               ml_scaler=sc)
    obj = calc.calculate_objectives_3d(d["x_init"], d["x_attacks"])
    for i in range(4):
        np.testing.assert_allclose(obj[i][..., 0], d[f"obj{i}"][..., 0], rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(calc._objective_respected(obj[i]), d[f"resp{i}"])
        np.testing.assert_array_equal(calc._objective_array(d["x_init"][i], d["x_attacks"][i]),
                                      d[f"resp{i}"])
    np.testing.assert_array_equal(calc.success_rate_3d(d["x_init"], d["x_attacks"]),
                                  d["success_rate"])


# ------------------------------------------------------------------ rows, tables and LDS at their edges
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [1, 3, 4, 5])  # one row, a partly filled workgroup, a full one,
@pytest.mark.parametrize("D", [63, 64, 65, 129])  # one row alone in a second workgroup
def test_constraintsx_rows_of_larger_d(D, n):
    """k_constraintsx keeps four rows of D doubles per workgroup and loads each with a lane
    loop: D below, at and above one trip and above two.  G is preset to a sentinel
    (run_constraints), so a row or column left unwritten shows; the same rows go through
    k_gen + k_consx<true, NT>."""
    from moeva2_amd.attacks.moeva2 import expr as E

    exprs = ee.wide_columns(D)
    x = ee.wide_rows(D, n, 1000 * D + n)
    g = run_constraints(device_program(ee.program(exprs, D), D), x)
    np.testing.assert_array_equal(g, E.evaluate_numpy(exprs, x))
    assert (g > 0).any()


def test_constraintsx_on_the_widest_synthetic_program(tmp_path):
    """x1024's program (D 1326, a third of its 300 columns expressions): mv_constraints on 1, 3,
    4 and 5 of the rows the row-route case evaluates; the restated columns against
    evaluate_numpy, the dedicated ones against the ops' numpy statement, bit for bit."""
    from moeva2_amd._native import Engine
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.problem import build_device_program

    sy = sp.build("x1024", tmp_path)
    genes, _ = sy.eval_genes(np.random.default_rng(5))
    rows = mo.genetic_to_ml(sy.lay, genes[0], sy.probs[0].x_init)
    cols = sy.expressions()
    idx = sorted(cols)
    rest = np.setdiff1d(np.arange(sy.case.C), idx)
    eng = Engine(build_device_program(sy.constraints), None, None)
    assert sy.D == 1326 and len(idx) == 100
    for n in (1, 3, 4, 5):
        x = np.ascontiguousarray(rows[7:7 + n])
        g = torch.full((n, sy.case.C), -7.0, dtype=torch.float64, device="cuda")
        eng.constraints(torch.as_tensor(x, device="cuda"), g)
        g = g.cpu().numpy()
        np.testing.assert_array_equal(g[:, idx], E.evaluate_numpy([cols[c] for c in idx], x))
        np.testing.assert_array_equal(g[:, rest], sp.eval_ops(sy.ops, x)[:, rest])
        assert (g > 0).any()


@pytest.mark.parametrize("odd", [False, True], ids=["constants-aligned", "constants-padded"])
def test_constants_come_back_bit_for_bit(odd):
    """40 constants (-0.0, 5e-324, the largest double, inf, a NaN with a payload among them),
    each returned by a column of its own through a select; with a five-word column in front the
    code words are odd in number and the engine pads one word before the table.  tol = -inf:
    no value here is clamped."""
    from moeva2_amd.attacks.moeva2 import expr as E

    exprs = ee.constant_columns(odd)
    prog = ee.program(exprs, 2)
    assert ee.const_parity(prog) == int(odd)
    x = np.array([[1.0, 1.0], [2.5, -0.0], [-3.0, 0.25]])
    g = run_constraints(device_program(prog, 2, tol=-INF), x, check_f3=False)
    k = ee.constants()
    np.testing.assert_array_equal(bits(g[:, int(odd):]), np.tile(bits(k), (3, 1)))
    np.testing.assert_array_equal(bits(g), bits(E.evaluate_numpy(exprs, x, tol=-INF)))


def test_sum_of_pools_from_empty_to_300_entries():
    """Left to right from 0.0 on both sides, over non-integer features: the same bits.  The
    empty pool gives +0.0, and so does the pool of one feature that is -0.0."""
    from moeva2_amd.attacks.moeva2 import expr as E

    exprs, pools = ee.sumf_columns()
    x = ee.sumf_rows()
    g = run_constraints(device_program(ee.program(exprs, ee.SUMF_D), ee.SUMF_D, tol=-INF), x,
                        check_f3=False)
    np.testing.assert_array_equal(bits(g), bits(E.evaluate_numpy(exprs, x, tol=-INF)))
    assert (bits(g[:, 0]) == 0).all() and (bits(g[:3, -1]) == 0).all()


@pytest.mark.parametrize("columns", [ee.LDS_BOUND_COLUMNS],
                         ids=[f"{ee.LDS_BOUND_COLUMNS}-columns"])
def test_program_at_the_lds_bound(columns):
    """The largest program of maximal (256-word) columns over 12 features whose constraint
    workspace fits the CU's 160 KiB (the count is the header's: tests/test_expr_edges_cpu.py) is
    accepted and evaluated; one more column is refused when the engine is created."""
    from moeva2_amd._native import Engine, NativeError
    from moeva2_amd.attacks.moeva2 import expr as E

    D = ee.LDS_BOUND_D
    exprs = ee.bound_columns(columns + 1)
    x = np.round(np.random.default_rng(12).uniform(-2, 2, size=(5, D)), 3) + 0.0625
    g = run_constraints(device_program(ee.program(exprs[:-1], D), D), x)
    ref = E.evaluate_numpy(exprs[:-1], x)
    np.testing.assert_array_equal(g, ref)
    assert len({tuple(c) for c in g.T}) == columns and (g > 0).all()
    with pytest.raises(NativeError, match="error 1: .*too large"):
        Engine(device_program(ee.program(exprs, D), D), None, None)
