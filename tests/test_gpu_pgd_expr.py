"""C-PGD on user-defined constraint expressions (MV_OP_EXPR tensor-path columns: k_pgd<true> /
k_pgd_grad<true>, csrc/pgd_expr.h).

The shipped tensor paths written as expressions (examples/generic.py) must give the dedicated
tensor programs' columns bit for bit and a gradient that obeys the rule of
test_gpu_pgd.py::test_gradient_matches_fp64_autograd; a coverage program with every opcode is
compared with ``expr.evaluate_grad_numpy`` and with fp64 autograd (tests/expr_torch_ref.py).
Shapes: LCLD n = 33 (two tiles and a one-row tail), botnet n = 17, the coverage problem D = 8
with the identity scaler and a fixed-seed 8-16-2 net, n = 17.

Measured (engine error / tolerance, MI355X): DESIGN.md section 7c.
"""
import os

import numpy as np
import pytest
import torch

import expr_torch_ref as xref
import pgd_torch_ref as ref
from test_gpu_pgd import (EPS, N, _assert_matches, _get, _kept_rows, _rel, _tiled, synthetic_net)

pytestmark = pytest.mark.gpu

RES = ref.RES
HEADLINE = "constraints+flip+adaptive_eps_step"
MAX_EXCLUDED = 3


class Generic:
    """The dedicated Case of a project and the same problem as an ExprConstraints estimator."""

    def __init__(self, project):
        from moeva2_amd.attacks.moeva2.constraints import ExprConstraints
        from moeva2_amd.attacks.pgd.classifier import TF2Classifier
        from moeva2_amd.examples import generic as G

        self.case = case = _get(project)
        feat = os.path.join(RES, "data", project, "features.csv")
        if project == "lcld":
            exprs, texprs = G.lcld_expressions(), G.lcld_tensor_expressions()
        else:
            fi = ref.load_feat_idx()
            exprs, texprs = G.botnet_expressions(fi), G.botnet_tensor_expressions(fi)
        self.texprs = texprs
        self.c = ExprConstraints(feat, feat.replace("features", "constraints"), exprs, texprs)
        self.est = TF2Classifier(case.model, self.c, case.scaler,
                                 parameters={"constraints_optim": "sum"})


_GEN = {}


def _gen(project):
    if project not in _GEN:
        _GEN[project] = Generic(project)
    return _GEN[project]


@pytest.fixture(params=["lcld", "botnet"])
def gen(request):
    return _gen(request.param)


def _program(exprs, D):
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram

    prog = ConstraintProgram()
    for e in exprs:
        prog.add_expr(e, D, max_tape=E.MAX_TAPE)
    return prog


def _small_pgd(prog, D=8, tol=xref.TOL):
    """The coverage problem's engine: identity scaler, a fixed-seed D-16-2 net, all mutable."""
    from moeva2_amd._native import Pgd

    W, b = synthetic_net((D, 16, 2), 3)
    return Pgd(prog, W, b, np.ones(D), np.zeros(D), np.ones(D, bool), tol=tol)


def _grad(pgd, x, flags=None):
    from moeva2_amd._native import PGD_LOSS_CONSTRAINTS

    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    y = torch.zeros(xd.shape[0], dtype=torch.int32, device="cuda")
    g = torch.empty_like(xd)
    losses = torch.empty((xd.shape[0], 2 + pgd.C), dtype=torch.float32, device="cuda")
    pgd.grad(xd, y, PGD_LOSS_CONSTRAINTS if flags is None else flags, g, losses)
    torch.cuda.synchronize()
    return g.cpu().numpy(), losses.cpu().numpy()


def _rule2(name, g, g64, g32):
    """test_gradient_matches_fp64_autograd's rule: error relative to the row's gradient
    inf-norm, at most 4x the helper's own fp32-vs-fp64 error on the same rows (floor 2^-23)."""
    gs = np.maximum(np.abs(g64).max(1, keepdims=True), 1e-30)
    floor = max(_rel(g32, g64, gs), 2.0 ** -23)
    err = _rel(g, g64, gs)
    print(f"{name}: gradient err {err:.3e} (floor {floor:.3e})")
    assert np.isfinite(g).all()
    assert err <= 4 * floor


# ---- 1. columns ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["candidates", "perturbed"])
def test_columns_equal_the_dedicated_program(gen, which):
    case = gen.case
    x, y = case.inputs[which], case.y[which]
    _, want = case.est.losses_and_gradient(x, y, "constraints+flip")
    _, got = gen.est.losses_and_gradient(x, y, "constraints+flip")
    assert got.shape == (N[case.project], 2 + gen.c.get_nb_constraints())
    np.testing.assert_array_equal(got, want)  # loss_class, the sum and every column
    if which == "perturbed":
        assert (got[:, 2:] > 0).any()


# ---- 2. gradient -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["constraints", "constraints+flip"])
@pytest.mark.parametrize("which", ["candidates", "perturbed"])
def test_gradient_matches_fp64_autograd(gen, which, mode):
    case = gen.case
    (g64, *_), (g32, *_) = case.grad_refs(which, mode)
    g, _ = gen.est.losses_and_gradient(case.inputs[which], case.y[which], mode)
    _rule2(f"generic {case.project} {which} {mode}", g, g64.numpy(), g32.numpy())


# ---- 3. coverage program ---------------------------------------------------------------------
def test_coverage_program_on_the_device():
    from moeva2_amd.attacks.moeva2 import expr as E

    exprs, x = xref.coverage_program(), xref.coverage_rows(17)
    g, losses = _grad(_small_pgd(_program(exprs, 8)), x)
    c32, g32 = E.evaluate_grad_numpy(exprs, x, tol=xref.TOL, dtype=np.float32)
    c64, g64 = xref.cols_and_grad(exprs, x, torch.float64)
    h32 = xref.cols_and_grad(exprs, x, torch.float32)[1]
    # every column without a transcendental is the fp32 statement's bit for bit
    exact = [j for j in range(len(exprs)) if j != 3]
    np.testing.assert_array_equal(losses[:, 2:][:, exact], c32[:, exact])
    cs = 1 + np.abs(c64).max(1, keepdims=True)
    floor_c = max(_rel(xref.cols_and_grad(exprs, x, torch.float32)[0], c64, cs), 2.0 ** -23)
    err_c = _rel(losses[:, 2:], c64, cs)
    print(f"coverage: columns err {err_c:.3e} (floor {floor_c:.3e})")
    assert err_c <= 4 * floor_c
    # mode constraints, identity scaler: the device gradient is -d(sum of columns)/dx
    _rule2("coverage vs fp64 autograd", -g, g64, h32)
    gs = np.maximum(np.abs(g64).max(1, keepdims=True), 1e-30)
    err = _rel(-g, g32, gs)
    print(f"coverage vs evaluate_grad_numpy fp32: gradient err {err:.3e}")
    assert err <= 4 * max(_rel(h32, g64, gs), 2.0 ** -23)
    assert (np.abs(g).max(0) > 0).all()


@pytest.mark.parametrize("kink", xref.KINKS, ids=[k[0] for k in xref.KINKS])
def test_kink_rows_exactly(kink):
    _, e, row, entries = kink
    g, _ = _grad(_small_pgd(_program([e], 8)), np.array([row]))
    np.testing.assert_array_equal(-g[0], xref.kink_expected(entries))


# ---- 4. mixed program ------------------------------------------------------------------------
def test_mixed_program_keeps_every_column_in_place():
    from moeva2_amd._native import PGD_LOSS_CONSTRAINTS, PGD_LOSS_FLIP, Pgd
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram

    gen = _gen("lcld")
    case = gen.case
    ded = case.c.tensor_program()
    prog = ConstraintProgram()
    for j in range(len(ded)):  # dedicated ops on the even columns, expressions on the odd ones
        if j % 2 == 0:
            prog.code.append(ded.code[j])
            prog.arg.append(ded.arg[j])
            prog.karg.append(ded.karg[j])
        else:
            prog.add_expr(gen.texprs[j], 47, max_tape=E.MAX_TAPE)
    mlp = case.model.dense_weights()
    pgd = Pgd(prog, mlp.weights, mlp.biases, case.scaler.scale_, case.scaler.min_, case.mask,
              *case.c.tensor_repair())
    which, mode = "perturbed", "constraints+flip"
    x, y = case.inputs[which], case.y[which]
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    g = torch.empty_like(xd)
    losses = torch.empty((x.shape[0], 12), dtype=torch.float32, device="cuda")
    pgd.grad(xd, yd, PGD_LOSS_FLIP | PGD_LOSS_CONSTRAINTS, g, losses)
    torch.cuda.synchronize()
    _, want = case.est.losses_and_gradient(x, y, mode)
    np.testing.assert_array_equal(losses.cpu().numpy(), want)
    (g64, *_), (g32, *_) = case.grad_refs(which, mode)
    _rule2("mixed lcld", g.cpu().numpy(), g64.numpy(), g32.numpy())


# ---- 5. limits and refusals ------------------------------------------------------------------
def test_columns_at_the_limits():
    from moeva2_amd.attacks.moeva2 import expr as E
    from moeva2_amd.attacks.moeva2.expr import X, absolute

    deep = X[7]
    for f in range(6, -1, -1):  # x0 + (x1 + (... + x7)): eight operands on the stack
        deep = X[f] + deep
    chain = X[0]
    for _ in range(31):
        chain = chain + 1.0
    full = absolute(chain)  # 1 + 31 * 2 + 1 = MV_EXPR_MAX_TAPE instructions
    assert E.stack_depth(E.compile_expr(deep)[0]) == E.MAX_DEPTH
    assert E.tape_length(E.compile_expr(full)[0]) == E.MAX_TAPE
    x = xref.coverage_rows(17)
    g, losses = _grad(_small_pgd(_program([deep + 64, full], 8)), x)
    c32, g32 = E.evaluate_grad_numpy([deep + 64, full], x, tol=xref.TOL, dtype=np.float32)
    np.testing.assert_array_equal(losses[:, 2:], c32)
    np.testing.assert_array_equal(-g, g32)
    assert (g32[:, 1:] == 1).all() and set(np.unique(g32[:, 0])) == {2.0}


class _RawProgram:
    """Tables handed to mv_pgd_create as they are (the Python compiler would not emit them)."""

    def __init__(self, words, arg, pool=(0, 1, 2)):
        self.tables = (np.array([1, 16], np.int32), np.array([[0, 1, 0, 0], arg], np.int32),
                       np.zeros((2, 2)), np.asarray(pool, np.int32))
        self.words = np.asarray(words, np.int32)

    def arrays(self):
        return self.tables

    def expr_arrays(self):
        return self.words, np.array([1.0, 2.0])


def _refusal_cases():
    from test_gpu_expr import MALFORMED

    cases = {k: (w, [0, len(w), d, 0]) for k, (w, d) in MALFORMED.items()}
    cases["empty column"] = ([1, 0], [0, 0, 1, 0])
    cases["range past the code"] = ([1, 0], [1, 2, 1, 0])
    cases["negative offset"] = ([1, 0], [-1, 2, 1, 0])
    cases["no code table"] = ([], [0, 2, 1, 0])
    over = [1, 0] + [2, 0, 4] * 32  # x0 + 1 + ... : 65 instructions, 98 words, depth 2
    cases["one instruction past the tape"] = (over, [0, len(over), 2, 0])
    return cases


@pytest.mark.parametrize("name", list(_refusal_cases()))
def test_pgd_create_refuses_malformed_bytecode(name):
    from moeva2_amd._native import NativeError

    words, arg = _refusal_cases()[name]
    pool = (0, 1, 6) if name == "pool entry no feature" else (0, 1, 2)
    what = "pool index out of range" if name == "pool entry no feature" else "MV_OP_EXPR"
    with pytest.raises(NativeError, match=f"error 1: .*{what}"):
        _small_pgd(_RawProgram(words, arg, pool), D=6)


def test_pgd_create_accepts_the_same_table_when_well_formed():
    words = [3, 0, 2, 2, 1, 4, 22]  # |x0 + x1 + 2|, as test_gpu_expr's well-formed table
    pgd = _small_pgd(_RawProgram(words, [0, 7, 2, 0]), D=6, tol=0.0)
    g, losses = _grad(pgd, np.array([[1.0, -8.0, 0, 0, 0, 0]]))
    np.testing.assert_array_equal(losses[0, 2:], [9.0, 5.0])
    # loss -sum: -(d DIFF) - sgn(-5) d(x0 + x1 + 2)
    np.testing.assert_array_equal(g[0], [-1.0 + 1.0, 1.0 + 1.0, 0, 0, 0, 0])


# ---- 6. attack -------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [np.inf, 2])
def test_attack_trajectory(norm):
    from moeva2_amd._native import PGD_LOSS_CONSTRAINTS, PGD_LOSS_FLIP

    gen = _gen("lcld")
    case = gen.case
    name = f"generic lcld {HEADLINE} norm {norm}"
    t32, t64 = case.traj("candidates", HEADLINE, norm, 10)
    keep, tol = _kept_rows(name, t32, t64, MAX_EXCLUDED)
    x = case.inputs["candidates"]
    got = case.run(x, HEADLINE, norm, 10, est=gen.est)  # PGDTF2(...).generate
    _assert_matches(name, got, t32, keep, tol)
    assert not np.array_equal(got, x)
    xd = torch.from_numpy(x).cuda()
    xa = torch.empty_like(xd)
    gen.est.pgd.run(xd, xa, 10, norm, EPS, 0.1, PGD_LOSS_FLIP | PGD_LOSS_CONSTRAINTS,
                    adaptive=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, xa.cpu().numpy())


# ---- 7. row independence ---------------------------------------------------------------------
def test_small_batches():
    gen = _gen("lcld")
    case = gen.case
    x, y = case.inputs["perturbed"], case.y["perturbed"]
    full = case.run(x, HEADLINE, 2, 7, est=gen.est)
    gfull, lfull = gen.est.losses_and_gradient(x, y, "constraints+flip")
    assert not np.array_equal(full, x)
    for n in (1, 15, 16):
        np.testing.assert_array_equal(case.run(x[:n], HEADLINE, 2, 7, est=gen.est), full[:n])
        g, losses = gen.est.losses_and_gradient(x[16 - n:16], y[16 - n:16], "constraints+flip")
        np.testing.assert_array_equal(g, gfull[16 - n:16])
        np.testing.assert_array_equal(losses, lfull[16 - n:16])


def test_two_tiles_per_workgroup():
    """n = 8193: two waves own tapes in one LDS block."""
    gen = _gen("lcld")
    case = gen.case
    x, y = case.inputs["perturbed"], case.y["perturbed"]
    base = case.run(x, "constraints+flip", 2, 3, est=gen.est)
    assert not np.array_equal(base, x)
    np.testing.assert_array_equal(case.run(_tiled(x, 8193), "constraints+flip", 2, 3, est=gen.est),
                                  _tiled(base, 8193))
    g0, l0 = gen.est.losses_and_gradient(x, y, "constraints+flip")
    g, losses = gen.est.losses_and_gradient(_tiled(x, 8193), _tiled(y, 8193), "constraints+flip")
    np.testing.assert_array_equal(g, _tiled(g0, 8193))
    np.testing.assert_array_equal(losses, _tiled(l0, 8193))


# ---- 8. surface ------------------------------------------------------------------------------
def test_surface(gen):
    case = gen.case
    xf = case.s32.unscale(torch.tensor(case.inputs["perturbed"])).numpy().astype(np.float32)
    cols = gen.c.evaluate(xf, use_tensors=True)
    assert cols.dtype == np.float32 and cols.shape == (xf.shape[0], gen.c.get_nb_constraints())
    np.testing.assert_array_equal(cols, case.c.evaluate(xf, use_tensors=True))
    assert (cols > 0).any()
    np.testing.assert_array_equal(gen.c.fix_features_types(xf), xf)
