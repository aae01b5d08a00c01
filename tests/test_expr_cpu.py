"""Generic constraint expressions on the CPU (moeva2_amd/attacks/moeva2/expr.py): the shipped
LCLD and botnet programs written with the builder reproduce the reference-generated goldens,
every instruction follows numpy on its edge inputs, and the compiled words mean what
``evaluate_numpy`` computes."""
import json
import os

import numpy as np
import pytest

from conftest import RES
from moeva2_amd.attacks.moeva2 import expr as E
from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram
from moeva2_amd.attacks.moeva2.expr import (X, absolute, floor, isinf, isnan, maximum, minimum,
                                            mod, power, sum_of, where)
from moeva2_amd.examples.generic import botnet_expressions, lcld_expressions

NAN, INF = float("nan"), float("inf")


def feat_idx():
    with open(os.path.join(RES, "data", "botnet", "feat_idx.json")) as f:
        return json.load(f)


def edge_rows():
    """Rows over 6 features that hit every instruction's edges: zeros of both signs (0/0,
    x/0), NaN and infinities on either side, negative operands for mod and floor, ties."""
    vals = [0.0, -0.0, 1.0, -1.0, 2.5, -2.5, 7.0, -7.0, 1e300, -1e300, INF, -INF, NAN, 0.5, -0.5,
            3.0]
    rng = np.random.default_rng(0)
    rows = [[a, b, 1.0, -3.0, 0.0, NAN] for a in vals for b in vals]
    rows += rng.choice(vals, size=(200, 6)).tolist()
    return np.array(rows)


def coverage_program():
    """Every instruction at least once: (expression, the direct numpy statement)."""
    t = lambda m: np.asarray(m).astype(np.float64)  # noqa: E731
    a, b, c = X[0], X[1], X[5]
    return [
        (a + b, lambda x: x[:, 0] + x[:, 1]),
        (a - b, lambda x: x[:, 0] - x[:, 1]),
        (a * b, lambda x: x[:, 0] * x[:, 1]),
        (a / b, lambda x: x[:, 0] / x[:, 1]),
        (2.0 / a, lambda x: 2.0 / x[:, 0]),
        (-a, lambda x: -x[:, 0]),
        (minimum(a, b), lambda x: np.minimum(x[:, 0], x[:, 1])),
        (maximum(a, b), lambda x: np.maximum(x[:, 0], x[:, 1])),
        (minimum(a, c), lambda x: np.minimum(x[:, 0], x[:, 5])),
        (maximum(c, a), lambda x: np.maximum(x[:, 5], x[:, 0])),
        (mod(a, b), lambda x: np.mod(x[:, 0], x[:, 1])),
        (mod(a, X[3]), lambda x: np.mod(x[:, 0], x[:, 3])),
        (floor(a), lambda x: np.floor(x[:, 0])),
        (floor(a / 3), lambda x: np.floor(x[:, 0] / 3)),
        (absolute(a), lambda x: np.absolute(x[:, 0])),
        (a < b, lambda x: t(x[:, 0] < x[:, 1])),
        (a <= b, lambda x: t(x[:, 0] <= x[:, 1])),
        (a > b, lambda x: t(x[:, 0] > x[:, 1])),
        (a >= b, lambda x: t(x[:, 0] >= x[:, 1])),
        (a == b, lambda x: t(x[:, 0] == x[:, 1])),
        (a != b, lambda x: t(x[:, 0] != x[:, 1])),
        (a < c, lambda x: t(x[:, 0] < x[:, 5])),
        (c == c, lambda x: t(x[:, 5] == x[:, 5])),
        (c != c, lambda x: t(x[:, 5] != x[:, 5])),
        ((a < b) & (b > 0), lambda x: t((x[:, 0] < x[:, 1]) & (x[:, 1] > 0))),
        ((a < b) | (b > 0), lambda x: t((x[:, 0] < x[:, 1]) | (x[:, 1] > 0))),
        ((a < b) ^ (b > 0), lambda x: t((x[:, 0] < x[:, 1]) ^ (x[:, 1] > 0))),
        (~(a < b), lambda x: t(~(x[:, 0] < x[:, 1]))),
        (isnan(a / b), lambda x: t(np.isnan(x[:, 0] / x[:, 1]))),
        (isinf(a / b), lambda x: t(np.isinf(x[:, 0] / x[:, 1]))),
        (where(a > b, a, b), lambda x: np.where(x[:, 0] > x[:, 1], x[:, 0], x[:, 1])),
        (where(a, b, c), lambda x: np.where(x[:, 0] != 0, x[:, 1], x[:, 5])),
        (where(c, a, b), lambda x: np.where(x[:, 5] != 0, x[:, 0], x[:, 1])),
        (sum_of([0, 1, 2, 3]), lambda x: ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]),
        (sum_of([]) + a, lambda x: 0.0 + x[:, 0]),
        (1 - (a - 2) * 3, lambda x: 1 - (x[:, 0] - 2) * 3),
    ]


POW_COLUMN = (power(absolute(X[0]), X[2] / 2 + X[4]),
              lambda x: np.power(np.absolute(x[:, 0]), x[:, 2] / 2 + x[:, 4]))


def interpret(code, consts, pool, x, pow_fn=np.power):
    """The bytecode's meaning in a few lines: a stack of numpy columns."""
    st, pc, code = [], 0, [int(w) for w in code]
    f = lambda m: np.asarray(m).astype(np.float64)  # noqa: E731
    binary = {4: np.add, 5: np.subtract, 6: np.multiply, 7: np.divide, 8: np.minimum,
              9: np.maximum, 10: np.mod, 11: pow_fn, 12: np.less, 13: np.less_equal,
              14: np.greater, 15: np.greater_equal, 16: np.equal, 17: np.not_equal,
              18: lambda a, b: (a != 0) & (b != 0), 19: lambda a, b: (a != 0) | (b != 0),
              20: lambda a, b: (a != 0) ^ (b != 0)}
    unary = {21: np.negative, 22: np.absolute, 23: np.floor, 24: lambda a: a == 0, 25: np.isnan,
             26: np.isinf}
    while pc < len(code):
        op = code[pc]
        pc += 1
        if op == 1:
            st.append(x[:, code[pc]])
            pc += 1
        elif op == 2:
            st.append(np.full(x.shape[0], consts[code[pc]]))
            pc += 1
        elif op == 3:
            s = np.zeros(x.shape[0])
            for q in range(code[pc], code[pc + 1]):
                s = s + x[:, pool[q]]
            st.append(s)
            pc += 2
        elif op in binary:
            b, a = st.pop(), st.pop()
            st.append(f(binary[op](a, b)))
        elif op in unary:
            st.append(f(unary[op](st.pop())))
        else:
            assert op == 27
            b, a, c = st.pop(), st.pop(), st.pop()
            st.append(np.where(c != 0, a, b))
    assert len(st) == 1
    return st[0]


@pytest.mark.parametrize("name", ["lcld", "botnet"])
def test_generic_programs_match_reference_goldens(golden, name):
    d = golden(f"{name}_constraints.npz")
    exprs = lcld_expressions() if name == "lcld" else botnet_expressions(feat_idx())
    g = E.evaluate_numpy(exprs, d["x"])
    assert g.shape == d["g"].shape
    np.testing.assert_array_equal(g > 0, d["g"] > 0)  # satisfied masks: exact
    np.testing.assert_allclose(g, d["g"], rtol=1e-13, atol=0)


def test_every_instruction_equals_numpy_on_edges():
    x = edge_rows()
    prog = coverage_program() + [POW_COLUMN]
    used = set()
    for e, _ in prog:
        code = [int(w) for w in E.compile_expr(e, x.shape[1])[0]]
        pc = 0
        while pc < len(code):
            used.add(code[pc])
            pc += 1 + E.N_OPERANDS.get(code[pc], 0)
    assert used == set(E.OPCODES.values())
    # the clamp off: every value is compared, negative ones too
    got = E.evaluate_numpy([e for e, _ in prog], x, tol=None)
    with np.errstate(all="ignore"):
        for c, (_, direct) in enumerate(prog):
            np.testing.assert_array_equal(got[:, c], direct(x), err_msg=f"column {c}")
    # the edges are really there
    q = got[:, 3]
    assert np.isnan(q).any() and (q == INF).any() and (q == -INF).any()
    assert np.isnan(got[:, 6]).any() and np.isnan(got[:, 32]).any()


def test_tol_clamp():
    x = np.array([[0.5e-3, 1e-3, 2e-3, -1.0, NAN, 0.0]])
    g = E.evaluate_numpy([X[0], X[1], X[2], X[3], X[4]], x)
    np.testing.assert_array_equal(g, [[0.0, 0.0, 2e-3, 0.0, NAN]])


@pytest.mark.parametrize("which", ["coverage", "lcld", "botnet"])
def test_compiled_words_mean_what_evaluate_numpy_computes(golden, which):
    if which == "coverage":
        x, exprs = edge_rows(), [e for e, _ in coverage_program()] + [POW_COLUMN[0]]
    else:
        x = golden(f"{which}_constraints.npz")["x"]
        exprs = lcld_expressions() if which == "lcld" else botnet_expressions(feat_idx())
    ref = E.evaluate_numpy(exprs, x, tol=None)
    # through the program builder: operands rebased into the program's tables
    prog = ConstraintProgram()
    prog.add_sumdiff([0, 1], [2])  # a dedicated column first, so every offset is non-zero
    for e in exprs:
        prog.add_expr(e, x.shape[1])
    code, arg, karg, pool = prog.arrays()
    words, consts = prog.expr_arrays()
    assert words.dtype == np.int32 and consts.dtype == np.float64
    with np.errstate(all="ignore"):
        for c in range(len(exprs)):
            assert code[c + 1] == 16
            off, n, depth, _ = arg[c + 1]
            assert 1 <= depth <= E.MAX_DEPTH and 1 <= n <= E.MAX_WORDS
            assert depth == E.stack_depth(words[off:off + n])
            np.testing.assert_array_equal(interpret(words[off:off + n], consts, pool, x),
                                          ref[:, c], err_msg=f"column {c}")


def test_operands_are_emitted_left_first():
    code, consts, pool = E.compile_expr((X[3] - 2) / where(X[1], X[4], sum_of([5, 0])))
    O = E.OPCODES
    assert list(code) == [O["X"], 3, O["K"], 0, O["SUB"], O["X"], 1, O["X"], 4, O["SUMF"], 0, 2,
                          O["WHERE"], O["DIV"]]
    assert list(consts) == [2.0] and list(pool) == [5, 0]


def _deep(n):
    """A right-nested sum whose evaluation holds n values on the stack."""
    e = X[0]
    for _ in range(n - 1):
        e = X[0] + e
    return e


def _long(n_ops):
    e = X[0]
    for _ in range(n_ops):
        e = e + X[0]  # three words per step, depth 2
    return e


def test_limits_and_value_errors():
    assert E.stack_depth(E.compile_expr(_deep(E.MAX_DEPTH))[0]) == E.MAX_DEPTH
    with pytest.raises(ValueError, match="stack"):
        E.compile_expr(_deep(E.MAX_DEPTH + 1))
    n_fit = (E.MAX_WORDS - 2) // 3
    assert len(E.compile_expr(_long(n_fit))[0]) == 2 + 3 * n_fit <= E.MAX_WORDS
    with pytest.raises(ValueError, match="words"):
        E.compile_expr(_long(n_fit + 1))
    with pytest.raises(ValueError, match="feature index"):
        E.compile_expr(X[-1] + 1)
    with pytest.raises(ValueError, match="feature index"):
        E.compile_expr(X[3] + X[7], n_features=7)
    with pytest.raises(ValueError, match="feature index"):
        E.compile_expr(sum_of([0, 9]), n_features=9)
    E.compile_expr(X[6], n_features=7)
    for empty in (None, [], ()):
        with pytest.raises(ValueError, match="empty"):
            E.compile_expr(empty)
    with pytest.raises(ValueError):
        ConstraintProgram().add_expr(X[12], 12)
    with pytest.raises(TypeError):
        bool(X[0] < X[1])  # `and` / `or` / `if` on expressions are mistakes, not silently true


def test_mixed_program_keeps_the_four_arrays():
    prog = ConstraintProgram()
    prog.add("DIFF", (1, 2))
    prog.add_expr(where(X[0] > 1, X[1], 0.5) - 0.5, 6)
    prog.add_sumdiff([0, 1, 2], [3, 4])
    prog.add_expr(absolute(sum_of([4, 5]) - 0.5), 6)
    arrays = prog.arrays()
    assert len(arrays) == 4 and len(prog) == 4
    code, arg, karg, pool = arrays
    assert list(code) == [1, 16, 3, 16]
    assert arg.shape == (4, 4) and karg.shape == (4, 2)
    assert list(pool) == [0, 1, 2, 3, 4, 4, 5]  # ABS_SUMDIFF's lists, then sum_of's
    words, consts = prog.expr_arrays()
    assert list(consts) == [1.0, 0.5]  # one table entry per distinct constant
    assert arg[1][0] == 0 and arg[3][0] == arg[1][1] and arg[1][1] + arg[3][1] == len(words)
    O = E.OPCODES
    assert list(words[arg[3][0]:]) == [O["SUMF"], 5, 7, O["K"], 1, O["SUB"], O["ABS"]]


def test_expr_constraints_class_routes_to_the_engine():
    from moeva2_amd.attacks.moeva2.constraints import ExprConstraints
    from moeva2_amd.problem import build_device_program, has_device_program

    feat = os.path.join(RES, "data", "lcld", "features.csv")
    c = ExprConstraints(feat, feat.replace("features", "constraints"), lcld_expressions())
    assert has_device_program(c) and c.get_nb_constraints() == 10
    dp = build_device_program(c)
    assert list(dp.op_code) == [16] * 10 and dp.expr_code.size == sum(dp.op_arg[:, 1])
    with pytest.raises(ValueError, match="feature index"):
        ExprConstraints(feat, feat.replace("features", "constraints"), [X[dp.D] - 1])
