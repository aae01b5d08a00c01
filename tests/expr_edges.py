"""MV_OP_EXPR programs at the edges of the tables and of k_constraintsx's row load (helper
module, not a test file): built here without a GPU, checked on the CPU by
tests/test_expr_edges_cpu.py and run on the device by tests/test_gpu_expr.py.

The engine appends the bytecode and, 8-byte aligned, the constants to the index pool after the
caller's entries (api.cpp); ``pool_words`` restates that count, which decides the size of the
constraint program's LDS region and the alignment word in front of the constants."""
import numpy as np

from moeva2_amd.attacks.moeva2 import expr as E
from moeva2_amd.attacks.moeva2.constraints import ConstraintProgram
from moeva2_amd.attacks.moeva2.expr import X, absolute, sum_of, where

INF = float("inf")
LDS_LIMIT = 160 * 1024
# maximal (256-word) columns of a D 12 program whose k_consx workspace is the last one within
# the CU's 160 KiB (csrc/kernels.h cons_lds_total, evaluated by tests/native/cons_lds_check.cpp;
# tests/test_expr_edges_cpu.py holds this number against the header)
LDS_BOUND_D = 12
LDS_BOUND_COLUMNS = 150


def program(exprs, D):
    prog = ConstraintProgram()
    for e in exprs:
        prog.add_expr(e, D)
    return prog


def pool_words(prog):
    """Entries of the engine's index pool: the caller's, the code words, one word of padding
    where those are odd in number, two words per constant."""
    n = len(prog.pool) + len(prog.expr_code)
    return n + (n & 1) + 2 * len(prog.expr_const)


def const_parity(prog):
    return (len(prog.pool) + len(prog.expr_code)) & 1


# ---------------------------------------------------------------- rows of D features
def wide_columns(D, C=70):
    """C columns over D features, no POW: every column reads the row's last features and a
    feature of each 64-feature trip of k_constraintsx's row load; a third sum a span."""
    out = []
    for c in range(C):
        a, b, z = X[(37 * c) % D], X[D - 1 - c % min(D, 5)], X[(64 * c + c) % D]
        k = 0.25 * (c % 7) - 0.5
        if c % 3 == 0:
            out.append(a - b + k * z)
        elif c % 3 == 1:
            out.append(where(b != 0, a / b, k) - z)
        else:
            span = [(c + 9 * j) % D for j in range(1 + c % 11)] + [D - 1]
            out.append(absolute(sum_of(span) - 1.5 * a))
    return out


def wide_rows(D, n, seed):
    rng = np.random.default_rng(seed)
    x = np.round(rng.uniform(-4, 4, size=(n, D)), 3)
    x[rng.random(x.shape) < 0.05] = 0.0
    return x


# ---------------------------------------------------------------- constants
def constants():
    """40 distinct bit patterns, the edge values among them (the NaN carries a payload)."""
    nan = float(np.uint64(0x7FF8000000000123).view(np.float64))
    edge = [-0.0, 0.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, INF,
            nan, 2.2250738585072014e-308, 1.0 + 2.0 ** -52, 1e-3, -1e-3]  # (tol -inf clamps -inf)
    rng = np.random.default_rng(40)
    rest = list(rng.standard_normal(40 - len(edge)) * 10.0 ** rng.integers(-30, 30, 40 - len(edge)))
    k = np.array(edge + rest, np.float64)
    assert len(set(k.view(np.uint64).tolist())) == 40
    return k


def constant_columns(odd):
    """One column per constant, each returning it untouched (a select moves the bits);
    ``odd``: a five-word column in front, so the constants start one word later."""
    cols = [where(X[0] == X[0], float(k), float(k)) for k in constants()]
    return ([X[0] - X[1]] if odd else []) + cols


# ---------------------------------------------------------------- sum_of pools
SUMF_D = 70
SUMF_SIZES = (0, 1, 64, 65, 300)


def sumf_columns():
    """sum_of over pools of 0, 1, 64, 65 and 300 entries (the last repeats features by
    necessity), one over a pool that repeats one feature, one over feature 0 alone: rows
    with x[0] = -0.0 show the leading 0.0 of the sum (0.0 + -0.0 is +0.0)."""
    rng = np.random.default_rng(65)
    pools = [list(map(int, rng.integers(1, SUMF_D, n))) for n in SUMF_SIZES]
    pools += [[3, 3, 3, 5, 3], [0]]
    return [sum_of(p) for p in pools], pools


def sumf_rows():
    rng = np.random.default_rng(66)
    x = rng.uniform(-3, 3, size=(6, SUMF_D))  # non-integer: the order of the sum shows
    x[:3, 0] = -0.0
    return x


# ---------------------------------------------------------------- the LDS bound
def maximal_column(c):
    """E.MAX_WORDS code words: a left-to-right sum of 84 features and one constant of its
    own, then - and | |; the columns differ in features and constant."""
    e = X[c % LDS_BOUND_D] + (0.125 * c + 0.0625)
    for i in range((E.MAX_WORDS - 7) // 3):
        e = e + X[(c + 5 * i) % LDS_BOUND_D]
    return absolute(-e)


def bound_columns(n):
    return [maximal_column(c) for c in range(n)]
