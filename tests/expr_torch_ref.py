"""Torch restatement of expression columns for the C-PGD gradient tests, shared by
tests/test_expr_grad_cpu.py and tests/test_gpu_pgd_expr.py.  Not a conftest: imported by name.

An expression tree of ``moeva2_amd.attacks.moeva2.expr`` is mapped node by node to torch ops in
fp32 or fp64 and differentiated by ``torch.autograd``.  Kink conventions are those of
tests/pgd_torch_ref.py: ``minimum`` / ``maximum`` are ``torch.where`` forms that give the whole
gradient to the first argument on a tie, ``mod`` is ``torch.remainder``, ``floor`` is
``torch.floor``, and the final ``relu(c - tol)`` passes gradient only where ``c - tol > 0``.

The module also holds the inputs both test files use: a coverage program over 8 features that
has every opcode in a position a gradient reaches or stops at, its rows of small dyadic values,
and the kink cases whose gradient entries are known exactly.
"""
import numpy as np
import torch

from moeva2_amd.attacks.moeva2 import expr as E
from moeva2_amd.attacks.moeva2.expr import (X, absolute, floor, isinf, isnan, maximum, minimum,
                                            mod, power, sum_of, where)

TOL = 2.0 ** -10  # exactly representable: the clamp adds no rounding of its own
NAN = float("nan")


def _flag(mask, like):
    return mask.to(like.dtype)


def torch_eval(node, x):
    """The value of ``node`` on the rows ``x`` (n, D), a tensor of x's dtype."""
    node = E._node(node)
    if isinstance(node, E.Feature):
        return x[:, node.index]
    if isinstance(node, E.Const):
        return torch.full((x.shape[0],), node.value, dtype=x.dtype)
    if isinstance(node, E.SumOf):
        s = torch.zeros(x.shape[0], dtype=x.dtype)
        for f in node.indices:
            s = s + x[:, f]
        return s
    if isinstance(node, E.Unary):
        a = torch_eval(node.a, x)
        return {"NEG": lambda: -a, "ABS": lambda: torch.abs(a), "FLOOR": lambda: torch.floor(a),
                "NOT": lambda: _flag(a == 0, a), "ISNAN": lambda: _flag(torch.isnan(a), a),
                "ISINF": lambda: _flag(torch.isinf(a), a)}[node.op]()
    if isinstance(node, E.Binary):
        a, b = torch_eval(node.a, x), torch_eval(node.b, x)
        return {"ADD": lambda: a + b, "SUB": lambda: a - b, "MUL": lambda: a * b,
                "DIV": lambda: a / b,
                "MIN": lambda: torch.where(b < a, b, a), "MAX": lambda: torch.where(b > a, b, a),
                "MOD": lambda: torch.remainder(a, b), "POW": lambda: torch.pow(a, b),
                "LT": lambda: _flag(a < b, a), "LE": lambda: _flag(a <= b, a),
                "GT": lambda: _flag(a > b, a), "GE": lambda: _flag(a >= b, a),
                "EQ": lambda: _flag(a == b, a), "NE": lambda: _flag(a != b, a),
                "AND": lambda: _flag((a != 0) & (b != 0), a),
                "OR": lambda: _flag((a != 0) | (b != 0), a),
                "XOR": lambda: _flag((a != 0) ^ (b != 0), a)}[node.op]()
    if isinstance(node, E.Where):
        c, a, b = (torch_eval(n, x) for n in (node.c, node.a, node.b))
        return torch.where(c != 0, a, b)
    raise TypeError(f"not an expression node: {node!r}")


def columns(exprs, x, tol=TOL):
    """relu(c - tol) of every column: (n, C)."""
    c = torch.stack([torch_eval(e, x) for e in exprs], 1)
    return torch.relu(c - torch.tensor(tol, dtype=x.dtype))


def cols_and_grad(exprs, x, dtype=torch.float64, tol=TOL):
    """(columns (n, C), d(sum of columns) / dx (n, D)) as numpy arrays, by autograd."""
    x = torch.tensor(np.asarray(x), dtype=dtype).requires_grad_(True)
    cols = columns(exprs, x, tol)
    if not cols.requires_grad:  # only comparisons and logic: autograd builds no graph at all
        return cols.detach().numpy(), np.zeros(tuple(x.shape), cols.detach().numpy().dtype)
    (g,) = torch.autograd.grad(cols.sum(), x)
    return cols.detach().numpy(), g.numpy()


def coverage_program():
    """12 columns over 8 features; every opcode at least once.  + 64 keeps a column above tol
    on every row of ``coverage_rows`` (|c| < 40 there), so its gradient is taken; the last
    column has no offset and is active on some rows only."""
    a, b, c, d, e, f, g, h = (X[i] for i in range(8))
    return [
        a + b * c - d / (absolute(e) + 1) + 64,                        # ADD MUL SUB DIV
        minimum(a, b) + maximum(c, d) + 64,                            # MIN MAX
        mod(a, absolute(e) + 1.5) + floor(b / 2) * 3 + 64,             # MOD FLOOR
        power(absolute(e) + 1, b / 2) + power(f, 2) + 64,              # POW, both operands
        -a + absolute(b - c) + 64,                                     # NEG ABS
        where(a > b, c * d, e - f) + 64,                               # WHERE GT
        where(((a < b) & (c <= d)) | ((e >= f) ^ (g == h)), a * 2, b * 3)
        + where(~(a != b), c, d) + 64,                                 # LT LE GE EQ NE AND OR XOR NOT
        where(isnan(a / g) | isinf(b / g), c, a / (absolute(g) + 0.5)) + 64,  # ISNAN ISINF
        sum_of([0, 2, 4, 6]) - sum_of([1, 3]) * 0.5 + 64,              # SUMF K
        floor(a) * 2 + (c > d) * 3 + ((a != 0) & (b != 0)) + 64,       # no gradient at all
        where(h != 0, a / (h + 0.25), b) + 64,                         # the smoothed guarded ratio
        a - b,                                                         # active on some rows
    ]


def coverage_rows(n=20):
    """n rows of halves in [-3, 3] (fixed seed), the first rows carrying ties (a == b, c == d),
    zeros (g == 0: 0 / 0 and x / 0 under isnan / isinf; h == 0) and a negative dividend."""
    rng = np.random.default_rng(5)
    x = rng.integers(-6, 7, size=(n, 8)) / 2.0
    x[0] = [1.5, 1.5, -2.0, -2.0, 0.5, 0.0, 0.0, 0.0]
    x[1] = [0.0, 2.0, 1.0, -1.0, -3.0, 1.5, 0.0, 2.5]
    x[2] = [-3.5, -1.0, 0.5, 0.5, 0.0, -2.0, 1.0, 1.0]
    return x


# (name, expression, row of 8 features, {feature: d column / d feature}); every other feature's
# entry is 0.  Each is run as a one-column program, so the entries are the whole gradient row.
_z = [0.0] * 8


def _row(**kw):
    r = list(_z)
    for k, v in kw.items():
        r["abcdefgh".index(k)] = v
    return r


KINKS = [
    ("abs at 0", absolute(X[0]) + 64, _row(a=0.0), {0: 0.0}),
    ("minimum tie", minimum(X[0], X[1]) + 64, _row(a=1.5, b=1.5), {0: 1.0, 1: 0.0}),
    ("maximum tie", maximum(X[0], X[1]) + 64, _row(a=1.5, b=1.5), {0: 1.0, 1: 0.0}),
    ("minimum second", minimum(X[0], X[1]) + 64, _row(a=2.0, b=1.5), {0: 0.0, 1: 1.0}),
    ("floor", floor(X[2]) * 2 + 64, _row(c=1.5), {2: 0.0}),
    ("comparison and logic", (X[2] > X[3]) * 3 + ((X[2] != 0) & (X[3] != 0)) + ~(X[2] == X[3]) + 64,
     _row(c=1.5, d=0.5), {2: 0.0, 3: 0.0}),
    ("mod negative dividend", mod(X[4], X[5]) + 64, _row(e=-3.5, f=2.0), {4: 1.0, 5: 2.0}),
    ("where first", where(X[6] > 0, X[6] * 2, X[6] * -3) + 64, _row(g=1.0), {6: 2.0}),
    ("where second", where(X[6] > 0, X[6] * 2, X[6] * -3) + 64, _row(g=-1.0), {6: -3.0}),
    ("power at 0", power(X[7], 2) + 64, _row(h=0.0), {7: 0.0}),
    ("guarded ratio trap", where(X[7] != 0, X[0] / X[7], 0) + 64, _row(a=1.0, h=0.0),
     {0: NAN, 7: NAN}),
    ("inactive column", X[0] - X[1], _row(a=1.0, b=1.0), {0: 0.0, 1: 0.0}),
]


def kink_expected(entries):
    want = np.zeros(8)
    for f, v in entries.items():
        want[f] = v
    return want
