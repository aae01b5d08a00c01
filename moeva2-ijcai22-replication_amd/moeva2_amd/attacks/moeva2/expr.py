"""User-defined constraint expressions: builder, bytecode compiler, numpy evaluator.

A constraint column is an arithmetic expression over the ML-space row, written with the
builder below (``X[i]``, Python numbers, ``+ - * /``, comparisons, ``& | ^ ~`` and the
functions ``absolute, minimum, maximum, floor, mod, power, where, isnan, isinf, sum_of``).
``compile_expr`` turns it into the postfix bytecode of ``MV_OP_EXPR``
(``include/moeva_mi355x.h``), which the device interprets in fp64; ``evaluate_numpy`` is the
CPU statement of the same program: the same operations in the same order on numpy arrays,
so a constraint class can be checked without a GPU.  This module has no GPU imports.

Semantics are numpy's on fp64: comparisons give 1.0 / 0.0, ``& | ^ ~`` act on truth values
(non-zero is true, NaN included), ``minimum`` / ``maximum`` propagate NaN, ``mod`` is
``np.mod`` (the result takes the divisor's sign), ``/`` is IEEE (x / 0 is +-inf or NaN and
does not trap), ``where(c, a, b)`` selects ``a`` where ``c != 0``.

Instruction set (int32 words, postfix, operands inline; left operand emitted first):

    X f (1)       push feature f                K i (2)      push constant i
    SUMF o0 o1 (3) push 0.0 + x[pool[o0]] + ... + x[pool[o1 - 1]]   (left to right)
    ADD SUB MUL DIV MIN MAX MOD POW (4..11)     b = pop, a = pop, push a . b
    LT LE GT GE EQ NE (12..17)                  ... push 1.0 / 0.0
    AND OR XOR (18..20)                         ... on (a != 0), (b != 0)
    NEG ABS FLOOR NOT ISNAN ISINF (21..26)      a = pop, push f(a)
    WHERE (27)                                  b = pop, a = pop, c = pop, push c != 0 ? a : b

Limits (the device's, checked again by ``mv_engine_create``): operand stack depth
``MAX_DEPTH`` = 8, ``MAX_WORDS`` = 256 code words per column.

C-PGD runs the same bytecode as a tensor-path column (``ExprConstraints.tensor_program``): the
device interprets it in fp32 and differentiates it with a reverse sweep over a tape of every
instruction's value, so a tensor-path column has at most ``MAX_TAPE`` = 64 instructions
(checked again by ``mv_pgd_create``).  ``evaluate_grad_numpy`` states that computation on the
CPU: the derivative rules, autograd's with TF's kinks, are listed there.
"""
from __future__ import annotations

import numbers
from typing import Iterable, List, Sequence

import numpy as np

MAX_DEPTH = 8
MAX_WORDS = 256
MAX_TAPE = 64

OPCODES = dict(X=1, K=2, SUMF=3, ADD=4, SUB=5, MUL=6, DIV=7, MIN=8, MAX=9, MOD=10, POW=11,
               LT=12, LE=13, GT=14, GE=15, EQ=16, NE=17, AND=18, OR=19, XOR=20,
               NEG=21, ABS=22, FLOOR=23, NOT=24, ISNAN=25, ISINF=26, WHERE=27)
N_OPERANDS = {OPCODES["X"]: 1, OPCODES["K"]: 1, OPCODES["SUMF"]: 2}  # inline operand words


def _truth(a):
    return np.asarray(a) != 0


def _f64(mask):
    return np.asarray(mask).astype(np.float64)


_NP_BINARY = {
    "ADD": lambda a, b, p: a + b, "SUB": lambda a, b, p: a - b, "MUL": lambda a, b, p: a * b,
    "DIV": lambda a, b, p: a / b, "MIN": lambda a, b, p: np.minimum(a, b),
    "MAX": lambda a, b, p: np.maximum(a, b), "MOD": lambda a, b, p: np.mod(a, b),
    "POW": lambda a, b, p: np.asarray(p(a, b), np.float64),
    "LT": lambda a, b, p: _f64(a < b), "LE": lambda a, b, p: _f64(a <= b),
    "GT": lambda a, b, p: _f64(a > b), "GE": lambda a, b, p: _f64(a >= b),
    "EQ": lambda a, b, p: _f64(a == b), "NE": lambda a, b, p: _f64(a != b),
    "AND": lambda a, b, p: _f64(_truth(a) & _truth(b)),
    "OR": lambda a, b, p: _f64(_truth(a) | _truth(b)),
    "XOR": lambda a, b, p: _f64(_truth(a) ^ _truth(b)),
}
_NP_UNARY = {
    "NEG": lambda a: -a, "ABS": np.absolute, "FLOOR": np.floor,
    "NOT": lambda a: _f64(~_truth(a)), "ISNAN": lambda a: _f64(np.isnan(a)),
    "ISINF": lambda a: _f64(np.isinf(a)),
}


def _node(v) -> "Node":
    if isinstance(v, Node):
        return v
    if isinstance(v, (bool, np.bool_)):
        return Const(1.0 if v else 0.0)
    if isinstance(v, numbers.Real):
        return Const(float(v))
    raise TypeError(f"{v!r} is not an expression (use X[i], numbers and the functions of "
                    "moeva2_amd.attacks.moeva2.expr)")


class Node:
    """An expression; combine with + - * / unary-, comparisons, & | ^ ~."""

    def __add__(self, o): return Binary("ADD", self, o)
    def __radd__(self, o): return Binary("ADD", o, self)
    def __sub__(self, o): return Binary("SUB", self, o)
    def __rsub__(self, o): return Binary("SUB", o, self)
    def __mul__(self, o): return Binary("MUL", self, o)
    def __rmul__(self, o): return Binary("MUL", o, self)
    def __truediv__(self, o): return Binary("DIV", self, o)
    def __rtruediv__(self, o): return Binary("DIV", o, self)
    def __neg__(self): return Unary("NEG", self)
    def __lt__(self, o): return Binary("LT", self, o)
    def __le__(self, o): return Binary("LE", self, o)
    def __gt__(self, o): return Binary("GT", self, o)
    def __ge__(self, o): return Binary("GE", self, o)
    def __eq__(self, o): return Binary("EQ", self, o)  # noqa: D105
    def __ne__(self, o): return Binary("NE", self, o)
    def __and__(self, o): return Binary("AND", self, o)
    def __rand__(self, o): return Binary("AND", o, self)
    def __or__(self, o): return Binary("OR", self, o)
    def __ror__(self, o): return Binary("OR", o, self)
    def __xor__(self, o): return Binary("XOR", self, o)
    def __rxor__(self, o): return Binary("XOR", o, self)
    def __invert__(self): return Unary("NOT", self)

    __hash__ = object.__hash__

    def __bool__(self):
        raise TypeError("an expression has no truth value: use & | ^ ~ and where(), not "
                        "and / or / not / if")


class Feature(Node):
    def __init__(self, index):
        if not isinstance(index, numbers.Integral):
            raise TypeError("X[i] takes one integer feature index")
        self.index = int(index)


class Const(Node):
    def __init__(self, value: float):
        self.value = float(value)


class SumOf(Node):
    def __init__(self, indices: Iterable[int]):
        self.indices = [int(i) for i in indices]


class Unary(Node):
    def __init__(self, op: str, a):
        self.op, self.a = op, _node(a)


class Binary(Node):
    def __init__(self, op: str, a, b):
        self.op, self.a, self.b = op, _node(a), _node(b)


class Where(Node):
    def __init__(self, c, a, b):
        self.c, self.a, self.b = _node(c), _node(a), _node(b)


class _Features:
    """``X[i]``: feature i of the ML-space row."""

    def __getitem__(self, index) -> Feature:
        return Feature(index)


X = _Features()


def absolute(a): return Unary("ABS", a)
def floor(a): return Unary("FLOOR", a)
def isnan(a): return Unary("ISNAN", a)
def isinf(a): return Unary("ISINF", a)
def minimum(a, b): return Binary("MIN", a, b)
def maximum(a, b): return Binary("MAX", a, b)
def mod(a, b): return Binary("MOD", a, b)
def power(a, b): return Binary("POW", a, b)
def where(c, a, b): return Where(c, a, b)


def sum_of(indices: Iterable[int]) -> SumOf:
    """The sum of the listed features, added left to right starting from 0.0 (the device's
    and ``evaluate_numpy``'s order).  ``np.sum`` adds pairwise, so for non-integer features
    it can differ from this sum in the last bit."""
    return SumOf(indices)


def compile_expr(node, n_features: int = None):
    """Expression -> (code int32 words, constants fp64, pool int32 feature indices).

    ``K`` operands index the returned constants and ``SUMF`` operands the returned pool
    (``ConstraintProgram.add_expr`` rebases both into the program's tables).  Raises
    ValueError for an empty expression, a feature index outside [0, n_features) (negative
    ones always), more than ``MAX_WORDS`` code words or a stack deeper than ``MAX_DEPTH``.
    """
    if node is None or (isinstance(node, (list, tuple, str)) and len(node) == 0):
        raise ValueError("empty expression")
    node = _node(node)
    code: List[int] = []
    consts: List[float] = []
    pool: List[int] = []
    depth = [0, 0]  # current, maximum

    def feat(f):
        if f < 0 or (n_features is not None and f >= n_features):
            raise ValueError(f"feature index {f} outside [0, "
                             f"{'D' if n_features is None else n_features})")
        return f

    def push():
        depth[0] += 1
        depth[1] = max(depth[1], depth[0])

    def emit(n):
        if isinstance(n, Feature):
            code.extend((OPCODES["X"], feat(n.index)))
            push()
        elif isinstance(n, Const):
            bits = np.float64(n.value).view(np.uint64)
            for i, c in enumerate(consts):  # one table entry per distinct bit pattern
                if np.float64(c).view(np.uint64) == bits:
                    break
            else:
                i = len(consts)
                consts.append(n.value)
            code.extend((OPCODES["K"], i))
            push()
        elif isinstance(n, SumOf):
            o0 = len(pool)
            pool.extend(feat(f) for f in n.indices)
            code.extend((OPCODES["SUMF"], o0, len(pool)))
            push()
        elif isinstance(n, Unary):
            emit(n.a)
            code.append(OPCODES[n.op])
        elif isinstance(n, Binary):
            emit(n.a)
            emit(n.b)
            code.append(OPCODES[n.op])
            depth[0] -= 1
        elif isinstance(n, Where):
            emit(n.c)
            emit(n.a)
            emit(n.b)
            code.append(OPCODES["WHERE"])
            depth[0] -= 2
        else:
            raise TypeError(f"not an expression node: {n!r}")

    emit(node)
    if len(code) > MAX_WORDS:
        raise ValueError(f"expression compiles to {len(code)} code words (limit {MAX_WORDS})")
    if depth[1] > MAX_DEPTH:
        raise ValueError(f"expression needs a stack of {depth[1]} (limit {MAX_DEPTH})")
    return (np.asarray(code, np.int32), np.asarray(consts, np.float64),
            np.asarray(pool, np.int32))


def stack_depth(code: Sequence[int]) -> int:
    """Maximum operand-stack depth of compiled code words."""
    d = m = 0
    pc = 0
    code = [int(w) for w in code]
    while pc < len(code):
        op = code[pc]
        pc += 1 + N_OPERANDS.get(op, 0)
        if op <= OPCODES["SUMF"]:
            d += 1
        elif op <= OPCODES["XOR"]:
            d -= 1
        elif op == OPCODES["WHERE"]:
            d -= 2
        m = max(m, d)
    return m


def _eval(n: Node, x: np.ndarray, pow_fn):
    if isinstance(n, Feature):
        return x[:, n.index]
    if isinstance(n, Const):
        return np.full(x.shape[0], n.value)
    if isinstance(n, SumOf):
        s = np.zeros(x.shape[0])
        for f in n.indices:
            s = s + x[:, f]
        return s
    if isinstance(n, Unary):
        return _NP_UNARY[n.op](_eval(n.a, x, pow_fn))
    if isinstance(n, Binary):
        a = _eval(n.a, x, pow_fn)
        b = _eval(n.b, x, pow_fn)
        return _NP_BINARY[n.op](a, b, pow_fn)
    if isinstance(n, Where):
        c = _eval(n.c, x, pow_fn)
        a = _eval(n.a, x, pow_fn)
        b = _eval(n.b, x, pow_fn)
        return np.where(c != 0, a, b)
    raise TypeError(f"not an expression node: {n!r}")


def evaluate_numpy(exprs, x, tol: float = 1e-3, pow_fn=np.power) -> np.ndarray:
    """The columns ``exprs`` on the rows ``x`` (n, D) -> (n, C) fp64: every operation of the
    bytecode in its order, then ``Constraints.evaluate``'s clamp (values <= tol become 0;
    ``tol=None`` returns the raw values).
    ``pow_fn`` stands in for the device's ``pow`` (default ``np.power``)."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    out = np.empty((x.shape[0], len(exprs)), np.float64)
    with np.errstate(all="ignore"):
        for c, e in enumerate(exprs):
            if e is None:
                raise ValueError("empty expression")
            out[:, c] = _eval(_node(e), x, pow_fn)
        if tol is not None:
            out[out <= tol] = 0.0
    return out


def decode(code: Sequence[int]):
    """Compiled code words -> one tuple per instruction ``(op, a0, a1, left, cond, start,
    skip)``, the table ``mv_pgd_create`` builds for the reverse sweep: ``left`` is the ordinal
    (index in this list) of the instruction that produced the left operand (``a`` of a binary
    operator and of WHERE; the right operand is always the previous instruction), ``cond``
    the one that produced WHERE's condition, ``start`` the first ordinal of the instruction's
    subtree, and ``skip`` marks the instructions no gradient passes through: comparisons,
    AND OR XOR NOT ISNAN ISINF and the root of a WHERE condition."""
    code = [int(w) for w in code]
    out, stack, pc = [], [], 0
    while pc < len(code):
        op, i = code[pc], len(out)
        pc += 1
        a0 = a1 = left = cond = 0
        start, skip = i, False
        if op <= OPCODES["SUMF"]:
            a0 = code[pc]
            a1 = code[pc + 1] if op == OPCODES["SUMF"] else 0
            pc += N_OPERANDS[op]
        elif op <= OPCODES["XOR"]:
            stack.pop()
            left, start = stack.pop()
            skip = op >= OPCODES["LT"]
        elif op <= OPCODES["ISINF"]:
            start = stack.pop()[1]
            skip = op >= OPCODES["NOT"]
        else:
            stack.pop()
            left = stack.pop()[0]
            cond, start = stack.pop()
            out[cond] = out[cond][:6] + (True,)
        stack.append((i, start))
        out.append((op, a0, a1, left, cond, start, skip))
    return out


def tape_length(code: Sequence[int]) -> int:
    """Instructions of compiled code words: the column's tape length in C-PGD."""
    return len(decode(code))


def evaluate_grad_numpy(exprs, x, tol: float = 1e-3, dtype=np.float64, pow_fn=np.power):
    """What C-PGD computes of the columns ``exprs`` on the rows ``x`` (n, D), in ``dtype``:
    ``(cols (n, C), grad (n, D))`` with ``cols = max(c - tol, 0)`` (NaN stays NaN) and
    ``grad = d(sum of cols) / dx``.

    The device's operations in the device's order: every column's bytecode forward with each
    instruction's value kept on a tape; then, on the rows where ``c - tol > 0``, the
    instructions backwards with an adjoint stack that starts from 1 -- an operator pops its
    adjoint ``g``, reads its operands ``a, b`` from the tape and pushes their adjoints, a leaf
    ``X f`` adds ``g`` to ``grad[:, f]`` (``sum_of``: to every listed feature, in order), a
    constant drops it.  Columns in ascending order, all into one gradient row.  Rules:

        a + b: g, g      a - b: g, -g      a * b: g b, g a      a / b: g / b, -(g a) / (b b)
        minimum: all of g to b if b < a else to a (the first on a tie); maximum: b > a
        mod(a, b): g, -g floor(a / b)      power(a, b): g (b a^(b-1)), g (a^b log a), the
        latter 0 where a == 0 and b >= 0   -a: -g      absolute: g sgn(a), sgn(0) = 0
        floor: 0      where(c, a, b): g to a where c != 0, else to b

    A zero adjoint is propagated arithmetically, as autograd does, so ``where(b != 0, a / b,
    0)`` has a NaN derivative for ``a`` at ``b = 0``; write the smoothed ``a / (b + alpha)``
    as the reference's tensor paths do.  Comparisons, ``& | ^ ~``, ``isnan``, ``isinf`` and
    the condition of ``where`` are outside the differentiated graph: nothing below them is
    visited.  ``pow_fn`` stands in for the device's ``powf``.  No GPU, no torch."""
    dt = np.dtype(dtype).type
    x = np.atleast_2d(np.asarray(x, dt))
    n, D = x.shape
    cols = np.empty((n, len(exprs)), dt)
    grad = np.zeros((n, D), dt)
    one, zero = dt(1), dt(0)
    O = OPCODES

    def flag(mask):
        return np.where(mask, one, zero)

    def sgn(a):
        return np.where(a > 0, one, np.where(a < 0, -one, zero))

    with np.errstate(all="ignore"):
        for c, e in enumerate(exprs):
            if e is None:
                raise ValueError("empty expression")
            code, consts, pool = compile_expr(e, D)
            ins = decode(code)
            if len(ins) > MAX_TAPE:
                raise ValueError(f"column {c} has {len(ins)} instructions (limit {MAX_TAPE})")
            consts = consts.astype(dt)
            tape, st = [], []
            for op, a0, a1, _l, _c, _s, _k in ins:
                if op == O["X"]:
                    v = x[:, a0]
                elif op == O["K"]:
                    v = np.full(n, consts[a0], dt)
                elif op == O["SUMF"]:
                    v = np.zeros(n, dt)
                    for f in pool[a0:a1]:
                        v = v + x[:, f]
                elif op <= O["XOR"]:
                    b = st.pop()
                    a = st.pop()
                    if op == O["ADD"]: v = a + b
                    elif op == O["SUB"]: v = a - b
                    elif op == O["MUL"]: v = a * b
                    elif op == O["DIV"]: v = a / b
                    elif op == O["MIN"]: v = np.where((a < b) | (a != a), a, b)
                    elif op == O["MAX"]: v = np.where((a > b) | (a != a), a, b)
                    elif op == O["MOD"]: v = np.mod(a, b)
                    elif op == O["POW"]: v = np.asarray(pow_fn(a, b), dt)
                    elif op == O["LT"]: v = flag(a < b)
                    elif op == O["LE"]: v = flag(a <= b)
                    elif op == O["GT"]: v = flag(a > b)
                    elif op == O["GE"]: v = flag(a >= b)
                    elif op == O["EQ"]: v = flag(a == b)
                    elif op == O["NE"]: v = flag(a != b)
                    elif op == O["AND"]: v = flag((a != 0) & (b != 0))
                    elif op == O["OR"]: v = flag((a != 0) | (b != 0))
                    else: v = flag((a != 0) ^ (b != 0))
                elif op <= O["ISINF"]:
                    a = st.pop()
                    if op == O["NEG"]: v = -a
                    elif op == O["ABS"]: v = np.absolute(a)
                    elif op == O["FLOOR"]: v = np.floor(a)
                    elif op == O["NOT"]: v = flag(a == 0)
                    elif op == O["ISNAN"]: v = flag(a != a)
                    else: v = flag(np.isinf(a))
                else:
                    b = st.pop()
                    a = st.pop()
                    cnd = st.pop()
                    v = np.where(cnd != 0, a, b)
                v = np.asarray(v, dt)
                st.append(v)
                tape.append(v)
            ct = st[0] - dt(tol)
            active = ct > 0
            cols[:, c] = np.where(active, ct, np.where(ct != ct, ct, zero))
            gs = [np.full(n, one, dt)]
            i = len(ins) - 1
            while i >= 0:
                op, a0, a1, left, cond, start, skip = ins[i]
                g = gs.pop()
                if skip:
                    i = start - 1
                    continue
                if op == O["X"]:
                    grad[:, a0] = grad[:, a0] + np.where(active, g, zero)
                elif op == O["SUMF"]:
                    for f in pool[a0:a1]:
                        grad[:, f] = grad[:, f] + np.where(active, g, zero)
                elif op == O["K"]:
                    pass
                elif op <= O["POW"]:
                    a, b = tape[left], tape[i - 1]
                    if op == O["ADD"]: ga, gb = g, g
                    elif op == O["SUB"]: ga, gb = g, -g
                    elif op == O["MUL"]: ga, gb = g * b, g * a
                    elif op == O["DIV"]: ga, gb = g / b, -(g * a) / (b * b)
                    elif op == O["MIN"]: ga, gb = np.where(b < a, zero, g), np.where(b < a, g, zero)
                    elif op == O["MAX"]: ga, gb = np.where(b > a, zero, g), np.where(b > a, g, zero)
                    elif op == O["MOD"]: ga, gb = g, -g * np.floor(a / b)
                    else:
                        ga = g * (b * np.asarray(pow_fn(a, b - one), dt))
                        gb = np.where((a == 0) & (b >= 0), zero, g * (tape[i] * np.log(a)))
                    gs.append(np.asarray(ga, dt))
                    gs.append(np.asarray(gb, dt))
                elif op <= O["FLOOR"]:
                    a = tape[i - 1]
                    gs.append(-g if op == O["NEG"] else
                              (g * sgn(a) if op == O["ABS"] else np.zeros(n, dt)))
                else:
                    cnd = tape[cond]
                    gs.append(np.zeros(n, dt))
                    gs.append(np.where(cnd != 0, g, zero))
                    gs.append(np.where(cnd != 0, zero, g))
                i -= 1
    return cols, grad
