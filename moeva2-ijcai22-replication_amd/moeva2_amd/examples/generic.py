"""The two shipped constraint programs written as generic expressions.

``lcld_expressions()`` and ``botnet_expressions(feat_idx)`` restate, with the builder of
``moeva2_amd.attacks.moeva2.expr``, the columns of ``lcld_program`` and ``botnet_program``
(the dedicated ops of ``include/moeva_mi355x.h``): the same operands in the same order, so
on the device every generic column equals its dedicated op bit for bit.  They show how a new
dataset's constraints are written (``ExprConstraints``), and they are the input of the
generic-path tests and of ``tools/expr_speed.py``.
"""
from ..attacks.moeva2.expr import X, absolute, floor, isnan, mod, power, sum_of, where
from .botnet.botnet_constraints import MAX_IDX, MIN_IDX, SUM_IDX


def _month(f):
    """MV_OP_MONTHDIFF's month count of a yyyymm feature: floor(f / 100) * 12 + f mod 100."""
    return floor(f / 100) * 12 + mod(f, 100)


def _abs_ratio(a0, a1, a2):
    """MV_OP_ABS_RATIO: |x[a0] - x[a1] / x[a2]|."""
    return absolute(X[a0] - X[a1] / X[a2])


def lcld_expressions():
    """The 10 LCLD columns (examples/lcld/lcld_constraints.py lcld_program)."""
    # LCLD_INSTALL (0, 1, 2, 3): |x3 - x0 r (1 + r)^x1 / ((1 + r)^x1 - 1)| - k0, r = x2 / 1200
    growth = power(1 + X[2] / 1200, X[1])
    installment = ((X[0] * (X[2] / 1200)) * growth) / (growth - 1)
    # RATIO_MASKED (25, 16, 11): -1 where the denominator is 0 or the ratio is +inf or NaN
    ratio = X[16] / X[11]
    masked = where((X[11] == 0) | (ratio == float("inf")) | isnan(ratio), -1, ratio)
    return [
        absolute(X[3] - installment) - 0.099999,
        X[10] - X[14],                                     # DIFF
        X[16] - X[11],                                     # DIFF
        absolute((36 - X[1]) * (60 - X[1])),               # LCLD_TERM
        _abs_ratio(20, 0, 6),
        _abs_ratio(21, 10, 14),
        absolute(X[22] - (_month(X[7]) - _month(X[9]))),   # MONTHDIFF
        _abs_ratio(23, 11, 22),
        _abs_ratio(24, 16, 22),
        absolute(X[25] - masked),
    ]


def botnet_expressions(feat_idx: dict):
    """The 360 botnet columns (examples/botnet/botnet_constraints.py botnet_program)."""
    fi = feat_idx
    out = []
    for d in ("s", "d"):  # ABS_SUMDIFF: |sum(first) - sum(second)|
        first = fi[f"icmp_sum_{d}_idx"] + fi[f"udp_sum_{d}_idx"] + fi[f"tcp_sum_{d}_idx"]
        second = fi[f"bytes_in_sum_{d}_idx"] + fi[f"bytes_out_sum_{d}_idx"]
        out.append(absolute(sum_of(first) - sum_of(second)))
    for bo, po in (("bytes_out_sum_s_idx", "pkts_out_sum_s_idx"),
                   ("bytes_out_sum_d_idx", "pkts_out_sum_d_idx")):
        for j in range(len(bo) - 2):  # RATIO_SAFE: (b != 0 ? a / b : 0) - 1500
            a, b = X[fi[bo][j]], X[fi[po][j]]
            out.append(where(b != 0, a / b, 0) - 1500)
    keys = list(fi.keys())
    for upper, lower in ((SUM_IDX, MAX_IDX), (SUM_IDX, MIN_IDX), (MAX_IDX, MIN_IDX)):
        for i in range(len(upper)):
            up_k, lo_k = keys[upper[i]], keys[lower[i]]
            for j in range(len(fi[up_k])):
                out.append(X[fi[lo_k][j]] - X[fi[up_k][j]])  # DIFF
    return out
